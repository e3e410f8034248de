// inference.hpp -- gpc::inference::{InferenceSettings, Forest} on MI355X.
//
// Host-side mirror of the reference's lib/gpc/inference.hpp: same class, method and field
// names, same by-value conventions, same messages on stdout, so that a caller such as
// samples/sparsematch.cpp compiles unchanged.  Every hot method forwards to the C ABI of
// libgpc_hip.so (include/gpc_hip.h) exactly where the reference calls its SSE kernels:
//
//   readForest       (inference.hpp:404-446)  -> gpc_hip_read_forest (host parser) + gpc_hip_warmup: the reference's sample
//                                                calls it BEFORE its clock starts (samples/sparsematch.cpp:42-45) and it is
//                                                the one call that knows the image size, so the device context, the code
//                                                objects and every workspace of that size are made here, not in the first
//                                                timed call (GPC_HIP_NO_WARMUP=1: a host parser only, as in the reference)
//   preprocessImage  (inference.hpp:302-333)  -> gpc_hip_preprocess_begin / _fetch (the image also stays on the device:
//                                                a PreprocessedImage handed to rectifiedMatch / stereoMatch unchanged is
//                                                matched from there, include/gpc_hip.h "Resident images")
//   stereoMatch      (inference.hpp:344-361)  -> gpc_hip_stereo_match
//   rectifiedMatch   (inference.hpp:375-393)  -> gpc_hip_rectified_match
//   matchPair        (extension: the whole t0..t2 region of sparsematch.cpp:45-52 in one
//                     call, raw images in, supports out -> gpc_hip_match_pair)
//
// There is no CPU fallback and, like the reference, no error channel on these methods: a call that cannot run (no gfx950
// device, a HIP error) prints the reason to std::cout and returns an EMPTY result -- the reference's own convention for
// what it can report (readPNG -> 1, readForest -> empty mask).  GPC_HIP_ABORT_ON_ERROR=1 aborts the process instead.
// One device context per host thread (thread_local), device chosen by GPC_HIP_DEVICE.
#ifndef GPC_AMD_INFERENCE_HPP
#define GPC_AMD_INFERENCE_HPP

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "gpc/buffer.hpp"
#include "gpc_hip.h"

using namespace std;  // the reference's headers do this; callers rely on it (sparsematch.cpp)

namespace gpc {
namespace evaluation {  // gpc/evaluation.hpp (extension: matches scored against ground truth)
class Truth;
struct Score;
}  // namespace evaluation
namespace tracking {  // gpc/tracking.hpp (extension: point tracks over a frame sequence)
struct Track;
class TrackStream;
}  // namespace tracking
namespace quads {  // gpc/quads.hpp (extension: circular matches of a stereo sequence closed into quads)
struct Quad;
}  // namespace quads
namespace inference {

typedef std::chrono::high_resolution_clock::time_point time_point;
inline time_point sysTick() { return std::chrono::high_resolution_clock::now(); }
inline float tickToMs(time_point t0, time_point t1) {
  return (float)std::abs(1000. * std::chrono::duration_cast<std::chrono::duration<double>>(t1 - t0).count());
}

struct InferenceSettings {
  uint8_t gradientThreshold_ = 10;
  int dispHigh_ = 128;
  int verticalTolerance_ = 1;
  bool epipolarMode_ = false;
  bool useHashtable_ = false;
  int numThreads_ = 1;

  InferenceSettings(uint8_t gradientThreshold, int dispHigh, int verticalTolerance, bool epipolarMode,
                    bool useHashtable, int numThreads)
      : gradientThreshold_(gradientThreshold), dispHigh_(dispHigh), verticalTolerance_(verticalTolerance),
        epipolarMode_(epipolarMode), useHashtable_(useHashtable), numThreads_(numThreads) {}
  InferenceSettings() {}
  InferenceSettings& builder(void) { return *this; }
  InferenceSettings& gradientThreshold(uint8_t v) { gradientThreshold_ = v; return *this; }
  InferenceSettings& dispHigh(int v) { dispHigh_ = v; return *this; }
  InferenceSettings& verticalTolerance(int v) { verticalTolerance_ = v; return *this; }
  InferenceSettings& epipolarMode(bool v) { epipolarMode_ = v; return *this; }
  InferenceSettings& useHashtable(bool v) { useHashtable_ = v; return *this; }
  InferenceSettings& numThreads(int v) {  // clamped like inference.hpp:122-128; unused on the GPU
    const int hw = (int)std::thread::hardware_concurrency();
    numThreads_ = (v > hw) ? hw : v;
    return *this;
  }
  gpc_settings toC() const {
    gpc_settings s;
    s.gradient_threshold = gradientThreshold_;
    s.disp_high = dispHigh_;
    s.vertical_tolerance = verticalTolerance_;
    s.epipolar_mode = epipolarMode_ ? 1 : 0;
    s.use_hashtable = useHashtable_ ? 1 : 0;
    s.num_threads = numThreads_;
    return s;
  }
};

namespace detail {
struct ContextHolder {
  gpc_hip_ctx* ctx = nullptr;
  // FilterMask last uploaded (the reference passes it by value into every call)
  gpc_filter_mask uploaded;
  bool have = false;
  size_t support_hint = 0;  // supports of this thread's last matchPair call (+ slack): how large the next result array starts
  gpc_filter_mask warmed;   // the forest (with its image size) readForest last warmed this thread's context for
  bool have_warmed = false;
  std::vector<gpc_filter_mask> uploaded_groups;  // the groups last uploaded (group mode; `have` is false then)
  std::vector<gpc_filter_mask> warmed_groups;
  uint8_t* seq_frames = nullptr;  // page-locked staging of sequenceMatch's frames (gpc_hip_host_alloc of ctx)
  size_t seq_cap = 0;
  ~ContextHolder() {
    if (ctx && seq_frames) gpc_hip_host_free(ctx, seq_frames);
    if (ctx) gpc_hip_destroy(ctx);
  }
};
// Status of the last gpc:: call on this thread that reached the library (GPC_OK = 0): the reference's API returns results
// by value and has no error channel, so a failed call returns an EMPTY result -- which also is what "no matches" looks
// like.  A pipeline that must tell the two apart asks gpc::inference::lastStatus() / lastError() after the call.
inline int& last_status() {
  static thread_local int st = GPC_OK;
  return st;
}
inline std::string& last_error() {
  static thread_local std::string msg;
  return msg;
}
inline void fail(int st, gpc_hip_ctx* ctx, const char* what) {
  last_status() = st;
  last_error() = std::string(what) + " failed: " + gpc_hip_status_string(st) +
                 ((st == GPC_E_HIP && ctx) ? std::string(" (") + gpc_hip_last_error(ctx) + ")" : std::string());
  std::cout << "gpc_hip: " << what << " failed: " << gpc_hip_status_string(st);
  if (st == GPC_E_HIP && ctx) std::cout << " (" << gpc_hip_last_error(ctx) << ")";
  std::cout << std::endl;
  if (std::getenv("GPC_HIP_ABORT_ON_ERROR")) std::abort();
}
// quiet: a context that cannot be made is not reported (readForest's warm-up: the call that needs the device will say so)
inline ContextHolder& holder(bool quiet = false) {
  static thread_local ContextHolder h;
  if (!h.ctx) {
    const char* dev = std::getenv("GPC_HIP_DEVICE");
    const int st = gpc_hip_create(dev ? std::atoi(dev) : 0, &h.ctx);
    if (st != GPC_OK) {
      if (!quiet) fail(st, nullptr, "gpc_hip_create");
      h.ctx = nullptr;
      return h;  // the caller returns an empty result
    }
    // Like the reference, the arithmetic variant is a build-time choice of the CALLER's
    // translation unit: -D_INTRINSICS_SSE (the reference's default, samples/CMakeLists.txt:13-17)
    // selects the SSE-exact kernels, its absence the *Naive ones (filter.hpp:157-282).
#ifdef _INTRINSICS_SSE
    gpc_hip_set_arithmetic(h.ctx, GPC_ARITH_SSE);
#else
    gpc_hip_set_arithmetic(h.ctx, GPC_ARITH_NAIVE);
#endif
  }
  return h;
}
}  // namespace detail

// Extension (the reference has no error channel): status / message of this thread's last failed gpc:: call, GPC_OK (0)
// and "" when none failed since clearStatus().  An empty result with lastStatus() == 0 means "no matches".
inline int lastStatus() { return detail::last_status(); }
inline const std::string& lastError() { return detail::last_error(); }
inline void clearStatus() {
  detail::last_status() = GPC_OK;
  detail::last_error().clear();
}

class Forest {
 public:
  struct FilterMask {
    std::vector<int32_t> mask;
    std::vector<int> tau;
    int width;
    int height;
    int type;
    FilterMask(std::vector<int32_t> mask, int width, int height, int type)
        : mask(mask), width(width), height(height), type(type) {}
    FilterMask(std::vector<int32_t> mask, std::vector<int> tau, int width, int height, int type)
        : mask(mask), tau(tau), width(width), height(height), type(type) {}
  };
  struct PreprocessedImage {
    ndb::Buffer<uint8_t> smooth;
    ndb::Buffer<uint8_t> grad;
    std::vector<int> mask;
    PreprocessedImage(ndb::Buffer<uint8_t>& smooth, ndb::Buffer<uint8_t>& grad, std::vector<int>& mask)
        : smooth(smooth), grad(grad), mask(mask) {}
    PreprocessedImage() {}  // what a call that could not run returns: no candidates
  };
  enum CorrMethod { sorting = 's', hashtable = 'h' };

  // inference.hpp:404-446
  FilterMask readForest(std::string path, int width, int height) {
    gpc_filter_mask fm;
    const int st = gpc_hip_read_forest(path.c_str(), width, height, &fm);
    if (st == GPC_E_IO && fm.num_tests == 0 && fm.discarded == 0) {
      cout << "Error opening forest file" << endl;
      return FilterMask(std::vector<int32_t>(), width, height, 0);
    }
    // the reference prints the fern count and one note per discarded test (:417, :431)
    cout << "number of ferns:" << countFerns(path) << endl;
    for (int i = 0; i < fm.discarded; ++i)
      cout << "Note: A maximum of 32 fern features are allowed, discarding remainder of forest." << endl;
    std::vector<int32_t> mask(fm.mask, fm.mask + 2 * fm.num_tests);
    std::vector<int> tau;
    if (fm.type != 0) tau.assign(fm.tau, fm.tau + fm.num_tests);
    FilterMask result = fm.type == 0 ? FilterMask(mask, width, height, 0) : FilterMask(mask, tau, width, height, 1);
    if (st == GPC_OK && fm.num_tests > 0 && !std::getenv("GPC_HIP_NO_WARMUP")) warmUp(result);
    return result;
  }

  // Extension (all trees of a forest): the forest's ferns packed into groups of <= 32 tests (gpc_hip_read_forest_groups).
  // No implicit warm-up: call warmUp(groups).  A missing or malformed file: an empty vector (lastStatus() says why).
  std::vector<FilterMask> readForestGroups(std::string path, int width, int height) {
    std::vector<gpc_filter_mask> fm(GPC_MAX_GROUPS);
    int n = 0;
    const int st = gpc_hip_read_forest_groups(path.c_str(), width, height, fm.data(), (int)fm.size(), &n);
    std::vector<FilterMask> groups;
    if (st != GPC_OK) {
      detail::fail(st, nullptr, "gpc_hip_read_forest_groups");
      return groups;
    }
    for (int g = 0; g < n; ++g) {
      std::vector<int32_t> mask(fm[g].mask, fm[g].mask + 2 * fm[g].num_tests);
      std::vector<int> tau;
      if (fm[g].type != 0) tau.assign(fm[g].tau, fm[g].tau + fm[g].num_tests);
      groups.push_back(fm[g].type == 0 ? FilterMask(mask, width, height, 0) : FilterMask(mask, tau, width, height, 1));
    }
    return groups;
  }

  // Group mode overloads: every group matches as a forest of its own, the result is their union (group 0's records, then
  // each later group's records not emitted before; include/gpc_hip.h, gpc_hip_set_forest_groups)
  std::vector<ndb::Correspondence> stereoMatch(PreprocessedImage& simg, PreprocessedImage& timg, std::vector<FilterMask>& groups,
                                               InferenceSettings settings) {
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, groups)) return std::vector<ndb::Correspondence>();
    const gpc_settings s = settings.toC();
    const int st = gpc_hip_stereo_match_begin(
        h.ctx, simg.smooth.data(), simg.grad.data(), simg.mask.data(), (int)simg.mask.size(), timg.smooth.data(),
        timg.grad.data(), timg.mask.data(), (int)timg.mask.size(), simg.smooth.cols(), simg.smooth.rows(), &s);
    return fetchAll<ndb::Correspondence>(h, st, groups.size() * std::min(simg.mask.size(), timg.mask.size()), "gpc_hip_stereo_match");
  }
  std::vector<ndb::Support> rectifiedMatch(PreprocessedImage& simg, PreprocessedImage& timg, std::vector<FilterMask>& groups,
                                           InferenceSettings settings) {
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, groups)) return std::vector<ndb::Support>();
    const gpc_settings s = settings.toC();
    const int st = gpc_hip_rectified_match_begin(
        h.ctx, simg.smooth.data(), simg.grad.data(), simg.mask.data(), (int)simg.mask.size(), timg.smooth.data(),
        timg.grad.data(), timg.mask.data(), (int)timg.mask.size(), simg.smooth.cols(), simg.smooth.rows(), &s);
    return fetchAll<ndb::Support>(h, st, groups.size() * std::min(simg.mask.size(), timg.mask.size()), "gpc_hip_rectified_match");
  }
  std::vector<ndb::Support> matchPair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, std::vector<FilterMask>& groups,
                                      InferenceSettings settings, int* candidatesL = nullptr, int* candidatesR = nullptr) {
    if (candidatesL) *candidatesL = 0;
    if (candidatesR) *candidatesR = 0;
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, groups)) return std::vector<ndb::Support>();
    const gpc_settings s = settings.toC();
    const int st = gpc_hip_match_pair_begin(h.ctx, simg.data(), timg.data(), simg.cols(), simg.rows(), &s);
    int cl = 0, cr = 0;
    std::vector<ndb::Support> supp = fetchAll<ndb::Support>(h, st, (size_t)simg.rows() * simg.cols(), "gpc_hip_match_pair", &cl, &cr);
    if (candidatesL) *candidatesL = cl;
    if (candidatesR) *candidatesR = cr;
    return supp;
  }
  // Extension (gpc/evaluation.hpp, which defines these): matchPair / sequenceMatch with the records scored against ground
  // truth on the device instead of returned (gpc_hip_score_batch / gpc_hip_score_sequence); precision and recall counts
  // per pair.  A failed call returns a zero Score / an empty vector (lastStatus() says why).
  evaluation::Score scorePair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, FilterMask& forestmask,
                              InferenceSettings settings, const evaluation::Truth& truth, const std::vector<float>& thresholds);
  evaluation::Score scorePair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, std::vector<FilterMask>& groups,
                              InferenceSettings settings, const evaluation::Truth& truth, const std::vector<float>& thresholds);
  std::vector<evaluation::Score> scoreSequence(std::vector<ndb::Buffer<uint8_t>>& frames, FilterMask& fm,
                                               InferenceSettings settings, const std::vector<evaluation::Truth>& truths,
                                               const std::vector<float>& thresholds);

  // Extension (gpc/tracking.hpp, which defines it): sequenceMatch with the correspondences of consecutive pairs chained
  // into point tracks on the device (gpc_hip_track_sequence); the tracks of at least minLength records, in track-id order.
  std::vector<tracking::Track> trackSequence(std::vector<ndb::Buffer<uint8_t>>& frames, FilterMask& fm,
                                             InferenceSettings settings, int minLength = 1);

  // Extension (gpc/quads.hpp, which defines it): a stereo sequence matched three ways from one hashing of its 2 N images --
  // supports of (L_t, R_t), correspondences of (L_t, L_t+1) and (R_t, R_t+1) -- and the circular matches closed into quads
  // on the device (gpc_hip_quads_sequence); result[t] holds the quads of frames t and t + 1.  The two settings must share
  // gradientThreshold_.
  std::vector<std::vector<quads::Quad>> stereoSequenceQuads(std::vector<ndb::Buffer<uint8_t>>& leftFrames,
                                                            std::vector<ndb::Buffer<uint8_t>>& rightFrames, FilterMask& fm,
                                                            InferenceSettings stereoSettings, InferenceSettings flowSettings,
                                                            int tol = 1);

  // the warm-up of readForest for a group-mode forest (gpc_hip_warmup with the groups set)
  void warmUp(std::vector<FilterMask>& groups) {
    detail::ContextHolder& h = detail::holder(true);
    if (!h.ctx || groups.empty()) return;
    const std::vector<gpc_filter_mask> key = toC(groups);
    if (same(h.warmed_groups, key)) return;
    const int st0 = detail::last_status();
    const std::string err0 = detail::last_error();
    if (upload(h, groups) && gpc_hip_warmup(h.ctx, groups[0].width, groups[0].height, nullptr) == GPC_OK) h.warmed_groups = key;
    detail::last_status() = st0;
    detail::last_error() = err0;
  }

  // inference.hpp:302-333
  PreprocessedImage preprocessImage(ndb::Buffer<uint8_t>& img, InferenceSettings settings) {
    assert((settings.gradientThreshold_ >= 0 && settings.gradientThreshold_ <= 255) &&
           "gradientThreshold needs to be within 0...255");
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx) return PreprocessedImage();
    int st = gpc_hip_preprocess_begin(h.ctx, img.data(), img.cols(), img.rows(), settings.gradientThreshold_);
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_preprocess");
      return PreprocessedImage();
    }
    // The arrays the caller keeps are made WHILE the device works, and written once, by the library's threads (no copy
    // of a copy).  The candidate list is sized for every pixel inside the margin and cut to the count afterwards.
    PreprocessedImage r;
    r.smooth = ndb::Buffer<uint8_t>::uninitialized(img.rows(), img.cols());
    r.smooth.width = img.width;
    r.grad = ndb::Buffer<uint8_t>::uninitialized(img.rows(), img.cols());
    r.grad.width = img.width;
    const size_t maxcand = (size_t)(img.cols() - 2 * GPC_PATCH_RADIUS) * (size_t)(img.rows() - 2 * GPC_PATCH_RADIUS);
    r.mask.resize(maxcand);
    int n = 0;
    st = gpc_hip_preprocess_fetch(h.ctx, r.smooth.data(), r.grad.data(), r.mask.data(), (int)maxcand, &n);
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_preprocess");
      return PreprocessedImage();
    }
    r.mask.resize((size_t)n);
    return r;
  }

  // inference.hpp:344-361
  std::vector<ndb::Correspondence> stereoMatch(PreprocessedImage& simg, PreprocessedImage& timg,
                                               FilterMask& forestmask, InferenceSettings settings) {
    assert((forestmask.width == simg.smooth.cols() && forestmask.height == simg.smooth.rows()) &&
           "Source Image: dimension does not fit dimension of supplied forest mask");
    assert((forestmask.width == timg.smooth.cols() && forestmask.height == simg.smooth.rows()) &&
           "Targe Image: dimension does not fit dimension of supplied forest mask");
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, forestmask)) return std::vector<ndb::Correspondence>();
    const gpc_settings s = settings.toC();
    // the kernels are queued, the result array is made (and zeroed by the allocator) while they run, the library's threads
    // fill it; no match of two candidate lists has more results than the shorter list
    int st = gpc_hip_stereo_match_begin(
        h.ctx, simg.smooth.data(), simg.grad.data(), simg.mask.data(), (int)simg.mask.size(), timg.smooth.data(),
        timg.grad.data(), timg.mask.data(), (int)timg.mask.size(), simg.smooth.cols(), simg.smooth.rows(), &s);
    std::vector<ndb::Correspondence> corr;
    int n = 0;
    if (st == GPC_OK) {
      corr.resize(std::min(simg.mask.size(), timg.mask.size()) + 1);
      st = gpc_hip_match_fetch(h.ctx, corr.data(), (int)corr.size(), &n, nullptr, nullptr);
    }
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_stereo_match");
      return std::vector<ndb::Correspondence>();
    }
    corr.resize((size_t)n);
    return corr;
  }

  // Extension (optical flow over a video): stereoMatch(preprocessImage(frames[t]), preprocessImage(frames[t + 1]), ...)
  // for every consecutive pair, t = 0 .. frames.size() - 2, with each frame preprocessed and hashed once
  // (gpc_hip_match_sequence).  The frames are staged contiguously in page-locked memory of this thread's context.  Fewer
  // than two frames, frames of different sizes or a failed call: an empty result (lastStatus() says why).
  std::vector<std::vector<ndb::Correspondence>> sequenceMatch(std::vector<ndb::Buffer<uint8_t>>& frames, FilterMask& fm,
                                                              InferenceSettings settings) {
    typedef std::vector<std::vector<ndb::Correspondence>> Result;
    if (frames.size() < 2) {
      detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_match_sequence");
      return Result();
    }
    const int W = frames[0].cols(), H = frames[0].rows(), N = (int)frames.size();
    for (const ndb::Buffer<uint8_t>& f : frames)
      if (f.cols() != W || f.rows() != H) {
        detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_match_sequence");
        return Result();
      }
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, fm)) return Result();
    const size_t n = (size_t)W * H, bytes = n * N;
    if (bytes > h.seq_cap) {
      if (h.seq_frames) gpc_hip_host_free(h.ctx, h.seq_frames);
      h.seq_frames = nullptr;
      h.seq_cap = 0;
      void* p = nullptr;
      const int st = gpc_hip_host_alloc(h.ctx, bytes, &p);
      if (st != GPC_OK) {
        detail::fail(st, h.ctx, "gpc_hip_host_alloc");
        return Result();
      }
      h.seq_frames = static_cast<uint8_t*>(p);
      h.seq_cap = bytes;
    }
    for (int f = 0; f < N; ++f) memcpy(h.seq_frames + (size_t)f * n, frames[f].data(), n);
    const gpc_settings s = settings.toC();
    // no match of two candidate lists has more results than the shorter list: a quarter of the pixels first, the true
    // largest count when that did not fit
    int cap = (int)std::max<size_t>(1024, n / 4);
    std::vector<gpc_correspondence> out;
    std::vector<int32_t> counts((size_t)N - 1);
    int st = GPC_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
      out.resize((size_t)cap * (N - 1));
      st = gpc_hip_match_sequence(h.ctx, h.seq_frames, W, H, N, &s, out.data(), cap, counts.data(), nullptr);
      if (st != GPC_E_CAPACITY) break;
      cap = *std::max_element(counts.begin(), counts.end());
    }
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_match_sequence");
      return Result();
    }
    Result r((size_t)N - 1);
    for (int t = 0; t < N - 1; ++t) {
      const gpc_correspondence* c = out.data() + (size_t)t * cap;
      r[t].reserve((size_t)counts[t]);
      for (int i = 0; i < counts[t]; ++i)
        r[t].push_back(ndb::Correspondence(ndb::Point(c[i].src_x, c[i].src_y), ndb::Point(c[i].tar_x, c[i].tar_y)));
    }
    return r;
  }

  // inference.hpp:375-393
  std::vector<ndb::Support> rectifiedMatch(PreprocessedImage& simg, PreprocessedImage& timg,
                                           FilterMask& forestmask, InferenceSettings settings) {
    assert((forestmask.width == simg.smooth.cols() && forestmask.height == simg.smooth.rows()) &&
           "Source Image: dimension does not fit dimension of supplied forest mask");
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, forestmask)) return std::vector<ndb::Support>();
    const gpc_settings s = settings.toC();
    int st = gpc_hip_rectified_match_begin(   // (queued; the array is made while the kernels run: see stereoMatch)
        h.ctx, simg.smooth.data(), simg.grad.data(), simg.mask.data(), (int)simg.mask.size(), timg.smooth.data(),
        timg.grad.data(), timg.mask.data(), (int)timg.mask.size(), simg.smooth.cols(), simg.smooth.rows(), &s);
    std::vector<ndb::Support> supp;
    int n = 0;
    if (st == GPC_OK) {
      supp.resize(std::min(simg.mask.size(), timg.mask.size()) + 1);
      st = gpc_hip_match_fetch(h.ctx, supp.data(), (int)supp.size(), &n, nullptr, nullptr);
    }
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_rectified_match");
      return std::vector<ndb::Support>();
    }
    supp.resize((size_t)n);
    return supp;
  }

  // Extension: preprocessImage x2 + rectifiedMatch without bringing the intermediates back
  // to the host (the timed region of samples/sparsematch.cpp:45-52 as one device pipeline).
  std::vector<ndb::Support> matchPair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, FilterMask& forestmask,
                                      InferenceSettings settings, int* candidatesL = nullptr,
                                      int* candidatesR = nullptr) {
    if (candidatesL) *candidatesL = 0;  // (defined on every path out, the failing ones included)
    if (candidatesR) *candidatesR = 0;
    detail::ContextHolder& h = detail::holder();
    if (!h.ctx || !upload(h, forestmask)) return std::vector<ndb::Support>();
    const gpc_settings s = settings.toC();
    // Queued (the images pass through page-locked memory of the context); the result array is made while the kernels run,
    // sized by this thread's last call rather than by the worst case (one support per pixel), and the library's threads
    // fill it.  Results that do not fit are fetched again into a larger array (they stay with the context until its next call).
    int st = gpc_hip_match_pair_begin(h.ctx, simg.data(), timg.data(), simg.cols(), simg.rows(), &s);
    std::vector<ndb::Support> supp;
    int n = 0, cl = 0, cr = 0;
    if (st == GPC_OK) {
      const size_t npix = (size_t)simg.rows() * simg.cols();
      size_t cap0 = h.support_hint ? h.support_hint : npix * 3 / 4 + 1;
      if (cap0 > npix + 1) cap0 = npix + 1;
      supp.resize(cap0);
      st = gpc_hip_match_fetch(h.ctx, supp.data(), (int)supp.size(), &n, &cl, &cr);
      if (st == GPC_E_CAPACITY) {
        supp.resize((size_t)n);
        st = gpc_hip_match_fetch(h.ctx, supp.data(), (int)supp.size(), &n, &cl, &cr);
      }
    }
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_match_pair");
      return std::vector<ndb::Support>();
    }
    supp.resize((size_t)n);
    if (candidatesL) *candidatesL = cl;
    if (candidatesR) *candidatesR = cr;
    h.support_hint = (size_t)n + (size_t)n / 8 + 1024;
    return supp;
  }

 private:
  friend class tracking::TrackStream;  // (gpc/tracking.hpp: hands the forest over as the match calls do)
  evaluation::Score scoreWith(detail::ContextHolder& h, ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg,
                              InferenceSettings settings, const evaluation::Truth& truth, const std::vector<float>& thresholds);
  // What the reference's caller does next -- preprocessImage x2, rectifiedMatch / matchPair on images of this size --
  // done once here on a synthetic image and thrown away: context, code objects, workspaces and page-locked staging
  // (gpc_hip_warmup), and this thread's own staging and the allocator's state for result arrays of this size (the dry run
  // below).  Says nothing and leaves no status when it cannot run (no device: the first real call reports that).
  void warmUp(FilterMask& forestmask) {
    detail::ContextHolder& h = detail::holder(true);
    if (!h.ctx) return;
    gpc_filter_mask key;
    if (!toC(forestmask, key)) return;
    if (h.have_warmed && memcmp(&h.warmed, &key, sizeof key) == 0) return;
    if (gpc_hip_set_forest(h.ctx, &key) != GPC_OK) return;
    h.uploaded = key;
    h.have = true;
    if (gpc_hip_warmup(h.ctx, forestmask.width, forestmask.height, nullptr) != GPC_OK) return;
    ndb::Buffer<uint8_t> img(forestmask.height, forestmask.width);
    for (int y = 0; y < img.rows(); ++y)
      for (int x = 0; x < img.cols(); ++x) {
        uint32_t v = ((uint32_t)(x >> 2) * 73856093u) ^ ((uint32_t)(y >> 2) * 19349663u);
        v ^= v >> 16; v *= 0x85ebca6bu; v ^= v >> 13;
        img(y, x) = (uint8_t)(v >> 9);
      }
    const int st0 = detail::last_status();
    const std::string err0 = detail::last_error();
    {
      // The allocator, too, has a cold start: glibc hands blocks of this size out as fresh mappings (every page of a result
      // array then faults on first touch: 0.3-0.5 ms of the first timed call at 1024x436) until it has seen a larger block
      // come and go -- after that it serves them from the heap and keeps the heap mapped between calls.  A loop over frames
      // reaches that state by itself after a few iterations; the one-shot caller is put there here: one block larger than
      // a call's arrays together (32 bytes per pixel, at most the 32 MiB up to which glibc adapts), never touched.
      size_t ballast = (size_t)forestmask.width * (size_t)forestmask.height * 32u;
      if (ballast > ((size_t)32 << 20) - 65536) ballast = ((size_t)32 << 20) - 65536;  // (the chunk, header included, must stay within the limit)
      void* b = std::malloc(ballast);
      asm volatile("" : "+r"(b));   // (or the compiler removes the pair)
      std::free(b);
    }
    InferenceSettings sparse(5, 128, 0, true, false, 1);
    for (int it = 0; it < 2; ++it) {
      PreprocessedImage a = preprocessImage(img, sparse), b = preprocessImage(img, sparse);
      std::vector<ndb::Support> r = rectifiedMatch(a, b, forestmask, sparse);
      std::vector<ndb::Support> f = matchPair(img, img, forestmask, sparse);
      h.support_hint = 0;  // (a pair matched against itself says nothing about the caller's)
    }
    detail::last_status() = st0;
    detail::last_error() = err0;
    h.warmed = key;
    h.have_warmed = true;
  }

  static int countFerns(const std::string& path) {
    FILE* fp = fopen(path.c_str(), "rb");
    int n = 0;
    if (fp) {
      if (fscanf(fp, "%d", &n) != 1) n = 0;
      fclose(fp);
    }
    return n;
  }
  static bool toC(const FilterMask& f, gpc_filter_mask& fm) {
    memset(&fm, 0, sizeof fm);
    fm.num_tests = (int)(f.mask.size() / 2);
    if (fm.num_tests > GPC_MAX_TESTS) fm.num_tests = GPC_MAX_TESTS;  // filter.hpp:574 `i < 64`
    for (int i = 0; i < 2 * fm.num_tests; ++i) fm.mask[i] = f.mask[i];
    for (int i = 0; i < fm.num_tests && i < (int)f.tau.size(); ++i) fm.tau[i] = f.tau[i];
    fm.type = f.type;
    fm.width = f.width;
    fm.height = f.height;
    return true;
  }
  static bool upload(detail::ContextHolder& h, const FilterMask& f) {
    gpc_filter_mask fm;
    toC(f, fm);
    if (h.have && memcmp(&h.uploaded, &fm, sizeof fm) == 0) return true;
    const int st = gpc_hip_set_forest(h.ctx, &fm);
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_set_forest");
      return false;
    }
    h.uploaded = fm;
    h.have = true;
    h.uploaded_groups.clear();
    return true;
  }
  static std::vector<gpc_filter_mask> toC(const std::vector<FilterMask>& groups) {
    std::vector<gpc_filter_mask> fm(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) toC(groups[g], fm[g]);
    return fm;
  }
  static bool same(const std::vector<gpc_filter_mask>& a, const std::vector<gpc_filter_mask>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(gpc_filter_mask) * a.size()) == 0);
  }
  static bool upload(detail::ContextHolder& h, const std::vector<FilterMask>& groups) {
    const std::vector<gpc_filter_mask> fm = toC(groups);
    if (!h.uploaded_groups.empty() && same(h.uploaded_groups, fm)) return true;
    const int st = fm.empty() ? GPC_E_INVALID : gpc_hip_set_forest_groups(h.ctx, fm.data(), (int)fm.size());
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, "gpc_hip_set_forest_groups");
      return false;
    }
    h.uploaded_groups = fm;
    h.have = false;  // (the single-forest record no longer describes the context)
    return true;
  }
  // begin + fetch of a group-mode call: the union can hold up to G * min(nL, nR) records; fetched again on GPC_E_CAPACITY
  template <class T>
  static std::vector<T> fetchAll(detail::ContextHolder& h, int st, size_t cap0, const char* what, int* cl = nullptr,
                                 int* cr = nullptr) {
    std::vector<T> out;
    int n = 0;
    if (st == GPC_OK) {
      out.resize(cap0 + 1);
      st = gpc_hip_match_fetch(h.ctx, out.data(), (int)out.size(), &n, cl, cr);
      if (st == GPC_E_CAPACITY) {
        out.resize((size_t)n);
        st = gpc_hip_match_fetch(h.ctx, out.data(), (int)out.size(), &n, cl, cr);
      }
    }
    if (st != GPC_OK) {
      detail::fail(st, h.ctx, what);
      return std::vector<T>();
    }
    out.resize((size_t)n);
    return out;
  }
};

}  // namespace inference
}  // namespace gpc
#endif
