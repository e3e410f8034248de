// gpc/evaluation.hpp -- extension (the reference has no evaluation code): matches scored against ground truth on the GPU
// (gpc_hip_score_*, include/gpc_hip.h).  A Score is a set of exact counts per pair; precision(k) = n_within[k] / n_judged is
// the share of the judged records that lie within thresholds[k] pixels of the truth, recall(k) = n_within[k] / n_matchable
// the share of the matchable pixels that were found -- the pair the Global Patch Collider is evaluated by and
// Fern.hpp's trainer optimises.
//
//   Truth                                 the float planes and the ignore mask of one pair, from the Sintel datasources' files
//   scoreSupports / scoreCorrespondences  records the caller holds (host vectors) against a Truth (gpc_hip_score_supports /
//                                         gpc_hip_score_correspondences)
//   Forest::scorePair / scoreSequence     match and score without the records coming back (declared in gpc/inference.hpp)
//
// Validity is the rule of the reference's samplers (getGroundTruthMatches): a pixel counts where every mask is zero AT THE
// SOURCE COORDINATES -- flow: occlusion and invalid of the source and of the target frame, OR-ed; stereo: occlusion and
// out-of-frame.  Disparities are decoded as the trainer was shown them: SintelStereo::decodeDisparity, the INTEGER
// 4 r + g / 64.  Truth::fromDisparitySubpixel is the named alternative (4 r + g / 64 + b / 16384 in float).
#ifndef _GPC_evaluation
#define _GPC_evaluation

#include <cstdint>
#include <cstring>
#include <vector>

#include "gpc/SintelOpticalFlow.hpp"
#include "gpc/SintelStereo.hpp"
#include "gpc/buffer.hpp"
#include "gpc/inference.hpp"
#include "gpc_hip.h"

namespace gpc {
namespace evaluation {

class Truth {
 public:
  int width = 0, height = 0;
  std::vector<float> u, v;      // row-major [height][width]; v empty: stereo (u = disparity)
  std::vector<uint8_t> ignore;  // nonzero: do not judge this source pixel
  bool flow() const { return !v.empty(); }
  bool empty() const { return u.empty(); }
  // the members are public: every plane that is there holds width x height values (ignore may be empty: nothing is ignored)
  bool consistent() const {
    const size_t n = (size_t)width * (size_t)height;
    return width > 0 && height > 0 && u.size() == n && (v.empty() || v.size() == n) && (ignore.empty() || ignore.size() == n);
  }

  // flow: the .flo field and the four masks read at the source coordinates (SintelOpticalFlow.hpp:509-540 of the reference)
  static Truth fromFlow(const gpc::datasource::FlowField& f, const ndb::Buffer<uint8_t>& oclSrc, const ndb::Buffer<uint8_t>& oclTar,
                        const ndb::Buffer<uint8_t>& invSrc, const ndb::Buffer<uint8_t>& invTar) {
    Truth t;
    t.width = f.width;
    t.height = f.height;
    t.u = f.u;
    t.v = f.v;
    t.ignore.assign((size_t)f.width * f.height, 0);
    for (const ndb::Buffer<uint8_t>* m : {&oclSrc, &oclTar, &invSrc, &invTar}) t.orMask(*m);
    return t;
  }
  // stereo: the RGB disparity map, occlusion and out-of-frame masks (SintelStereo.hpp:416-440 of the reference); integer decode
  static Truth fromDisparity(const ndb::RGBBuffer& disp, const ndb::Buffer<uint8_t>& occlusion, const ndb::Buffer<uint8_t>& outOfFrame) {
    return fromDisparityWith(disp, occlusion, outOfFrame, false);
  }
  static Truth fromDisparitySubpixel(const ndb::RGBBuffer& disp, const ndb::Buffer<uint8_t>& occlusion,
                                     const ndb::Buffer<uint8_t>& outOfFrame) {
    return fromDisparityWith(disp, occlusion, outOfFrame, true);
  }
  // the planes padded (or cut) to cols x rows, as readPNG pads an image's columns to a multiple of 16; new pixels are ignored
  Truth resized(int cols, int rows) const {
    Truth t;
    t.width = cols;
    t.height = rows;
    t.u.assign((size_t)cols * rows, 0.f);
    if (flow()) t.v.assign((size_t)cols * rows, 0.f);
    t.ignore.assign((size_t)cols * rows, 1);
    for (int y = 0; y < rows && y < height; ++y)
      for (int x = 0; x < cols && x < width; ++x) {
        const size_t a = (size_t)y * cols + x, b = (size_t)y * width + x;
        t.u[a] = u[b];
        if (flow()) t.v[a] = v[b];
        t.ignore[a] = ignore.empty() ? 0 : ignore[b];
      }
    return t;
  }
  gpc_truth toC() const { return gpc_truth{u.data(), flow() ? v.data() : nullptr, ignore.empty() ? nullptr : ignore.data()}; }

 private:
  void orMask(const ndb::Buffer<uint8_t>& m) {
    for (int y = 0; y < height && y < m.rows(); ++y)
      for (int x = 0; x < width && x < m.cols(); ++x)
        if (m.getPixel(x, y) != 0) ignore[(size_t)y * width + x] = 1;
  }
  static Truth fromDisparityWith(const ndb::RGBBuffer& disp, const ndb::Buffer<uint8_t>& occlusion,
                                 const ndb::Buffer<uint8_t>& outOfFrame, bool subpixel) {
    Truth t;
    t.width = disp.cols();
    t.height = disp.rows();
    t.u.resize((size_t)t.width * t.height);
    t.ignore.assign(t.u.size(), 0);
    for (int y = 0; y < t.height; ++y)
      for (int x = 0; x < t.width; ++x) {
        const ndb::RGBColor c = disp.getPixel(x, y);
        t.u[(size_t)y * t.width + x] = subpixel ? (float)c.r * 4.f + (float)c.g / 64.f + (float)c.b / 16384.f
                                                : (float)gpc::datasource::SintelStereo::decodeDisparity(c);
      }
    t.orMask(occlusion);
    t.orMask(outOfFrame);
    return t;
  }
};

struct Score : gpc_score {
  Score() { std::memset(static_cast<gpc_score*>(this), 0, sizeof(gpc_score)); }
  explicit Score(const gpc_score& s) : gpc_score(s) {}
  double precision(int k) const { return n_judged > 0 ? (double)n_within[k] / (double)n_judged : 0.0; }
  double recall(int k) const { return n_matchable > 0 ? (double)n_within[k] / (double)n_matchable : 0.0; }
  Score& operator+=(const gpc_score& o) {
    n_records += o.n_records;
    n_ignored += o.n_ignored;
    n_no_truth += o.n_no_truth;
    n_judged += o.n_judged;
    for (int k = 0; k < GPC_SCORE_MAX_THR; ++k) n_within[k] += o.n_within[k];
    sum_e2_q8 += o.sum_e2_q8;
    n_candidates += o.n_candidates;
    n_matchable += o.n_matchable;
    return *this;
  }
};

namespace detail {
// one pair's records (host) against a Truth through the library's host records forms
template <class Rec>
inline Score scoreRecords(const std::vector<Rec>& rec, const Truth& truth, const std::vector<float>& thr, bool corr) {
  namespace inf = gpc::inference::detail;
  static_assert(sizeof(ndb::Support) == sizeof(gpc_support) && sizeof(ndb::Correspondence) == sizeof(gpc_correspondence), "layouts");
  Score out;
  inf::ContextHolder& h = inf::holder();
  if (!h.ctx) return out;
  if (!truth.consistent() || truth.flow() != corr) {
    inf::fail(GPC_E_INVALID, h.ctx, corr ? "gpc_hip_score_correspondences" : "gpc_hip_score_supports");
    return out;
  }
  const Rec none{};
  const Rec* r = rec.empty() ? &none : rec.data();  // (no records: one unread slot, count 0)
  const int cap = rec.empty() ? 1 : (int)rec.size();
  const int32_t count = (int32_t)rec.size();
  const gpc_truth t = truth.toC();
  const int st = corr ? gpc_hip_score_correspondences(h.ctx, reinterpret_cast<const gpc_correspondence*>(r), cap, &count, truth.width,
                                                      truth.height, 1, &t, thr.data(), (int)thr.size(), &out)
                      : gpc_hip_score_supports(h.ctx, reinterpret_cast<const gpc_support*>(r), cap, &count, truth.width, truth.height,
                                               1, &t, thr.data(), (int)thr.size(), &out);
  if (st != GPC_OK) {
    inf::fail(st, h.ctx, corr ? "gpc_hip_score_correspondences" : "gpc_hip_score_supports");
    return Score();
  }
  return out;
}
}  // namespace detail

// Records the caller already holds.  A failed call returns a zero Score (gpc::inference::lastStatus() says why).
inline Score scoreSupports(std::vector<ndb::Support>& supports, const Truth& truth, const std::vector<float>& thresholds) {
  return detail::scoreRecords(supports, truth, thresholds, false);
}
inline Score scoreCorrespondences(std::vector<ndb::Correspondence>& corr, const Truth& truth, const std::vector<float>& thresholds) {
  return detail::scoreRecords(corr, truth, thresholds, true);
}

}  // namespace evaluation

namespace inference {

// Forest::scorePair / scoreSequence (declared in gpc/inference.hpp): matchPair / sequenceMatch with the records scored on
// the device instead of returned.
inline evaluation::Score Forest::scoreWith(detail::ContextHolder& h, ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg,
                                           InferenceSettings settings, const evaluation::Truth& truth,
                                           const std::vector<float>& thresholds) {
  evaluation::Score out;
  if (!truth.consistent() || truth.width != simg.cols() || truth.height != simg.rows() || timg.cols() != simg.cols() ||
      timg.rows() != simg.rows() || truth.flow()) {
    detail::fail(GPC_E_INVALID, h.ctx, "gpc_hip_score_batch");
    return out;
  }
  const gpc_settings s = settings.toC();
  const gpc_truth t = truth.toC();
  const int st = gpc_hip_score_batch(h.ctx, simg.data(), timg.data(), simg.cols(), simg.rows(), 1, &s, &t, thresholds.data(),
                                     (int)thresholds.size(), &out);
  if (st != GPC_OK) {
    detail::fail(st, h.ctx, "gpc_hip_score_batch");
    return evaluation::Score();
  }
  return out;
}
inline evaluation::Score Forest::scorePair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, FilterMask& forestmask,
                                           InferenceSettings settings, const evaluation::Truth& truth,
                                           const std::vector<float>& thresholds) {
  detail::ContextHolder& h = detail::holder();
  if (!h.ctx || !upload(h, forestmask)) return evaluation::Score();
  return scoreWith(h, simg, timg, settings, truth, thresholds);
}
inline evaluation::Score Forest::scorePair(ndb::Buffer<uint8_t>& simg, ndb::Buffer<uint8_t>& timg, std::vector<FilterMask>& groups,
                                           InferenceSettings settings, const evaluation::Truth& truth,
                                           const std::vector<float>& thresholds) {
  detail::ContextHolder& h = detail::holder();
  if (!h.ctx || !upload(h, groups)) return evaluation::Score();
  return scoreWith(h, simg, timg, settings, truth, thresholds);
}
inline std::vector<evaluation::Score> Forest::scoreSequence(std::vector<ndb::Buffer<uint8_t>>& frames, FilterMask& fm,
                                                            InferenceSettings settings, const std::vector<evaluation::Truth>& truths,
                                                            const std::vector<float>& thresholds) {
  typedef std::vector<evaluation::Score> Result;
  const int N = (int)frames.size();
  bool ok = N >= 2 && (int)truths.size() == N - 1;
  const int W = N ? frames[0].cols() : 0, H = N ? frames[0].rows() : 0;
  for (int f = 0; ok && f < N; ++f) ok = frames[f].cols() == W && frames[f].rows() == H;
  bool masks = false;  // one of the pairs has an ignore mask: the others get an empty one
  for (int t = 0; ok && t < N - 1; ++t) {
    ok = truths[t].consistent() && truths[t].width == W && truths[t].height == H && truths[t].flow();
    masks = masks || !truths[t].ignore.empty();
  }
  if (!ok) {
    detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_score_sequence");
    return Result();
  }
  detail::ContextHolder& h = detail::holder();
  if (!h.ctx || !upload(h, fm)) return Result();
  const size_t n = (size_t)W * H;
  std::vector<uint8_t> fr(n * N), ig(masks ? n * (N - 1) : 0, 0);
  std::vector<float> u(n * (N - 1)), v(n * (N - 1));
  for (int f = 0; f < N; ++f) std::memcpy(&fr[n * f], frames[f].data(), n);
  for (int t = 0; t < N - 1; ++t) {
    std::memcpy(&u[n * t], truths[t].u.data(), sizeof(float) * n);
    std::memcpy(&v[n * t], truths[t].v.data(), sizeof(float) * n);
    if (!truths[t].ignore.empty()) std::memcpy(&ig[n * t], truths[t].ignore.data(), n);
  }
  const gpc_settings s = settings.toC();
  const gpc_truth t = {u.data(), v.data(), masks ? ig.data() : nullptr};
  std::vector<gpc_score> sc((size_t)N - 1);
  const int st = gpc_hip_score_sequence(h.ctx, fr.data(), W, H, N, &s, &t, thresholds.data(), (int)thresholds.size(), sc.data());
  if (st != GPC_OK) {
    detail::fail(st, h.ctx, "gpc_hip_score_sequence");
    return Result();
  }
  Result r;
  for (const gpc_score& x : sc) r.push_back(evaluation::Score(x));
  return r;
}

}  // namespace inference
}  // namespace gpc
#endif
