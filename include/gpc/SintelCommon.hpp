// gpc/SintelCommon.hpp -- what gpc/SintelOpticalFlow.hpp and gpc/SintelStereo.hpp share: the scene list and directory
// walk of the reference's datasources (SintelOpticalFlow.hpp:63-334, SintelStereo.hpp:58-284), the frame generators, and
// the extraction itself, which runs on the GPU (gpc_hip_extract_triplets, include/gpc_hip.h) instead of through one
// host-side ndb::Buffer per patch.
//
// Extensions (not in the reference), marked where they are defined:
//   - seed(s): frame ordinal f draws from std::mt19937(s + f), the final shuffle runs after srand(s);
//   - a cap of 1000 x numTripletsPerPair sampler draws per frame (the reference loops forever on a frame without a
//     valid pixel);
//   - extractTrainingSet(): the extracted set stays on the device (DeviceTrainingSet) instead of becoming host objects;
//   - DeviceTrainingSet::fromHost / fromBytes: a host set uploaded once, for Forest::trainAndExport's device overload.
#ifndef _GPC_SintelCommon
#define _GPC_SintelCommon

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "gpc/Feature.hpp"
#include "gpc/buffer.hpp"
#include "gpc/inference.hpp"
#include "gpc_hip.h"

namespace gpc {
namespace datasource {

// A training set extracted on the device (extension): an ordinary gpc_hip_train_set of this thread's context, which
// every gpc_hip_train_* call scores as it is.  Move-only; destroyed with the object.
class DeviceTrainingSet {
 public:
  typedef gpc::training::Feature::GPCPatchTriplet GPCTriplet_t;
  DeviceTrainingSet() {}
  DeviceTrainingSet(gpc_hip_ctx* ctx, gpc_hip_train_set* set, int n) : ctx_(ctx), set_(set), n_(n) {}
  DeviceTrainingSet(DeviceTrainingSet&& o) noexcept { swap(o); }
  DeviceTrainingSet& operator=(DeviceTrainingSet&& o) noexcept {
    DeviceTrainingSet t(std::move(o));
    swap(t);
    return *this;
  }
  DeviceTrainingSet(const DeviceTrainingSet&) = delete;
  DeviceTrainingSet& operator=(const DeviceTrainingSet&) = delete;
  ~DeviceTrainingSet() {
    if (set_) gpc_hip_train_set_destroy(ctx_, set_);
  }
  int size() const { return n_; }
  bool empty() const { return n_ == 0; }
  gpc_hip_ctx* ctx() const { return ctx_; }
  gpc_hip_train_set* set() const { return set_; }
  // triplets [first, first + n) in the byte order of Feature::storeAllTriplets (n * 3 * 729 bytes)
  int read(int first, int n, uint8_t* aos) const { return set_ ? gpc_hip_train_set_read(ctx_, set_, first, n, aos) : (n ? GPC_E_INVALID : GPC_OK); }

  // n triplets in the byte order of Feature::storeAllTriplets (a loaded .bin as it is) as a device set of this thread's
  // context: one upload, all marks cleared.  Empty on failure (gpc::inference::lastStatus() says why).
  static DeviceTrainingSet fromBytes(const uint8_t* aos, int n) {
    if (!aos || n <= 0) return DeviceTrainingSet();
    gpc_hip_ctx* ctx = gpc::inference::detail::holder().ctx;
    if (!ctx) return DeviceTrainingSet();
    gpc_hip_train_set* set = nullptr;
    const int st = gpc_hip_train_set_create(ctx, aos, n, &set);
    if (st != GPC_OK) {
      gpc::inference::detail::fail(st, ctx, "gpc_hip_train_set_create");
      return DeviceTrainingSet();
    }
    return DeviceTrainingSet(ctx, set, n);
  }
  // the same from the reference's host vector (what loadTrainingData returns); the triplets' split marks are not carried over
  static DeviceTrainingSet fromHost(std::vector<GPCTriplet_t>& data) {
    std::vector<uint8_t> aos(data.size() * 3 * 729);
    for (size_t k = 0; k < data.size(); ++k) {
      std::memcpy(&aos[(k * 3 + 0) * 729], data[k].ref.feature.data(), 729);
      std::memcpy(&aos[(k * 3 + 1) * 729], data[k].pos.feature.data(), 729);
      std::memcpy(&aos[(k * 3 + 2) * 729], data[k].neg.feature.data(), 729);
    }
    return fromBytes(aos.data(), (int)data.size());
  }

 private:
  void swap(DeviceTrainingSet& o) {
    std::swap(ctx_, o.ctx_);
    std::swap(set_, o.set_);
    std::swap(n_, o.n_);
  }
  gpc_hip_ctx* ctx_ = nullptr;
  gpc_hip_train_set* set_ = nullptr;
  int n_ = 0;
};

namespace detail {

// SintelOpticalFlow.hpp:194-200 (SintelStereo.hpp:186-192): the 23 training scenes; the extraction visits the first 20
inline const std::vector<std::string>& sceneNames() {
  static const std::vector<std::string> names = {
      "alley_1",   "alley_2",   "ambush_2",  "ambush_4",   "ambush_5",   "ambush_6",   "ambush_7", "bamboo_1",
      "bamboo_2",  "bandage_1", "bandage_2", "cave_2",     "cave_4",     "market_2",   "market_5", "market_6",
      "mountain_1", "shaman_2", "shaman_3",  "sleeping_1", "sleeping_2", "temple_2",   "temple_3"};
  return names;
}
static const int kVisitedScenes = 20;  // SintelOpticalFlow.hpp:126, SintelStereo.hpp:120: sceneId < 20

// SintelOpticalFlow.hpp:77-83
inline bool isDir(const std::string& path) {
  struct stat info;
  return stat(path.c_str(), &info) == 0 && (info.st_mode & S_IFDIR);
}

// SintelOpticalFlow.hpp:281-301: every directory entry whose name ends in "png"
inline int countImages(const std::string& dir) {
  DIR* d = opendir(dir.c_str());
  if (!d) {
    std::cout << "ERR:couldn't open directory" << std::endl;
    return 0;
  }
  int cnt = 0;
  while (struct dirent* ent = readdir(d)) {
    const std::string name = ent->d_name;
    if (name.length() >= 3 && name.substr(name.length() - 3) == "png") cnt++;
  }
  closedir(d);
  return cnt;
}

inline std::string frameName(int id) {  // "frame_%04d" (SintelOpticalFlow.hpp:348)
  char buf[32];
  snprintf(buf, sizeof buf, "frame_%04d", id);
  return buf;
}

// SintelOpticalFlow.hpp:269-274: 1024 x 436 is hard-coded by both samplers
inline bool isSafePatchCenter(int x, int y, int width, int height) {
  return x > 20 && y > 20 && x < (width - 21) && y < (height - 21);
}

// The generator of one frame: std::mt19937 seeded from std::random_device (SintelOpticalFlow.hpp:497-498), or, after
// seed(s) (extension), std::mt19937(s + ordinal), the ordinal counting every frame the scene walk reaches.
struct Generators {
  bool seeded = false;
  unsigned seed = 0;
  std::mt19937 frame(long ordinal) const {
    if (seeded) return std::mt19937((unsigned)(seed + (unsigned long)ordinal));
    std::random_device rd;
    return std::mt19937(rd());
  }
  // std::random_shuffle of the whole set (SintelOpticalFlow.hpp:160), applied to the indices of the triplets instead of to
  // the triplets: the algorithm draws the same numbers for any element type, so triplet k ends where the reference's
  // shuffle would put it.  order[k] = that position (the `order` of gpc_hip_extract_triplets).
  std::vector<int32_t> shuffle(int n) const {
    if (seeded) srand(seed);
    std::vector<int32_t> at(n), order(n);
    for (int k = 0; k < n; ++k) at[k] = k;
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wdeprecated-declarations"
    std::random_shuffle(at.begin(), at.end());
#pragma GCC diagnostic pop
    for (int j = 0; j < n; ++j) order[at[j]] = j;
    return order;
  }
};

// Draw cap (extension): at most 1000 x numKpts sampler draws per frame
inline long drawCap(int numKpts) { return 1000l * (numKpts > 0 ? numKpts : 1); }
inline void warnDrawCap(size_t found, int numKpts) {
  std::cout << "WARN: sampler draw cap reached, keeping " << found << " of " << numKpts << " triplets of this frame" << std::endl;
}

// The frames and keypoints of an extraction, gathered during the scene walk and handed to the device in one call.
// Frames are the raw gray images as readPNG returns them (columns padded to a multiple of 16: the image
// Feature::extractAllTriplets smooths and cuts, Feature.hpp:197-214); frames of another size than the first are skipped.
struct FrameBatch {
  int W = 0, H = 0, nframes = 0;
  std::vector<uint8_t> L, R;
  std::vector<gpc_triplet_points> pts;
  std::vector<int32_t> first = std::vector<int32_t>(1, 0);
  std::vector<std::string> names;  // "<scene>/frame_%04d" of each frame

  bool add(const std::string& name, const ndb::Buffer<uint8_t>& imgL, const ndb::Buffer<uint8_t>& imgR,
           const std::vector<ndb::Point>& kL, const std::vector<ndb::Point>& kR, const std::vector<ndb::Point>& kN) {
    if (nframes == 0) {
      W = imgL.cols();
      H = imgL.rows();
    }
    if (imgL.cols() != W || imgL.rows() != H || imgR.cols() != W || imgR.rows() != H) {
      std::cout << "ERR: frame of another size than the first (" << W << "x" << H << "): skipped" << std::endl;
      return false;
    }
    L.insert(L.end(), imgL.data(), imgL.data() + (size_t)W * H);
    R.insert(R.end(), imgR.data(), imgR.data() + (size_t)W * H);
    for (size_t k = 0; k < kL.size(); ++k)
      pts.push_back(gpc_triplet_points{kL[k].x, kL[k].y, kR[k].x, kR[k].y, kN[k].x, kN[k].y});
    first.push_back((int32_t)pts.size());
    names.push_back(name);
    nframes++;
    return true;
  }

  // the kept triplets' points in set order (Feature.hpp:208-214, then `order`)
  std::vector<gpc_triplet_points> keptInOrder(const std::vector<int32_t>& order) const {
    std::vector<gpc_triplet_points> kept;
    auto inside = [this](int x, int y) { return x > 20 && y > 20 && x < W - 20 && y < H - 20; };
    for (const gpc_triplet_points& p : pts)
      if (inside(p.rx, p.ry) && inside(p.px, p.py) && inside(p.nx, p.ny)) kept.push_back(p);
    std::vector<gpc_triplet_points> out(kept.size());
    for (size_t k = 0; k < kept.size(); ++k) out[order.empty() ? k : order[k]] = kept[k];
    return out;
  }
  int keptCount() const { return (int)keptInOrder(std::vector<int32_t>()).size(); }

  // gpc_hip_extract_triplets on this thread's context, the reference's final shuffle applied as `order`
  DeviceTrainingSet extract(const Generators& gen, std::vector<int32_t>* order_out = nullptr) const {
    const std::vector<int32_t> order = gen.shuffle(keptCount());
    if (order_out) *order_out = order;
    if (order.empty()) return DeviceTrainingSet();
    gpc_hip_ctx* ctx = gpc::inference::detail::holder().ctx;
    if (!ctx) return DeviceTrainingSet();
    gpc_hip_train_set* set = nullptr;
    int n = 0;
    const int st = gpc_hip_extract_triplets(ctx, L.data(), R.data(), W, H, nframes, pts.data(), first.data(), order.data(),
                                            &set, &n);
    if (st != GPC_OK) {
      gpc::inference::detail::fail(st, ctx, "gpc_hip_extract_triplets");
      return DeviceTrainingSet();
    }
    return DeviceTrainingSet(ctx, set, n);
  }
};

// the device set as the reference's host vector (x, y of each descriptor included, Feature.hpp:222-240)
inline std::vector<gpc::training::Feature::GPCPatchTriplet> toHost(const DeviceTrainingSet& dev, const FrameBatch& batch,
                                                                  const std::vector<int32_t>& order) {
  std::vector<gpc::training::Feature::GPCPatchTriplet> data(dev.size());
  if (dev.empty()) return data;
  std::vector<uint8_t> aos((size_t)dev.size() * 3 * 729);
  const int st = dev.read(0, dev.size(), aos.data());
  if (st != GPC_OK) {
    gpc::inference::detail::fail(st, dev.ctx(), "gpc_hip_train_set_read");
    return std::vector<gpc::training::Feature::GPCPatchTriplet>();
  }
  const std::vector<gpc_triplet_points> at = batch.keptInOrder(order);
  for (size_t k = 0; k < data.size(); ++k) {
    gpc::training::Feature::GPCDescriptor* d[3] = {&data[k].ref, &data[k].pos, &data[k].neg};
    const int xy[3][2] = {{at[k].rx, at[k].ry}, {at[k].px, at[k].py}, {at[k].nx, at[k].ny}};
    for (int p = 0; p < 3; ++p) {
      d[p]->feature.resize(27, 27);
      std::memcpy(d[p]->feature.data(), &aos[(k * 3 + p) * 729], 729);
      d[p]->x = xy[p][0];
      d[p]->y = xy[p][1];
    }
  }
  return data;
}

}  // namespace detail
}  // namespace datasource
}  // namespace gpc
#endif
