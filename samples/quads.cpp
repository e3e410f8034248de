// quads -- circular matches over a stereo sequence closed into quads (include/gpc/quads.hpp):
//   quads forest.txt L0.png R0.png L1.png R1.png [L2.png R2.png ...]
// matches every stereo frame (epipolar) and both sides over time (optical flow) from one hashing of every image
// (Forest::stereoSequenceQuads), closes the circles L_t -> R_t -> R_t+1 -> L_t+1 -> L_t with a tolerance of one pixel and
// prints the quads per step and an FNV-1a-64 over the records: per step the int32 words (step, quads), then per quad
// (x, y, d0, u, v, d1, support0, support1) as gpc_quad has them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpc/quads.hpp"

namespace {
uint64_t fnv(uint64_t h, int32_t w) {
  for (int k = 0; k < 4; ++k) h = (h ^ (uint64_t)(((uint32_t)w >> (8 * k)) & 0xFFu)) * 1099511628211ull;
  return h;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 6 || (argc % 2) != 0) {
    std::printf("usage: quads forest.txt L0.png R0.png L1.png R1.png [L2.png R2.png ...]\n");
    return 1;
  }
  std::vector<ndb::Buffer<uint8_t>> left, right;
  for (int k = 2; k < argc; ++k) {
    ndb::Buffer<uint8_t> img;
    if (img.readPNG(argv[k])) {
      std::printf("cannot read %s\n", argv[k]);
      return 1;
    }
    if (!left.empty() && (img.cols() != left[0].cols() || img.rows() != left[0].rows())) {
      std::printf("%s: %d x %d, the first image is %d x %d\n", argv[k], img.cols(), img.rows(), left[0].cols(), left[0].rows());
      return 1;
    }
    (k % 2 == 0 ? left : right).push_back(img);
  }
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(argv[1], left[0].cols(), left[0].rows());
  gpc::inference::InferenceSettings stereo(5, 128, 0, true, false, 1);  // rectified pairs: matches within a row
  gpc::inference::InferenceSettings flow(5, 128, 0, false, false, 1);   // over time: no epipolar constraint
  const gpc::inference::time_point t0 = gpc::inference::sysTick();
  std::vector<std::vector<gpc::quads::Quad>> quads = forest.stereoSequenceQuads(left, right, fm, stereo, flow, 1);
  const gpc::inference::time_point t1 = gpc::inference::sysTick();
  if (gpc::inference::lastStatus() != GPC_OK) {
    std::printf("failed: %s\n", gpc::inference::lastError().c_str());
    return 1;
  }
  std::printf("%zu stereo frames, %.2f ms\n", left.size(), gpc::inference::tickToMs(t0, t1));
  uint64_t h = 1469598103934665603ull;
  for (size_t t = 0; t < quads.size(); ++t) {
    std::printf("step %zu: %zu quads\n", t, quads[t].size());
    h = fnv(fnv(h, (int32_t)t), (int32_t)quads[t].size());
    for (const gpc::quads::Quad& q : quads[t]) {
      const int32_t w[8] = {q.l0.x, q.l0.y, q.l0.x - q.r0.x, q.l1.x - q.l0.x, q.l1.y - q.l0.y, q.l1.x - q.r1.x, q.support0, q.support1};
      for (int k = 0; k < 8; ++k) h = fnv(h, w[k]);
    }
  }
  std::printf("fnv %016llx\n", (unsigned long long)h);
  return 0;
}
