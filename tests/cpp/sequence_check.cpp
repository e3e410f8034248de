// sequence_check -- Forest::sequenceMatch of include/gpc/inference.hpp against Forest::stereoMatch pair by pair, for pytest.
//   sequence_check <forest.txt> <width> <height> <nframes> <frames.raw> <epipolar 0|1> <hashtable 0|1>
// frames.raw: nframes frames of width x height bytes.  Prints "PAIR <t> <records> <fnv1a64 of the int32 (sx, sy, tx, ty)
// records in output order>" for sequenceMatch and "STEREO <t> <records> <fnv1a64>" for stereoMatch(preprocessImage(f[t]),
// preprocessImage(f[t + 1])).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpc/inference.hpp"

static uint64_t fnv(const std::vector<ndb::Correspondence>& c) {
  uint64_t h = 1469598103934665603ull;  // (the oracle's gpc_oracle_fnv1a64)
  for (const ndb::Correspondence& r : c) {
    const int32_t v[4] = {(int32_t)r.srcPt.x, (int32_t)r.srcPt.y, (int32_t)r.tarPt.x, (int32_t)r.tarPt.y};
    const uint8_t* b = reinterpret_cast<const uint8_t*>(v);
    for (int i = 0; i < 16; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]);
  std::vector<uint8_t> bytes((size_t)W * H * N);
  FILE* f = fopen(argv[5], "rb");
  if (!f) return 3;
  const size_t got = fread(bytes.data(), 1, bytes.size(), f);
  fclose(f);
  if (got != bytes.size()) return 3;
  std::vector<ndb::Buffer<uint8_t>> frames;
  for (int k = 0; k < N; ++k) {
    ndb::Buffer<uint8_t> b(H, W);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) b(y, x) = bytes[((size_t)k * H + y) * W + x];
    frames.push_back(b);
  }
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(argv[1], W, H);
  gpc::inference::InferenceSettings s(5, 128, 0, atoi(argv[6]) != 0, atoi(argv[7]) != 0, 1);
  std::vector<std::vector<ndb::Correspondence>> seq = forest.sequenceMatch(frames, fm, s);
  if (gpc::inference::lastStatus() != GPC_OK || (int)seq.size() != N - 1) return 4;
  for (int t = 0; t < N - 1; ++t) printf("PAIR %d %zu %llu\n", t, seq[t].size(), (unsigned long long)fnv(seq[t]));
  for (int t = 0; t < N - 1; ++t) {
    gpc::inference::Forest::PreprocessedImage a = forest.preprocessImage(frames[t], s);
    gpc::inference::Forest::PreprocessedImage b = forest.preprocessImage(frames[t + 1], s);
    std::vector<ndb::Correspondence> c = forest.stereoMatch(a, b, fm, s);
    if (gpc::inference::lastStatus() != GPC_OK) return 5;
    printf("STEREO %d %zu %llu\n", t, c.size(), (unsigned long long)fnv(c));
  }
  // fewer than two frames: an empty result and a status
  std::vector<ndb::Buffer<uint8_t>> one(1, frames[0]);
  if (!forest.sequenceMatch(one, fm, s).empty() || gpc::inference::lastStatus() != GPC_E_INVALID) return 6;
  return 0;
}
