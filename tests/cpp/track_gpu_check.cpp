// track_gpu_check -- Forest::trackSequence of include/gpc/tracking.hpp, for pytest.
//   track_gpu_check <forest.txt> <width> <height> <nframes> <frames.raw> <epipolar 0|1> <hashtable 0|1> <minLength>
// frames.raw: nframes frames of width x height bytes.  Prints "TRACKS <number> <fnv1a64>": the hash runs over the int32
// words (firstFrame, number of points, x, y, x, y, ...) of every track in order.  Then trackRecords over sequenceMatch's
// records: "RECORDS <number> <fnv1a64>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpc/tracking.hpp"

static uint64_t fnv(const std::vector<gpc::tracking::Track>& tracks) {
  uint64_t h = 1469598103934665603ull;
  auto word = [&](int32_t v) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(&v);
    for (int i = 0; i < 4; ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  for (const gpc::tracking::Track& t : tracks) {
    word(t.firstFrame);
    word((int32_t)t.points.size());
    for (const ndb::Point& p : t.points) word(p.x), word(p.y);
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), minLength = atoi(argv[8]);
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
  std::vector<gpc::tracking::Track> tracks = forest.trackSequence(frames, fm, s, minLength);
  if (gpc::inference::lastStatus() != GPC_OK) return 4;
  printf("TRACKS %zu %llu\n", tracks.size(), (unsigned long long)fnv(tracks));
  std::vector<std::vector<ndb::Correspondence>> seq = forest.sequenceMatch(frames, fm, s);
  if (gpc::inference::lastStatus() != GPC_OK) return 5;
  std::vector<gpc::tracking::Track> again = gpc::tracking::trackRecords(seq, W, H, minLength);
  if (gpc::inference::lastStatus() != GPC_OK) return 6;
  printf("RECORDS %zu %llu\n", again.size(), (unsigned long long)fnv(again));
  // fewer than two frames: an empty result and a status
  std::vector<ndb::Buffer<uint8_t>> one(1, frames[0]);
  if (!forest.trackSequence(one, fm, s).empty() || gpc::inference::lastStatus() != GPC_E_INVALID) return 7;
  return 0;
}
