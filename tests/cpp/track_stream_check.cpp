// track_stream_check -- gpc::tracking::TrackStream (include/gpc/tracking.hpp) compiles and, given a forest and raw frames,
// pushes them one at a time and then all at once: the two runs must deliver the same records, links and ids.
// usage: track_stream_check forest W H N frames.raw   (without arguments: compile check only, prints "ok")
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "gpc/tracking.hpp"

int main(int argc, char** argv) {
  if (argc < 6) {
    std::printf("ok\n");
    return 0;
  }
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), N = std::atoi(argv[4]);
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(argv[1], W, H);
  std::vector<ndb::Buffer<uint8_t>> frames;
  std::ifstream in(argv[5], std::ios::binary);
  for (int f = 0; f < N; ++f) {
    ndb::Buffer<uint8_t> b(H, W);
    in.read(reinterpret_cast<char*>(b.data()), (std::streamsize)W * H);
    frames.push_back(b);
  }
  gpc::inference::InferenceSettings s;
  gpc::tracking::TrackStream one(W, H, fm, s), all(W, H, fm, s);
  if (!one.valid() || !all.valid()) return 2;
  std::vector<gpc::tracking::TrackStream::Pair> a, b = all.push(frames);
  for (int f = 0; f < N; ++f)
    for (auto& p : one.push(frames[(size_t)f])) a.push_back(p);
  if (a.size() != b.size() || (int)a.size() != N - 1 || one.tracksSoFar() != all.tracksSoFar()) return 3;
  for (size_t t = 0; t < a.size(); ++t)
    if (a[t].pair != b[t].pair || a[t].prev != b[t].prev || a[t].trackId != b[t].trackId || a[t].records.size() != b[t].records.size())
      return 4;
  std::printf("TRACKS %d PAIRS %zu\n", (int)one.tracksSoFar(), a.size());
  return 0;
}
