// tracks -- point tracks over a frame sequence (include/gpc/tracking.hpp):
//   tracks forest.txt frame0.png frame1.png [frame2.png ...]
// matches every consecutive pair of frames (Forest::trackSequence: each frame preprocessed and hashed once, the matches
// chained on the device) and prints the number of tracks and a histogram of their lengths in records: a track of length
// n follows one point through n + 1 frames.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "gpc/tracking.hpp"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::printf("usage: tracks forest.txt frame0.png frame1.png [frame2.png ...]\n");
    return 1;
  }
  std::vector<ndb::Buffer<uint8_t>> frames;
  for (int k = 2; k < argc; ++k) {
    ndb::Buffer<uint8_t> img;
    if (img.readPNG(argv[k])) {
      std::printf("cannot read %s\n", argv[k]);
      return 1;
    }
    if (!frames.empty() && (img.cols() != frames[0].cols() || img.rows() != frames[0].rows())) {
      std::printf("%s: %d x %d, the first frame is %d x %d\n", argv[k], img.cols(), img.rows(), frames[0].cols(), frames[0].rows());
      return 1;
    }
    frames.push_back(img);
  }
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(argv[1], frames[0].cols(), frames[0].rows());
  gpc::inference::InferenceSettings settings(5, 128, 0, false, false, 1);  // optical flow: no epipolar constraint
  const gpc::inference::time_point t0 = gpc::inference::sysTick();
  std::vector<gpc::tracking::Track> tracks = forest.trackSequence(frames, fm, settings);
  const gpc::inference::time_point t1 = gpc::inference::sysTick();
  if (gpc::inference::lastStatus() != GPC_OK) return 1;
  std::map<size_t, size_t> hist;
  for (const gpc::tracking::Track& t : tracks) ++hist[t.points.size() - 1];
  std::printf("%zu frames, %zu tracks, %.2f ms\n", frames.size(), tracks.size(), gpc::inference::tickToMs(t0, t1));
  for (const auto& kv : hist) std::printf("length %3zu: %zu\n", kv.first, kv.second);
  return 0;
}
