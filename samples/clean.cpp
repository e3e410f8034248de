// clean -- match one rectified pair, fill the matches into a disparity map, and clean it (include/gpc/clean.hpp):
//   clean forest.txt left.png right.png [before.png after.png]
// The forward field is the fill of the supports, the backward field the fill of the same supports read from the right
// image's side (no second match).  Prints the number of pixels kept, without a value, failing the left-right check and
// removed as speckles (check 256, diff 256, min 64, median 1; --tol, --diff, --min, --median change them), and writes the
// disparity before and after as 8-bit images: |d| in pixels, clipped to 255, 0 where there is no value.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/clean.hpp"

static void writeDisparity(const gpc::dense::Field& f, const std::string& path) {
  ndb::Buffer<uint8_t> img(f.height, f.width);
  for (int y = 0; y < f.height; ++y)
    for (int x = 0; x < f.width; ++x) {
      const int32_t v = f.value[0](y, x);
      const long d = v == GPC_DENSE_NONE ? 0 : (std::labs((long)v) + 128) >> 8;
      img(y, x) = (uint8_t)(d > 255 ? 255 : d);
    }
  img.writePNG(path);
}

int main(int argc, char** argv) {
  gpc::clean::Params cp;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--tol") && i + 1 < argc) cp.checkTol = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--diff") && i + 1 < argc) cp.speckleDiff = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--min") && i + 1 < argc) cp.speckleMin = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--median") && i + 1 < argc) cp.medianRadius = atoi(argv[++i]);
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3 && pos.size() != 5) {
    std::printf("usage: clean forest.txt left.png right.png [before.png after.png]\n"
                "       options: --tol Q8 (-1: no check) --diff Q8 --min PIXELS --median 0|1|2\n");
    return 1;
  }
  ndb::Buffer<uint8_t> L, R;
  if (L.readPNG(pos[1]) || R.readPNG(pos[2]) || L.cols() != R.cols() || L.rows() != R.rows()) return 1;
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(pos[0], L.cols(), L.rows());
  gpc::inference::InferenceSettings settings(5, 128, 0, true, false, 1);
  const std::vector<ndb::Support> supports = forest.matchPair(L, R, fm, settings);
  if (gpc::inference::lastStatus() != GPC_OK) return 2;
  const gpc::dense::Field fwd = gpc::dense::densify(supports, L.cols(), L.rows());
  const gpc::dense::Field bwd = gpc::dense::densify(gpc::clean::reversed(supports), L.cols(), L.rows());
  if (fwd.empty() || bwd.empty()) return 2;
  const gpc::clean::Result r = gpc::clean::clean(fwd, cp.checkTol >= 0 ? &bwd : nullptr, cp);
  if (r.empty()) return 2;
  std::printf("%zu matches; %d pixels kept, %d without a value, %d fail the check, %d speckles\n", supports.size(), r.stats[0],
              r.stats[1], r.stats[2], r.stats[3]);
  if (pos.size() == 5) {
    writeDisparity(fwd, pos[3]);
    writeDisparity(r.field, pos[4]);
  }
  return 0;
}
