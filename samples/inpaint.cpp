// inpaint_fields -- match one rectified pair, fill the matches into a disparity map, clean it and complete it, guided by the
// left image (include/gpc/inpaint.hpp):
//   inpaint_fields forest.txt left.png right.png [cleaned.png completed.png]
// Prints the holes the cleaner leaves, the pixels the completion fills and the holes it leaves (radius 4, range shift 3,
// min weight 512, 32 passes; --radius, --shift, --weight, --passes change them), and writes the disparity before and after
// as 8-bit images: |d| in pixels, clipped to 255, 0 where there is no value.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/clean.hpp"
#include "gpc/inpaint.hpp"

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
  gpc::inpaint::Params ip;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--radius") && i + 1 < argc) ip.radius = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--shift") && i + 1 < argc) ip.rangeShift = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--weight") && i + 1 < argc) ip.minWeight = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--passes") && i + 1 < argc) ip.passes = atoi(argv[++i]);
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3 && pos.size() != 5) {
    std::printf("usage: inpaint_fields forest.txt left.png right.png [cleaned.png completed.png]\n"
                "       options: --radius 1..8 --shift 0..8 (8: unguided) --weight 1..2^24 --passes 1..254\n");
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
  const gpc::clean::Result c = gpc::clean::clean(fwd, &bwd);
  if (c.empty()) return 2;
  const gpc::inpaint::Result r = gpc::inpaint::inpaint(c.field, L, ip);
  if (r.empty()) return 2;
  std::printf("%zu matches; the cleaner leaves %d holes; %d filled, %d left\n", supports.size(), c.stats[1] + c.stats[2] + c.stats[3],
              r.stats[0], r.stats[1]);
  if (pos.size() == 5) {
    writeDisparity(c.field, pos[3]);
    writeDisparity(r.field, pos[4]);
  }
  return 0;
}
