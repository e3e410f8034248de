// aggregate -- match one rectified pair, fill the matches into a disparity map, choose among the search's candidates around
// every pixel of it by costs aggregated along scanlines, and clean the result (include/gpc/aggregate.hpp):
//   aggregate forest.txt left.png right.png [filled.png aggregated.png]
// The forward field is the fill of the supports, aggregated against (left, right); the backward field the fill of the same
// supports read from the right image's side, aggregated against (right, left).  Prints what the stage did to the forward
// field (radius 2, range 1, sub-pixel, no ceiling, p1 128, p2 512, all four paths; --radius, --range, --whole, --max-cost, --p1,
// --p2, --paths change them), at how many pixels its choice differs from the search's, and what the cleaner keeps with and
// without it, and writes the disparity before and after as 8-bit images: |d| in pixels, clipped to 255, 0 where there is no
// value.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/aggregate.hpp"
#include "gpc/clean.hpp"
#include "gpc/search.hpp"

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
  gpc::aggregate::Params ap;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--radius") && i + 1 < argc) ap.radius = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--range") && i + 1 < argc) ap.range = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--max-cost") && i + 1 < argc) ap.maxCost = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--p1") && i + 1 < argc) ap.p1 = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--p2") && i + 1 < argc) ap.p2 = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--paths") && i + 1 < argc) ap.paths = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--whole")) ap.subpixel = false;
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3 && pos.size() != 5) {
    std::printf("usage: aggregate forest.txt left.png right.png [filled.png aggregated.png]\n"
                "       options: --radius 1..4 --range 0..2 --max-cost 0..65535 --whole (no sub-pixel part)\n"
                "                --p1 0..32767 --p2 p1..32767 --paths 0..15 (1 right, 2 left, 4 down, 8 up)\n");
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
  const gpc::aggregate::Result af = gpc::aggregate::aggregate(fwd, L, R, ap), ab = gpc::aggregate::aggregate(bwd, R, L, ap);
  gpc::search::Params sp;
  sp.radius = ap.radius, sp.range = ap.range, sp.subpixel = ap.subpixel, sp.maxCost = ap.maxCost;
  const gpc::search::Result sf = gpc::search::search(fwd, L, R, sp);
  if (af.empty() || ab.empty() || sf.empty()) return 2;
  long differ = 0;
  for (int y = 0; y < L.rows(); ++y)
    for (int x = 0; x < L.cols(); ++x) differ += af.choice(y, x) != sf.choice(y, x);
  const gpc::clean::Result before = gpc::clean::clean(fwd, &bwd), after = gpc::clean::clean(af.field, &ab.field);
  if (before.empty() || after.empty()) return 2;
  std::printf("%zu matches; aggregate: %d pixels kept, %d without a value, %d without a target inside the image, %d above the ceiling\n",
              supports.size(), af.stats[0], af.stats[1], af.stats[2], af.stats[3]);
  std::printf("its choice differs from the search's at %ld pixels\n", differ);
  std::printf("the cleaner keeps %d pixels of the filled field and %d of the aggregated one\n", before.stats[0], after.stats[0]);
  if (pos.size() == 5) {
    writeDisparity(fwd, pos[3]);
    writeDisparity(af.field, pos[4]);
  }
  return 0;
}
