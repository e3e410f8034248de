// search -- match one rectified pair, fill the matches into a disparity map, search the image pair around every pixel of
// it, and clean the result (include/gpc/search.hpp):
//   search forest.txt left.png right.png [filled.png searched.png]
// The forward field is the fill of the supports, searched against (left, right); the backward field the fill of the same
// supports read from the right image's side, searched against (right, left).  Prints what the search did to the forward
// field (radius 2, range 1, sub-pixel, no ceiling; --radius, --range, --whole, --max-cost change them) and what the cleaner
// keeps with and without it, and writes the disparity before and after as 8-bit images: |d| in pixels, clipped to 255, 0
// where there is no value.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
  gpc::search::Params sp;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--radius") && i + 1 < argc) sp.radius = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--range") && i + 1 < argc) sp.range = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--max-cost") && i + 1 < argc) sp.maxCost = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--whole")) sp.subpixel = false;
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3 && pos.size() != 5) {
    std::printf("usage: search forest.txt left.png right.png [filled.png searched.png]\n"
                "       options: --radius 1..4 --range 0..2 --max-cost 0..65535 --whole (no sub-pixel part)\n");
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
  const gpc::search::Result sf = gpc::search::search(fwd, L, R, sp), sb = gpc::search::search(bwd, R, L, sp);
  if (sf.empty() || sb.empty()) return 2;
  const gpc::clean::Result before = gpc::clean::clean(fwd, &bwd), after = gpc::clean::clean(sf.field, &sb.field);
  if (before.empty() || after.empty()) return 2;
  std::printf("%zu matches; search: %d pixels kept, %d without a value, %d without a target inside the image, %d above the ceiling\n",
              supports.size(), sf.stats[0], sf.stats[1], sf.stats[2], sf.stats[3]);
  std::printf("the cleaner keeps %d pixels of the filled field and %d of the searched one\n", before.stats[0], after.stats[0]);
  if (pos.size() == 5) {
    writeDisparity(fwd, pos[3]);
    writeDisparity(sf.field, pos[4]);
  }
  return 0;
}
