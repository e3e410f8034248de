// evaluate_dense -- the dense chain against Sintel's ground truth, stage by stage (include/gpc/dense_evaluation.hpp):
//   evaluate_dense forest.txt <sintel stereo root> [scene] [frame]
// Reads one stereo pair through the datasource of gpc/SintelStereo.hpp, matches it, and scores the forward disparity field
// after each stage of the chain with the library's defaults: after the fill (gpc::dense::densify), after the search
// (gpc::search::search), after the cleaner (gpc::clean::clean) and after the completion (gpc::inpaint::inpaint).  Truth is
// the integer-decoded disparity; out-of-frame pixels are ignored, and the occlusion mask is the class plane, so that every
// figure is printed for all judged pixels, for the visible ones (class 0) and for the occluded ones (class 1).  One table
// line per stage and class: density, end-point error, the share within 1 / 3 / 5 pixels, the outlier rate (3 px and 5 %).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gpc/clean.hpp"
#include "gpc/dense_evaluation.hpp"
#include "gpc/inpaint.hpp"
#include "gpc/search.hpp"

static bool line(const char* stage, const gpc::dense::Field& f, const gpc::evaluation::Truth& truth, const ndb::Buffer<uint8_t>& cls) {
  const gpc::evaluation::FieldScore s = gpc::evaluation::scoreField(f, truth, gpc::evaluation::FieldParams(), &cls);
  if (s.empty()) return false;
  const char* names[3] = {"all", "visible", "occluded"};
  for (int b = -1; b < 2; ++b)
    std::printf("%-9s %-9s density %.4f  epe %7.3f  <1px %.4f  <3px %.4f  <5px %.4f  outliers %.4f  (%lld judged)\n", stage, names[b + 1],
                s.density(b), s.epe(b), s.within(0, b), s.within(1, b), s.within(2, b), s.outlierRate(b), (long long)s.tally(b).n_judged);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: evaluate_dense forest.txt <sintel stereo root> [scene] [frame]\n");
    return 1;
  }
  const std::string scene = argc > 3 ? argv[3] : "alley_1";
  const int id = argc > 4 ? atoi(argv[4]) : 1;
  gpc::datasource::SintelStereo src(argv[2]);
  if (src.selectScene(scene)) return 1;
  ndb::Buffer<uint8_t> L, R, ocl, oof;
  ndb::RGBBuffer disp;
  if (src.getBW(id, L, R) | src.getDisparity(id, disp) | src.getOcclusion(id, ocl) | src.getInvalid(id, oof)) return 1;
  if (disp.cols() < ocl.cols() - 15 || disp.rows() != L.rows() || ocl.rows() != L.rows() || oof.rows() != L.rows()) return 1;
  const int W = L.cols(), H = L.rows();
  // occluded pixels are judged, in a class of their own; what lies outside the other view (and the padding) is ignored
  const gpc::evaluation::Truth truth = gpc::evaluation::Truth::fromDisparity(disp, ndb::Buffer<uint8_t>(), oof).resized(W, H);
  ndb::Buffer<uint8_t> cls(H, W);
  for (int y = 0; y < H && y < ocl.rows(); ++y)
    for (int x = 0; x < W && x < ocl.cols(); ++x) cls(y, x) = ocl.getPixel(x, y) != 0 ? 1 : 0;

  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(argv[1], W, H);
  gpc::inference::InferenceSettings settings(5, 128, 0, true, false, 1);
  const std::vector<ndb::Support> supports = forest.matchPair(L, R, fm, settings);
  if (gpc::inference::lastStatus() != GPC_OK) return 2;
  const gpc::dense::Field fwd = gpc::dense::densify(supports, W, H), bwd = gpc::dense::densify(gpc::clean::reversed(supports), W, H);
  if (fwd.empty() || bwd.empty()) return 2;
  const gpc::search::Result sf = gpc::search::search(fwd, L, R), sb = gpc::search::search(bwd, R, L);
  if (sf.empty() || sb.empty()) return 2;
  const gpc::clean::Result cleaned = gpc::clean::clean(sf.field, &sb.field);
  if (cleaned.empty()) return 2;
  const gpc::inpaint::Result done = gpc::inpaint::inpaint(cleaned.field, L);
  if (done.empty()) return 2;
  std::printf("%s frame %d, %d x %d, %zu matches\n", scene.c_str(), id, W, H, supports.size());
  return line("fill", fwd, truth, cls) && line("search", sf.field, truth, cls) && line("clean", cleaned.field, truth, cls) &&
                 line("complete", done.field, truth, cls)
             ? 0
             : 2;
}
