// propagate -- match one rectified pair, fill the matches into a disparity map, propagate values between neighbours and
// search the image pair around every pixel of the result (include/gpc/propagate.hpp):
//   propagate forest.txt left.png right.png [--truth disparity.png [--occlusions occlusions.png]]
// Prints what every iteration of the propagation did to the filled field (radius 2, span 1, 6 iterations, 8 neighbours;
// --radius, --span, --iterations, --neighbours change them) and what the search makes of the field with and without it.
// With ground truth (a disparity map in Sintel's RGB encoding; optionally its occlusion mask, which puts the occluded pixels
// into a class of their own) every stage gets the scorer's lines: fill, fill + search, fill + propagate, fill + propagate +
// search.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/dense_evaluation.hpp"
#include "gpc/propagate.hpp"
#include "gpc/search.hpp"

static bool line(const char* stage, const gpc::dense::Field& f, const gpc::evaluation::Truth& truth, const ndb::Buffer<uint8_t>& cls) {
  const gpc::evaluation::FieldScore s = gpc::evaluation::scoreField(f, truth, gpc::evaluation::FieldParams(), &cls);
  if (s.empty()) return false;
  const char* names[3] = {"all", "visible", "occluded"};
  for (int b = -1; b < 2; ++b)
    std::printf("%-26s %-9s density %.4f  epe %7.3f  <1px %.4f  <3px %.4f  <5px %.4f  outliers %.4f  (%lld judged)\n", stage, names[b + 1],
                s.density(b), s.epe(b), s.within(0, b), s.within(1, b), s.within(2, b), s.outlierRate(b), (long long)s.tally(b).n_judged);
  return true;
}

int main(int argc, char** argv) {
  gpc::propagate::Params pp;
  std::vector<std::string> pos;
  std::string truthPath, oclPath;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--radius") && i + 1 < argc) pp.radius = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--span") && i + 1 < argc) pp.span = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--iterations") && i + 1 < argc) pp.iterations = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--neighbours") && i + 1 < argc) pp.neighbours = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--truth") && i + 1 < argc) truthPath = argv[++i];
    else if (!strcmp(argv[i], "--occlusions") && i + 1 < argc) oclPath = argv[++i];
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3) {
    std::printf("usage: propagate forest.txt left.png right.png [--truth disparity.png [--occlusions occlusions.png]]\n"
                "       options: --radius 1..4 --span 1..64 --iterations 1..16 --neighbours 4|8\n");
    return 1;
  }
  ndb::Buffer<uint8_t> L, R;
  if (L.readPNG(pos[1]) || R.readPNG(pos[2]) || L.cols() != R.cols() || L.rows() != R.rows()) return 1;
  const int W = L.cols(), H = L.rows();
  gpc::inference::Forest forest;
  gpc::inference::Forest::FilterMask fm = forest.readForest(pos[0], W, H);
  gpc::inference::InferenceSettings settings(5, 128, 0, true, false, 1);
  const std::vector<ndb::Support> supports = forest.matchPair(L, R, fm, settings);
  if (gpc::inference::lastStatus() != GPC_OK) return 2;
  const gpc::dense::Field fill = gpc::dense::densify(supports, W, H);
  if (fill.empty()) return 2;
  const gpc::propagate::Result pr = gpc::propagate::propagate(fill, L, R, pp);
  if (pr.empty()) return 2;
  const gpc::search::Result plain = gpc::search::search(fill, L, R), after = gpc::search::search(pr.field, L, R);
  if (plain.empty() || after.empty()) return 2;
  std::printf("%zu matches\n", supports.size());
  for (int i = 0; i < pp.iterations; ++i) {
    const int32_t* s = &pr.stats[4 * (size_t)i];
    int stride = pp.span >> (i < 31 ? i : 31);
    std::printf("iteration %d, stride %d: %d pixels kept their own value, %d took a neighbour's, %d without a value, %d without a target "
                "inside the image\n", i, stride < 1 ? 1 : stride, s[gpc::propagate::Own], s[gpc::propagate::Moved],
                s[gpc::propagate::Hole], s[gpc::propagate::Unmatched]);
  }
  long long c0 = 0, c1 = 0, n0 = 0, n1 = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      if (plain.cost(y, x) != 0xFFFF) c0 += plain.cost(y, x), ++n0;
      if (after.cost(y, x) != 0xFFFF) c1 += after.cost(y, x), ++n1;
    }
  std::printf("the search's mean cost: %.2f over %lld pixels of the filled field, %.2f over %lld of the propagated one\n",
              n0 ? (double)c0 / n0 : 0.0, n0, n1 ? (double)c1 / n1 : 0.0, n1);
  if (!truthPath.empty()) {
    ndb::RGBBuffer disp;
    ndb::Buffer<uint8_t> ocl;
    if (disp.readPNGRGB(truthPath) || (!oclPath.empty() && ocl.readPNG(oclPath))) return 1;
    const gpc::evaluation::Truth truth =
        gpc::evaluation::Truth::fromDisparity(disp, ndb::Buffer<uint8_t>(), ndb::Buffer<uint8_t>()).resized(W, H);
    ndb::Buffer<uint8_t> cls(H, W);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) cls(y, x) = y < ocl.rows() && x < ocl.cols() && ocl(y, x) != 0 ? 1 : 0;
    if (!(line("fill", fill, truth, cls) && line("fill, search", plain.field, truth, cls) && line("fill, propagate", pr.field, truth, cls) &&
          line("fill, propagate, search", after.field, truth, cls)))
      return 2;
  }
  return 0;
}
