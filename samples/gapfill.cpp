// gapfill -- match one rectified pair in both directions, fill, search and clean, then close the cleaned field's holes along
// scanlines from the background side and complete what is left (include/gpc/gapfill.hpp):
//   gapfill_fields forest.txt left.png right.png [--truth disparity.png [--occlusions occlusions.png]]
// Prints how many holes each kind of closing took (--max-gap, --discon, --select 0|1, --border 0|1 change the parameters) and
// how many the completion closed afterwards.  With ground truth (a disparity map in Sintel's RGB encoding; optionally its
// occlusion mask, which puts the occluded pixels into a class of their own) every arm gets the scorer's lines: clean,
// clean + complete, clean + gapfill, clean + gapfill + complete.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/clean.hpp"
#include "gpc/dense_evaluation.hpp"
#include "gpc/gapfill.hpp"
#include "gpc/inpaint.hpp"
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
  gpc::gapfill::Params gp;
  std::vector<std::string> pos;
  std::string truthPath, oclPath;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--max-gap") && i + 1 < argc) gp.maxGap = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--discon") && i + 1 < argc) gp.discon = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--select") && i + 1 < argc) gp.select = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--border") && i + 1 < argc) gp.border = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--truth") && i + 1 < argc) truthPath = argv[++i];
    else if (!strcmp(argv[i], "--occlusions") && i + 1 < argc) oclPath = argv[++i];
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 3) {
    std::printf("usage: gapfill_fields forest.txt left.png right.png [--truth disparity.png [--occlusions occlusions.png]]\n"
                "       options: --max-gap 1..32767 --discon 0..16777216 --select 0|1 --border 0|1\n");
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
  const gpc::dense::Field fill_f = gpc::dense::densify(supports, W, H), fill_b = gpc::dense::densify(gpc::clean::reversed(supports), W, H);
  if (fill_f.empty() || fill_b.empty()) return 2;
  const gpc::search::Result fwd = gpc::search::search(fill_f, L, R), bwd = gpc::search::search(fill_b, R, L);
  if (fwd.empty() || bwd.empty()) return 2;
  const gpc::clean::Result cl = gpc::clean::clean(fwd.field, &bwd.field);
  if (cl.empty()) return 2;
  const gpc::gapfill::Result gf = gpc::gapfill::gapfill(cl.field, L, gp);
  if (gf.empty()) return 2;
  const gpc::inpaint::Result today = gpc::inpaint::inpaint(cl.field, L), after = gpc::inpaint::inpaint(gf.field, L);
  if (today.empty() || after.empty()) return 2;
  std::printf("%zu matches\n", supports.size());
  std::printf("gapfill: %d holes interpolated between agreeing ends, %d took one end of a depth edge, %d the end beside the border, %d left\n",
              gf.stats[gpc::gapfill::Continuous], gf.stats[gpc::gapfill::Edge], gf.stats[gpc::gapfill::Border], gf.stats[gpc::gapfill::HolesLeft]);
  long long rows = 0, cols = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int k = gf.how(y, x);
      rows += k >= gpc::gapfill::RowContinuous && k <= gpc::gapfill::RowBorder;
      cols += k >= gpc::gapfill::ColumnContinuous && k <= gpc::gapfill::ColumnBorder;
    }
  std::printf("         %lld along their row, %lld along their column\n", rows, cols);
  if (!truthPath.empty()) {
    ndb::RGBBuffer disp;
    ndb::Buffer<uint8_t> ocl;
    if (disp.readPNGRGB(truthPath) || (!oclPath.empty() && ocl.readPNG(oclPath))) return 1;
    const gpc::evaluation::Truth truth =
        gpc::evaluation::Truth::fromDisparity(disp, ndb::Buffer<uint8_t>(), ndb::Buffer<uint8_t>()).resized(W, H);
    ndb::Buffer<uint8_t> cls(H, W);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) cls(y, x) = y < ocl.rows() && x < ocl.cols() && ocl(y, x) != 0 ? 1 : 0;
    if (!(line("clean", cl.field, truth, cls) && line("clean, complete", today.field, truth, cls) &&
          line("clean, gapfill", gf.field, truth, cls) && line("clean, gapfill, complete", after.field, truth, cls)))
      return 2;
  }
  return 0;
}
