// gpc/dense_evaluation.hpp -- extension (the reference has no evaluation code): a dense field scored against ground truth on
// the GPU (gpc_hip_score_fields, include/gpc_hip.h has the rule).  The counterpart of gpc/evaluation.hpp for what
// gpc::dense::densify, gpc::search::search, gpc::clean::clean and gpc::inpaint::inpaint return.
//
//   gpc::evaluation::FieldParams                       thresholds, the outlier test, speed bounds (in pixels / per mille)
//   gpc::evaluation::FieldScore                        the exact counts of one field and the rates derived from them
//   gpc::evaluation::scoreField(field, truth, p, cls)  one FieldScore from a Field and a Truth of its size
//
// The library returns counts only; epe(), rms(), within(k), outlierRate() and density() divide them here, over all judged
// pixels or (bin = 0 .. 3) over one class or speed bin, and return 0 where nothing was judged.
// Errors are reported as everywhere in inference.hpp: an empty FieldScore and lastStatus() / lastError().
#ifndef GPC_AMD_DENSE_EVALUATION_HPP
#define GPC_AMD_DENSE_EVALUATION_HPP

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gpc/dense.hpp"
#include "gpc/evaluation.hpp"

namespace gpc {
namespace evaluation {

struct FieldParams {
  std::vector<int> thresholdsQ8 = {256, 768, 1280};  // at most 8, each 0 .. 65535 in 1/256 pixel
  int outlierAbsQ8 = 768;                            // KITTI's D1 / Fl: more than 3 pixels ...
  int outlierRelPm = 50;                             // ... and more than 5 % of the true magnitude; 0: the absolute test alone
  std::vector<int> speedsQ8;                         // at most 3, ascending; Sintel's s0-10 / s10-40 / s40+: {2560, 10240}
  bool wantError = false;                            // fill FieldScore::error
  gpc_field_score_prm toC() const {
    gpc_field_score_prm c;
    std::memset(&c, 0, sizeof c);
    c.n_thr = (int32_t)thresholdsQ8.size();
    for (size_t k = 0; k < thresholdsQ8.size() && k < 8; ++k) c.thr_q8[k] = thresholdsQ8[k];
    c.out_abs_q8 = outlierAbsQ8, c.out_rel_pm = outlierRelPm;
    c.n_speed = (int32_t)speedsQ8.size();
    for (size_t k = 0; k < speedsQ8.size() && k < 3; ++k) c.speed_q8[k] = speedsQ8[k];
    return c;
  }
};

struct FieldScore {
  gpc_field_score counts;
  ndb::Buffer<uint16_t> error;  // with wantError: min(e, 0xFFFE) in 1/256 pixel for a judged pixel, 0xFFFF for every other
  bool valid = false;
  FieldScore() { std::memset(&counts, 0, sizeof counts); }
  bool empty() const { return !valid; }
  const gpc_field_tally& tally(int bin = -1) const { return bin < 0 ? counts.all : counts.bin[bin]; }
  double epe(int bin = -1) const { return ratio((double)tally(bin).sum_e_q8, 256.0 * (double)tally(bin).n_judged); }
  double rms(int bin = -1) const { return std::sqrt(ratio((double)tally(bin).sum_e2_q16, 65536.0 * (double)tally(bin).n_judged)); }
  double within(int k, int bin = -1) const { return ratio((double)tally(bin).n_within[k], (double)tally(bin).n_judged); }
  double outlierRate(int bin = -1) const { return ratio((double)tally(bin).n_outlier, (double)tally(bin).n_judged); }
  // judged pixels over the pixels that could be judged (judged + holes); with a bin, the bin's share of them
  double density(int bin = -1) const { return ratio((double)tally(bin).n_judged, (double)(counts.all.n_judged + counts.n_hole)); }

 private:
  static double ratio(double a, double b) { return b > 0 ? a / b : 0.0; }
};

inline FieldScore scoreField(const gpc::dense::Field& f, const Truth& truth, const FieldParams& p = FieldParams(),
                             const ndb::Buffer<uint8_t>* cls = nullptr) {
  namespace inf = gpc::inference;
  const bool shaped = !f.empty() && f.width >= 1 && f.height >= 1 && (f.channels == 1 || f.channels == 2) &&
                      (int)f.value.size() == f.channels && truth.consistent() && truth.width == f.width && truth.height == f.height &&
                      truth.flow() == (f.channels == 2) && (!cls || (cls->width == f.width && cls->height == f.height)) &&
                      p.thresholdsQ8.size() <= 8 && p.speedsQ8.size() <= 3;
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_score_fields");
    return FieldScore();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return FieldScore();
  const int W = f.width, H = f.height, C = f.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> in((size_t)C * n);
  std::vector<uint8_t> c(cls ? n : 0);
  std::vector<uint16_t> err(p.wantError ? n : 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      for (int k = 0; k < C; ++k) in[(size_t)k * n + at] = f.value[(size_t)k](y, x);
      if (cls) c[at] = (*cls)(y, x);
    }
  const gpc_field_score_prm prm = p.toC();
  const gpc_truth t = truth.toC();
  FieldScore res;
  const int st = gpc_hip_score_fields(h.ctx, in.data(), C, W, H, 1, &t, &prm, cls ? c.data() : nullptr, &res.counts,
                                      p.wantError ? err.data() : nullptr);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_score_fields");
    return FieldScore();
  }
  res.valid = true;
  if (p.wantError) {
    res.error = ndb::Buffer<uint16_t>(H, W);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) res.error(y, x) = err[(size_t)y * W + x];
  }
  return res;
}

}  // namespace evaluation
}  // namespace gpc
#endif
