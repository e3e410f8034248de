// clean.hpp -- cleaning a dense field (extension; the reference writes disparity.png from the raw supports): the
// left-right (forward-backward) consistency check against the field of the reversed records, the removal of small
// connected segments and a small median; integers only, run on the device by gpc_hip_clean_fields (include/gpc_hip.h has
// the rule).
//
//   gpc::clean::Params                       checkTol, speckleDiff (both in 1/256 pixel), speckleMin, medianRadius
//   gpc::clean::Result                       field (the kept values), state, label, stats
//   gpc::clean::reversed(records)            the records read from their target's side: densify them for the backward field
//   gpc::clean::clean(fwd, bwd, params)      one Result from the forward field and (optionally) the backward field
//
// The matcher is symmetric, so the backward field costs no second match:
//   Field fwd = gpc::dense::densify(supports, w, h), bwd = gpc::dense::densify(gpc::clean::reversed(supports), w, h);
//   gpc::clean::Result r = gpc::clean::clean(fwd, &bwd);
// Without bwd the check must be off (checkTol = -1).  Errors are reported as everywhere in inference.hpp: an empty Result
// and lastStatus() / lastError().
#ifndef GPC_AMD_CLEAN_HPP
#define GPC_AMD_CLEAN_HPP

#include <cmath>
#include <cstdint>
#include <vector>

#include "gpc/dense.hpp"

namespace gpc {
namespace clean {

struct Params {
  int checkTol = 256;     // -1: no cross-check; else the largest |forward + backward| a pixel may show, in 1/256 pixel
  int speckleDiff = 256;  // 4-neighbours belong together when they differ by at most this, in 1/256 pixel
  int speckleMin = 64;    // a connected segment of fewer pixels is removed; 0 and 1: none
  int medianRadius = 1;   // 0: none, 1: 3x3, 2: 5x5
  gpc_clean toC() const { return gpc_clean{checkTol, speckleDiff, speckleMin, medianRadius}; }
};

enum State : uint8_t { Kept = 0, None = 1, FailedCheck = 2, Speckle = 3 };

struct Result {
  gpc::dense::Field field;      // the kept pixels' values (the median of their kept neighbourhood); GPC_DENSE_NONE elsewhere
  ndb::Buffer<uint8_t> state;   // a State per pixel
  ndb::Buffer<int32_t> label;   // the lowest pixel index of the pixel's segment; -1 where it has no value or failed the check
  int32_t stats[4] = {0, 0, 0, 0};  // pixels per State
  bool empty() const { return field.empty(); }
};

// (x, y, d) -> (x - d, y, -d); a support whose d is not a whole number below 2^24 becomes (-1, -1, 0), which no fill takes
inline std::vector<ndb::Support> reversed(const std::vector<ndb::Support>& records) {
  std::vector<ndb::Support> out(records.size());
  for (size_t i = 0; i < records.size(); ++i) {
    const float d = records[i].d;
    const bool whole = d == std::trunc(d) && std::fabs(d) < 16777216.f;
    out[i] = whole ? ndb::Support((int)((uint32_t)records[i].x - (uint32_t)(int)d), records[i].y, -d) : ndb::Support(-1, -1, 0.f);
  }
  return out;
}
inline std::vector<ndb::Correspondence> reversed(const std::vector<ndb::Correspondence>& records) {
  std::vector<ndb::Correspondence> out(records.size());
  for (size_t i = 0; i < records.size(); ++i) out[i] = ndb::Correspondence(records[i].tarPt, records[i].srcPt);
  return out;
}
// the sub-pixel shifts of the reversed records
inline std::vector<gpc::refine::Result> reversed(const std::vector<gpc::refine::Result>& results) {
  std::vector<gpc::refine::Result> out(results);
  for (gpc::refine::Result& r : out) r.dx = -r.dx, r.dy = -r.dy;
  return out;
}

namespace detail {
inline void planes(const gpc::dense::Field& f, std::vector<int32_t>& out) {
  const size_t n = (size_t)f.width * (size_t)f.height;
  out.resize((size_t)f.channels * n);
  for (int c = 0; c < f.channels; ++c)
    for (int y = 0; y < f.height; ++y)
      for (int x = 0; x < f.width; ++x) out[(size_t)c * n + (size_t)y * f.width + x] = f.value[(size_t)c](y, x);
}
}  // namespace detail

inline Result clean(const gpc::dense::Field& fwd, const gpc::dense::Field* bwd = nullptr, const Params& p = Params()) {
  namespace inf = gpc::inference;
  const bool shaped = !fwd.empty() && fwd.width >= 1 && fwd.height >= 1 && (int)fwd.value.size() == fwd.channels &&
                      (!bwd || (bwd->width == fwd.width && bwd->height == fwd.height && bwd->channels == fwd.channels &&
                                bwd->value.size() == fwd.value.size()));
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_clean_fields");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int W = fwd.width, H = fwd.height, C = fwd.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> f, g, out((size_t)C * n), label(n);
  std::vector<uint8_t> state(n);
  detail::planes(fwd, f);
  if (bwd) detail::planes(*bwd, g);
  const gpc_clean prm = p.toC();
  Result r;
  const int st = gpc_hip_clean_fields(h.ctx, f.data(), bwd ? g.data() : nullptr, C, W, H, 1, &prm, out.data(), state.data(),
                                      label.data(), r.stats);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_clean_fields");
    return Result();
  }
  r.field.width = W, r.field.height = H, r.field.channels = C;
  r.field.level = fwd.level;
  r.state = ndb::Buffer<uint8_t>(H, W);
  r.label = ndb::Buffer<int32_t>(H, W);
  for (int c = 0; c < C; ++c) r.field.value.emplace_back(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      r.state(y, x) = state[at];
      r.label(y, x) = label[at];
      for (int c = 0; c < C; ++c) r.field.value[(size_t)c](y, x) = out[(size_t)c * n + at];
    }
  return r;
}

}  // namespace clean
}  // namespace gpc
#endif
