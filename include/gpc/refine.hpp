// refine.hpp -- sub-pixel position and photometric cost of matches (extension; the reference matches one pair and leaves
// every use of the result to its caller).  The windows around the two ends of a match are compared: the sum of absolute
// differences is the match's cost, the costs at the neighbouring target positions give the sub-pixel position; integers
// only, run on the device by gpc_hip_refine_* (include/gpc_hip.h has the rule).
//
//   gpc::refine::Result                                  dx, dy in pixels, cost, evaluated / minimumX / minimumY
//   gpc::refine::refine(records, left, right, w, h, r)   one Result per correspondence / support of one pair
//   gpc::refine::refined(supports, results)              the supports with d moved to the sub-pixel position
//
// left / right: w * h bytes each, raw or smoothed as the caller likes.  No forest is needed.  Errors are reported as
// everywhere in inference.hpp: an empty result and lastStatus() / lastError().
#ifndef GPC_AMD_REFINE_HPP
#define GPC_AMD_REFINE_HPP

#include <cstdint>
#include <vector>

#include "gpc/consensus.hpp"
#include "gpc/inference.hpp"

namespace gpc {
namespace refine {

struct Result {
  float dx = 0.f, dy = 0.f;   // the target's sub-pixel shift in pixels, -0.5 .. 0.5
  int cost = 0xFFFF;          // sum of absolute differences at the integer position; 0xFFFF: not evaluated
  bool evaluated = false;     // every window lay inside the image (and a support's d was a whole number)
  bool minimumX = false;      // the integer position is a local minimum of the cost along x
  bool minimumY = false;      // ... along y (correspondences only)
};

namespace detail {
inline Result fromC(const gpc_refinement& r) {
  Result o;
  o.dx = (float)r.dx_q8 * 0.00390625f, o.dy = (float)r.dy_q8 * 0.00390625f;
  o.cost = r.cost;
  o.evaluated = (r.flags & 1) != 0, o.minimumX = (r.flags & 2) != 0, o.minimumY = (r.flags & 4) != 0;
  return o;
}
inline int call(gpc_hip_ctx* ctx, const gpc_correspondence* r, int cap, const int32_t* n, const uint8_t* l, const uint8_t* rt, int w,
                int h, int radius, gpc_refinement* out) {
  return gpc_hip_refine_correspondences(ctx, r, cap, n, l, rt, w, h, 1, radius, out);
}
inline int call(gpc_hip_ctx* ctx, const gpc_support* r, int cap, const int32_t* n, const uint8_t* l, const uint8_t* rt, int w, int h,
                int radius, gpc_refinement* out) {
  return gpc_hip_refine_supports(ctx, r, cap, n, l, rt, w, h, 1, radius, out, nullptr);
}

template <class Rec, class CRec>
std::vector<Result> refineOne(const std::vector<Rec>& records, const uint8_t* left, const uint8_t* right, int width, int height,
                              int radius) {
  namespace inf = gpc::inference;
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return std::vector<Result>();
  if (records.empty()) return std::vector<Result>();
  std::vector<CRec> rec(records.size());
  for (size_t i = 0; i < records.size(); ++i) rec[i] = gpc::consensus::detail::toC(records[i]);
  std::vector<gpc_refinement> out(records.size());
  const int32_t n = (int32_t)records.size();
  const int st = call(h.ctx, rec.data(), (int)records.size(), &n, left, right, width, height, radius, out.data());
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_refine");
    return std::vector<Result>();
  }
  std::vector<Result> res(records.size());
  for (size_t i = 0; i < records.size(); ++i) res[i] = fromC(out[i]);
  return res;
}
}  // namespace detail

inline std::vector<Result> refine(const std::vector<ndb::Correspondence>& records, const uint8_t* left, const uint8_t* right, int width,
                                  int height, int radius = 3) {
  return detail::refineOne<ndb::Correspondence, gpc_correspondence>(records, left, right, width, height, radius);
}
inline std::vector<Result> refine(const std::vector<ndb::Support>& records, const uint8_t* left, const uint8_t* right, int width,
                                  int height, int radius = 3) {
  return detail::refineOne<ndb::Support, gpc_support>(records, left, right, width, height, radius);
}

// the supports with d = d - dx (the target moves by +dx, so the disparity x - tx shrinks by it); one float32 subtraction
inline std::vector<ndb::Support> refined(const std::vector<ndb::Support>& supports, const std::vector<Result>& results) {
  std::vector<ndb::Support> out(supports);
  for (size_t i = 0; i < out.size() && i < results.size(); ++i) out[i].d = out[i].d - results[i].dx;
  return out;
}

}  // namespace refine
}  // namespace gpc
#endif
