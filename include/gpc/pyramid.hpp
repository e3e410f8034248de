// pyramid.hpp -- matching over an image pyramid (extension; the reference matches at one resolution).  Every level of the
// 2x2-mean pyramid of a pair is matched with the same forest (its tests are offsets within the 27x27 patch) and the levels'
// supports are merged into one list in level 0's coordinates: level 0 whole, then the coarser levels' records whose block
// holds no record kept before; integers only, run on the device by gpc_hip_pyramid_* (include/gpc_hip.h has the rules).
//
//   gpc::pyramid::levels(w, h, levels, widths, heights)              the levels' sizes; false where the geometry is refused
//   gpc::pyramid::Result                                             supports, and how many of them each level gave
//   gpc::pyramid::matchPair(left, right, forestmask, settings, n)    the merged supports of one raw pair over n levels
//
// A support of level l stands for a 2^l x 2^l block (its top-left corner is reported) and carries d * 2^l.  Errors are
// reported as everywhere in inference.hpp: an empty result and lastStatus() / lastError().
#ifndef GPC_AMD_PYRAMID_HPP
#define GPC_AMD_PYRAMID_HPP

#include <cstdint>
#include <cstring>
#include <vector>

#include "gpc/consensus.hpp"
#include "gpc/inference.hpp"

namespace gpc {
namespace pyramid {

inline bool levels(int width, int height, int nlevels, int* widths, int* heights) {
  int32_t w[GPC_MAX_PYRAMID_LEVELS], h[GPC_MAX_PYRAMID_LEVELS];
  if (gpc_hip_pyramid_levels(width, height, nlevels, w, h) != GPC_OK) return false;
  for (int l = 0; l < nlevels; ++l) {
    if (widths) widths[l] = w[l];
    if (heights) heights[l] = h[l];
  }
  return true;
}

struct Result {
  std::vector<ndb::Support> supports;  // level 0's, then level 1's kept ones, ...
  std::vector<int> perLevel;           // supports of each level: their sum is supports.size()
};

inline Result matchPair(ndb::Buffer<uint8_t>& left, ndb::Buffer<uint8_t>& right, const gpc::inference::Forest::FilterMask& forestmask,
                        gpc::inference::InferenceSettings settings, int nlevels) {
  namespace inf = gpc::inference;
  Result res;
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return res;
  const int W = left.cols(), H = left.rows();
  if (right.cols() != W || right.rows() != H || nlevels < 1 || nlevels > GPC_MAX_PYRAMID_LEVELS) {
    inf::detail::fail(GPC_E_INVALID, h.ctx, "gpc_hip_pyramid_batch");
    return res;
  }
  gpc_filter_mask fm;
  memset(&fm, 0, sizeof fm);
  fm.num_tests = (int)(forestmask.mask.size() / 2);
  if (fm.num_tests > GPC_MAX_TESTS) fm.num_tests = GPC_MAX_TESTS;
  for (int i = 0; i < 2 * fm.num_tests; ++i) fm.mask[i] = forestmask.mask[i];
  for (int i = 0; i < fm.num_tests && i < (int)forestmask.tau.size(); ++i) fm.tau[i] = forestmask.tau[i];
  fm.type = forestmask.type, fm.width = forestmask.width, fm.height = forestmask.height;
  int st = gpc_hip_set_forest(h.ctx, &fm);  // (the same forest again costs nothing)
  h.have = false;                           // Forest's own calls hand theirs over again
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_set_forest");
    return res;
  }
  const gpc_settings s = settings.toC();
  int cap = (W - 2 * GPC_PATCH_RADIUS) * (H - 2 * GPC_PATCH_RADIUS) + 1;  // level 0's every record; the levels add a third at most
  cap += cap / 2;
  std::vector<gpc_support> out((size_t)cap);
  int32_t count = 0, per[GPC_MAX_PYRAMID_LEVELS] = {0, 0, 0, 0};
  st = gpc_hip_pyramid_batch(h.ctx, left.data(), right.data(), W, H, 1, nlevels, &s, out.data(), cap, &count, per, nullptr);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_pyramid_batch");
    return res;
  }
  res.supports.reserve((size_t)count);
  for (int i = 0; i < count; ++i) res.supports.push_back(gpc::consensus::detail::fromC(out[(size_t)i]));
  res.perLevel.assign(per, per + nlevels);
  return res;
}

}  // namespace pyramid
}  // namespace gpc
#endif
