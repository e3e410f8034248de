// dense_host.h -- the host-side checks of the densifier (gpc_hip_densify_*) that need no HIP: the parameters, the size
// limits, Lmax, the geometry of the cell pyramid and the sizes of the workspaces.  Plain C++ so that a stand-alone program
// can drive it under the sanitizers (tests/cpp/dense_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"

#define DN_MAX_LEVEL 15  // a side of at most 32768 pixels has one cell at level 15

namespace gpc {

// the grids of levels 1 .. top of one pair, back to back: what the kernels index by (made on the host, passed by value)
struct DnGeom {
  int32_t W, H;
  int32_t top;                    // min(max_level, Lmax): the last level a pixel may take its value from
  int32_t min_count, spread;
  int32_t gw[DN_MAX_LEVEL + 1];   // columns of level l (entry 0 unused)
  int32_t gh[DN_MAX_LEVEL + 1];   // rows
  int32_t off[DN_MAX_LEVEL + 2];  // first cell of level l in a pair's pyramid; off[top + 1] = cells per pair
};

inline int dn_params(const gpc_densify* p, bool have_ref) {
  if (!p) return GPC_E_INVALID;
  if (p->max_level < 1 || p->max_level > DN_MAX_LEVEL || p->min_count < 1 || p->min_count > 65536) return GPC_E_INVALID;
  if ((p->spread != 0 && p->spread != 1) || p->max_cost < 0 || p->max_cost > 0xFFFF) return GPC_E_INVALID;
  if (p->max_cost < 0xFFFF && !have_ref) return GPC_E_INVALID;
  return GPC_OK;
}

// |value| < 2^24 and a pair has at most 2^30 pixels, so every sum stays below 2^54 (a 3x3 neighbourhood below 2^58); a
// launch has one grid layer per pair, and a record's number in the whole call fits an int
inline int dn_limits(int W, int H, int npairs, int64_t cap) {
  if (W < 1 || H < 1 || npairs < 1 || cap < 1) return GPC_E_INVALID;
  if (W > 32768 || H > 32768 || (int64_t)W * H > ((int64_t)1 << 30)) return GPC_E_UNSUPPORTED;
  if (npairs > 65535 || (int64_t)npairs * cap > 0x7FFFFFFFll) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// the first level l >= 1 whose grid is one cell
inline int dn_lmax(int W, int H) {
  int l = 1;
  while (((W - 1) >> l) != 0 || ((H - 1) >> l) != 0) ++l;
  return l;
}

// W, H within dn_limits, prm within dn_params
inline DnGeom dn_geom(int W, int H, const gpc_densify& prm) {
  DnGeom g = {};
  g.W = W, g.H = H;
  const int lmax = dn_lmax(W, H);
  g.top = prm.max_level < lmax ? prm.max_level : lmax;
  g.min_count = prm.min_count, g.spread = prm.spread;
  int32_t at = 0;
  for (int l = 1; l <= g.top; ++l) {
    g.gw[l] = ((W - 1) >> l) + 1, g.gh[l] = ((H - 1) >> l) + 1;
    g.off[l] = at;
    at += g.gw[l] * g.gh[l];  // (level 1 has at most 2^28 cells, every level at most half the one below: the sum fits)
  }
  g.off[g.top + 1] = at;
  return g;
}

inline int64_t dn_cells(const DnGeom& g) { return g.off[g.top + 1]; }

// workspace bytes of `npairs` pairs: the owner plane, the cells' counts, the cells' sums (channels = 1 or 2)
inline int64_t dn_owner_bytes(int W, int H, int npairs) { return (int64_t)4 * W * H * npairs; }
inline int64_t dn_count_bytes(const DnGeom& g, int npairs) { return (int64_t)4 * dn_cells(g) * npairs; }
inline int64_t dn_sum_bytes(const DnGeom& g, int npairs, int channels) { return (int64_t)8 * channels * dn_cells(g) * npairs; }

}  // namespace gpc
