// inpaint_host.h -- the host-side checks of the field completion (gpc_hip_inpaint_*) that need no HIP: the parameters, the
// size limits, the aliasing rule of the output against the field (the same pointer or no shared byte), the tile geometry and
// the layout of the control workspace.  Plain C++ so that a stand-alone program can drive it under the sanitizers
// (tests/cpp/inpaint_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "clean_host.h"

#define IP_TILE 32         // pixels per tile edge, as the fill and the cleaner
#define IP_MAX_RADIUS 8    // the staged tile is at most (32 + 16)^2 pixels
#define IP_MAX_PASSES 254  // pass numbers are bytes: 0 = valued on input, 255 = still a hole

namespace gpc {

inline int ip_params(const gpc_inpaint* p) {
  if (!p) return GPC_E_INVALID;
  if (p->radius < 1 || p->radius > IP_MAX_RADIUS) return GPC_E_INVALID;
  if (p->range_shift < 0 || p->range_shift > 8) return GPC_E_INVALID;
  if (p->min_weight < 1 || p->min_weight > (1 << 24)) return GPC_E_INVALID;
  if (p->passes < 1 || p->passes > IP_MAX_PASSES) return GPC_E_INVALID;
  return GPC_OK;
}

// the limits of the densify block, as the cleaner has them
inline int ip_limits(int channels, int W, int H, int npairs) { return cl_limits(channels, W, H, npairs); }

// out may be the field itself; any other shared byte is refused
inline bool ip_alias_ok(uintptr_t out, uintptr_t field, int64_t bytes) { return out == field || !cl_overlap(out, bytes, field, bytes); }

// the weight of a neighbour whose guide differs by `diff` grey levels (0 .. 255): 1 .. 256, never 0
inline int32_t ip_weight(int diff, int range_shift) {
  const int s = diff >> range_shift;
  return 256 >> (s < 8 ? s : 8);
}

// sgn(S) * ((2 |S| + Wt) div (2 Wt)): the weighted mean, rounded half away from zero.  |S| < 2^49 and 1 <= Wt < 2^18.
inline int32_t ip_mean(int64_t S, int64_t Wt) {
  const uint64_t a = S < 0 ? (uint64_t)0 - (uint64_t)S : (uint64_t)S, q = (2 * a + (uint64_t)Wt) / (2 * (uint64_t)Wt);
  return (int32_t)(S < 0 ? -(int64_t)q : (int64_t)q);
}

inline int ip_tiles(int n) { return (n + IP_TILE - 1) / IP_TILE; }

// The control workspace, int32 words: [0, 256) the pixels filled by pass k at word k (word 0 unused), then 2 words of stats
// per pair (used where the caller passes no d_stats), then one hole count per tile and pair.  The first two parts are
// cleared per call; the tile counts are written whole by the first launch.
inline int64_t ip_ctl_stats_at() { return 256; }
inline int64_t ip_ctl_tiles_at(int npairs) { return 256 + (int64_t)2 * npairs; }
inline int64_t ip_ctl_bytes(int W, int H, int npairs) {
  return 4 * (ip_ctl_tiles_at(npairs) + (int64_t)ip_tiles(W) * ip_tiles(H) * npairs);
}
inline int64_t ip_pass_bytes(int W, int H, int npairs) { return (int64_t)W * H * npairs; }

}  // namespace gpc
