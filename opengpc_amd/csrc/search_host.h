// search_host.h -- the host-side checks of the local dense search (gpc_hip_search_*) that need no HIP: the parameters, the
// size limits, the aliasing rule of the output against the field and the images, the rounding of a field value to its
// whole-pixel shift and the tile geometry.  Plain C++ so that a stand-alone program can drive it under the sanitizers
// (tests/cpp/search_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "clean_host.h"

#define SR_TILE_W 32     // pixels per tile row: one lane each, a wave holds two rows
#define SR_TILE_H 8      // rows per tile: 256 lanes a workgroup
#define SR_MAX_RADIUS 4  // a window row is at most 9 bytes
#define SR_MAX_RANGE 2   // 9 + 2 * (2 + 1) = 15 bytes: a target row with all its shifts is one 16-byte load

namespace gpc {

inline int sr_params(const gpc_search* p) {
  if (!p) return GPC_E_INVALID;
  if (p->radius < 1 || p->radius > SR_MAX_RADIUS) return GPC_E_INVALID;
  if (p->range < 0 || p->range > SR_MAX_RANGE) return GPC_E_INVALID;
  if (p->subpixel < 0 || p->subpixel > 1) return GPC_E_INVALID;
  if (p->max_cost < 0 || p->max_cost > 0xFFFF) return GPC_E_INVALID;
  return GPC_OK;
}

// the limits of the densify block, as the cleaner has them
inline int sr_limits(int channels, int W, int H, int npairs) { return cl_limits(channels, W, H, npairs); }

// out may be the field itself; any other byte shared with the field, and any byte shared with an image, is refused
inline bool sr_alias_ok(uintptr_t out, uintptr_t field, int64_t field_bytes, uintptr_t imgL, uintptr_t imgR, int64_t img_bytes) {
  if (out != field && cl_overlap(out, field_bytes, field, field_bytes)) return false;
  return !cl_overlap(out, field_bytes, imgL, img_bytes) && !cl_overlap(out, field_bytes, imgR, img_bytes);
}

// sgn(F) * ((|F| + 128) >> 8), the cleaner's rounding; |F| + 128 is taken in 64 bits, so INT32_MAX and INT32_MIN + 1 are
// values like any other (|result| <= 2^23)
inline int32_t sr_round(int32_t f) {
  const int64_t a = f < 0 ? -(int64_t)f : (int64_t)f;
  const int32_t r = (int32_t)((a + 128) >> 8);
  return f < 0 ? -r : r;
}

inline int sr_tiles_x(int W) { return (W + SR_TILE_W - 1) / SR_TILE_W; }
inline int sr_tiles_y(int H) { return (H + SR_TILE_H - 1) / SR_TILE_H; }

}  // namespace gpc
