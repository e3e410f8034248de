// clean_host.h -- the host-side checks of the field cleaner (gpc_hip_clean_*) that need no HIP: the parameters, the size
// limits, the overlap test of the output against the inputs, the tile geometry and the sizes of the workspaces.  Plain C++
// so that a stand-alone program can drive it under the sanitizers (tests/cpp/clean_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"

#define CL_TILE 32  // pixels per tile edge of the labelling and of the median

namespace gpc {

inline int cl_params(const gpc_clean* p, bool have_bwd) {
  if (!p) return GPC_E_INVALID;
  if (p->check_tol_q8 < -1 || p->check_tol_q8 > (1 << 24)) return GPC_E_INVALID;
  if (p->speckle_diff_q8 < 0 || p->speckle_diff_q8 > (1 << 24)) return GPC_E_INVALID;
  if (p->speckle_min < 0 || p->speckle_min > (1 << 30)) return GPC_E_INVALID;
  if (p->median_radius < 0 || p->median_radius > 2) return GPC_E_INVALID;
  if (p->check_tol_q8 >= 0 && !have_bwd) return GPC_E_INVALID;
  return GPC_OK;
}

// the limits of the densify block: a launch has one grid layer per pair, a pixel's index fits 30 bits
inline int cl_limits(int channels, int W, int H, int npairs) {
  if ((channels != 1 && channels != 2) || W < 1 || H < 1 || npairs < 1) return GPC_E_INVALID;
  if (W > 32768 || H > 32768 || (int64_t)W * H > ((int64_t)1 << 30)) return GPC_E_UNSUPPORTED;
  if (npairs > 65535) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

inline int64_t cl_field_bytes(int channels, int W, int H, int npairs) { return (int64_t)4 * channels * W * H * npairs; }

// do [a, a + na) and [b, b + nb) share a byte (addresses as integers: the arrays may be device memory)
inline bool cl_overlap(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  return a < b + (uintptr_t)nb && b < a + (uintptr_t)na;
}

inline int cl_tiles(int n) { return (n + CL_TILE - 1) / CL_TILE; }

// pixels on the inner tile edges of one pair: a lane of the border kernel each.  First the (tiles_x - 1) * H pixels left
// of which a tile ends, then the (tiles_y - 1) * W pixels above which one ends.
inline int64_t cl_border_pixels(int W, int H) { return (int64_t)(cl_tiles(W) - 1) * H + (int64_t)(cl_tiles(H) - 1) * W; }

// workspace bytes of `npairs` pairs: the label plane, the sizes of the components (kept at their roots)
inline int64_t cl_label_bytes(int W, int H, int npairs) { return (int64_t)4 * W * H * npairs; }
inline int64_t cl_size_bytes(int W, int H, int npairs) { return (int64_t)4 * W * H * npairs; }

// is the labelling needed at all
inline bool cl_labels_needed(const gpc_clean& p, bool want_label) { return want_label || p.speckle_min > 1; }

}  // namespace gpc
