// gapfill_host.h -- the host-side part of the scanline hole closing (gpc_hip_gapfill_*) that needs no HIP: the parameters,
// the size limits, the aliasing rule of the output, the codes of a stored distance, the height of a band of the column scan
// and the size of the workspace.  Plain C++ so that a stand-alone program can drive it under the sanitizers
// (tests/cpp/gapfill_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "clean_host.h"

#define GF_MAX_GAP 32767
#define GF_MAX_DISCON (1 << 24)
#define GF_THREADS 256      // lanes a workgroup, all three kernels
#define GF_BAND 64          // the least rows of a band of the column scan
#define GF_NO_END 0xFFFFu   // a stored distance: no valued pixel before the border
#define GF_FAR 0xFFFEu      // a stored vertical distance: whatever the end is, it lies more than max_gap away

namespace gpc {

inline int gf_params(const gpc_gapfill* p, bool have_guide) {
  if (!p) return GPC_E_INVALID;
  if (p->max_gap < 1 || p->max_gap > GF_MAX_GAP) return GPC_E_INVALID;
  if (p->discon_q8 < 0 || p->discon_q8 > GF_MAX_DISCON) return GPC_E_INVALID;
  if (p->select < 0 || p->select > 1) return GPC_E_INVALID;
  if (p->border < 0 || p->border > 1) return GPC_E_INVALID;
  if (p->select == 1 && !have_guide) return GPC_E_INVALID;
  return GPC_OK;
}

// the limits of the densify block, as the cleaner has them: a real distance is at most 32768 and stays below GF_FAR
inline int gf_limits(int channels, int W, int H, int npairs) { return cl_limits(channels, W, H, npairs); }

// out may be the field itself; any other byte shared with the field, and any byte shared with the guide, is refused
inline bool gf_alias_ok(uintptr_t out, uintptr_t field, int64_t field_bytes, uintptr_t guide, int64_t guide_bytes) {
  if (out != field && cl_overlap(out, field_bytes, field, field_bytes)) return false;
  return !cl_overlap(out, field_bytes, guide, guide_bytes);
}

// Rows of a band of the column scan.  A band finds the state it starts in by looking back over at most max_gap rows (a
// valued pixel further away than that closes no run), so a band of at least max_gap rows reads no row more than twice.
inline int gf_band(int max_gap) { return max_gap > GF_BAND ? max_gap : GF_BAND; }
inline int gf_bands(int H, int max_gap) { return (H + gf_band(max_gap) - 1) / gf_band(max_gap); }

// workspace bytes of `npairs` pairs: the distances to the left, right, upper and lower end, a uint16 plane each
inline int64_t gf_plane_pixels(int W, int H, int npairs) { return (int64_t)W * H * npairs; }
inline int64_t gf_ws_bytes(int W, int H, int npairs) { return 4 * 2 * gf_plane_pixels(W, H, npairs); }

}  // namespace gpc
