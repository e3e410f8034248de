// pyramid_host.h -- the host-side checks of the pyramid matcher (gpc_hip_pyramid_*) that need no HIP: the geometry of the
// levels, the settings of a level, the capacity that holds every record of a level, the arguments of the downsampling step.
// Plain C++ so that a stand-alone program can drive it under the sanitizers (tests/cpp/pyramid_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"

namespace gpc {

// what the library takes as an image (check_dims of gpc_hip.hip: the margin of 13 on every side, a row within one
// workgroup's join table, a pixel index within 30 bits)
inline int pyr_image_ok(int W, int H) {
  if (W <= 0 || H <= 0 || (W % 16) != 0) return GPC_E_INVALID;
  if (W < 2 * GPC_PATCH_RADIUS + 16 || H < 2 * GPC_PATCH_RADIUS + 4) return GPC_E_INVALID;
  if (W > 16384 || (int64_t)W * H > ((int64_t)1 << 30)) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// W_l = W >> l, H_l = H_{l-1} / 2; every level an image the library takes.  widths / heights (optional): `levels` entries.
inline int pyr_levels(int W, int H, int levels, int32_t* widths, int32_t* heights) {
  if (levels < 1 || levels > GPC_MAX_PYRAMID_LEVELS) return GPC_E_INVALID;
  int w = W, h = H;
  for (int l = 0; l < levels; ++l) {
    if (l) {
      if (w & 1) return GPC_E_INVALID;
      w >>= 1;
      h /= 2;
    }
    const int st = pyr_image_ok(w, h);
    if (st != GPC_OK) return st;
  }
  w = W, h = H;
  for (int l = 0; l < levels; ++l) {
    if (l) w >>= 1, h /= 2;
    if (widths) widths[l] = w;
    if (heights) heights[l] = h;
  }
  return GPC_OK;
}

// disp_high and vertical_tolerance shifted right by l, the rest unchanged: a mapped record stays within the caller's bounds
inline gpc_settings pyr_level_settings(const gpc_settings& s, int l) {
  gpc_settings t = s;
  t.disp_high = s.disp_high >> l;
  t.vertical_tolerance = s.vertical_tolerance >> l;
  return t;
}

// every record a pair of W x H can have: one per inner pixel, and one more
inline int64_t pyr_level_cap(int W, int H) {
  return (int64_t)(W - 2 * GPC_PATCH_RADIUS) * (H - 2 * GPC_PATCH_RADIUS) + 1;
}

// one downsampling step over nimages images of W x H: a lane reads 8 bytes of a row and writes 4, a launch has one grid
// layer per image
inline int pyr_down_check(const void* src, const void* dst, int W, int H, int nimages) {
  if (!src || !dst || W <= 0 || H < 2 || nimages < 1 || (W % 32) != 0) return GPC_E_INVALID;
  if (((uintptr_t)src & 7u) || ((uintptr_t)dst & 3u)) return GPC_E_INVALID;
  if (nimages > 65535 || (H / 2 + 3) / 4 > 65535) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// the merge of `levels` record lists per pair over level 0's W x H: the plane has a bit per pixel, a launch one grid row per
// pair; caps[l] >= 1
inline int pyr_merge_check(int W, int H, int npairs, int levels, const int32_t* caps, int cap_out) {
  if (W <= 0 || H <= 0 || npairs < 1 || levels < 1 || levels > GPC_MAX_PYRAMID_LEVELS || !caps || cap_out < 1) return GPC_E_INVALID;
  for (int l = 0; l < levels; ++l)
    if (caps[l] < 1) return GPC_E_INVALID;
  if (npairs > 65535 || (int64_t)W * H > ((int64_t)1 << 30)) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

}  // namespace gpc
