// field_score_host.h -- the host-side part of the dense field scorer (gpc_hip_score_fields*) that needs no HIP: the
// parameter and size checks, the squared parameters the kernel compares against, the word layout of gpc_field_score and
// the geometry of the launch.  Plain C++ so that a stand-alone program can drive it under the sanitizers
// (tests/cpp/field_score_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "clean_host.h"

#define FS_THREADS 256                        // lanes per workgroup
#define FS_PX 4                               // pixels per lane and slot: one 16-byte load per int32 / float plane
#define FS_UNROLL 2                           // slots per lane and chunk
#define FS_SLOTS (FS_THREADS * FS_UNROLL)     // slots per chunk: 2048 pixels
#define FS_MAX_GROUPS 2048                    // workgroups of a launch at most: 8 per CU
#define FS_FLUSH_CHUNKS 8000                  // a lane's packed 16-bit counts hold 4 * FS_UNROLL * this < 65536 pixels
#define FS_WORDS 64                           // 64-bit words of gpc_field_score
#define FS_TALLY_WORDS 12                     // of gpc_field_tally: n_judged, n_within[8], n_outlier, sum_e_q8, sum_e2_q16
#define FS_WORD_ALL 4                         // n_pixels, n_ignored, n_no_truth, n_hole, then `all`, then the bins
#define FS_WORD_BIN (FS_WORD_ALL + FS_TALLY_WORDS)
#define FS_TRUTH_MAX 32768.f                  // a truth value beyond it is no truth
#define FS_AXIS_MAX 65536                     // the per-axis clamp, 256 pixels
#define FS_E2_MAX (1ull << 32)                // the clamp of the squared error

namespace gpc {

static_assert(sizeof(gpc_field_score_prm) == 64 && sizeof(gpc_field_tally) == 8 * FS_TALLY_WORDS &&
                  sizeof(gpc_field_score) == 8 * FS_WORDS && FS_WORD_BIN + 4 * FS_TALLY_WORDS == FS_WORDS,
              "the structs of the field scorer as the kernel's words");
static_assert(4 * FS_UNROLL * FS_FLUSH_CHUNKS < 65536, "a packed 16-bit count cannot overflow between two flushes");

// what the kernel compares against: the squares, as a kernel argument
struct FsPrm {
  unsigned long long sp2[3];   // speed_q8[k]^2 <= 2^46
  uint32_t thr2[8];            // thr_q8[k]^2 <= 65535^2 < 2^32 - 1
  uint32_t abs2;               // out_abs_q8^2, likewise
  uint32_t rel2;               // out_rel_pm^2
  int32_t n_thr, n_speed;
};

inline int fs_params(const gpc_field_score_prm* p) {
  if (!p) return GPC_E_INVALID;
  if (p->n_thr < 0 || p->n_thr > 8 || p->n_speed < 0 || p->n_speed > 3 || p->reserved != 0) return GPC_E_INVALID;
  for (int k = 0; k < p->n_thr; ++k)
    if (p->thr_q8[k] < 0 || p->thr_q8[k] > 65535) return GPC_E_INVALID;
  if (p->out_abs_q8 < 0 || p->out_abs_q8 > 65535 || p->out_rel_pm < 0 || p->out_rel_pm > 255) return GPC_E_INVALID;
  for (int k = 0; k < p->n_speed; ++k) {
    if (p->speed_q8[k] < 0 || p->speed_q8[k] > (1 << 23)) return GPC_E_INVALID;
    if (k && p->speed_q8[k] < p->speed_q8[k - 1]) return GPC_E_INVALID;
  }
  return GPC_OK;
}

inline FsPrm fs_squares(const gpc_field_score_prm& p) {
  FsPrm q = {};
  for (int k = 0; k < p.n_thr; ++k) q.thr2[k] = (uint32_t)p.thr_q8[k] * (uint32_t)p.thr_q8[k];
  for (int k = 0; k < p.n_speed; ++k) q.sp2[k] = (unsigned long long)p.speed_q8[k] * (unsigned long long)p.speed_q8[k];
  q.abs2 = (uint32_t)p.out_abs_q8 * (uint32_t)p.out_abs_q8;
  q.rel2 = (uint32_t)(p.out_rel_pm * p.out_rel_pm);
  q.n_thr = p.n_thr, q.n_speed = p.n_speed;
  return q;
}

// the limits of the densify block, as the cleaner has them
inline int fs_limits(int channels, int W, int H, int npairs) { return cl_limits(channels, W, H, npairs); }

// v must be absent for a disparity and present for a flow
inline int fs_truth(const gpc_truth* t, int channels) {
  if (!t || !t->u) return GPC_E_INVALID;
  if (channels == 2 ? !t->v : t->v != nullptr) return GPC_E_INVALID;
  return GPC_OK;
}

// chunks of one pair: its slots start up to 3 pixels before the plane, at the 16-byte boundary below it
inline int64_t fs_chunks(int W, int H) { return (((int64_t)W * H + 3 + FS_PX - 1) / FS_PX + FS_SLOTS - 1) / FS_SLOTS; }
inline int64_t fs_groups(int W, int H, int npairs) {
  const int64_t items = fs_chunks(W, H) * npairs;
  return items < FS_MAX_GROUPS ? items : FS_MAX_GROUPS;
}

// the exact floor of the square root of x <= 2^32 (the host's statement of what the kernel does with a float estimate)
inline uint32_t fs_isqrt(uint64_t x) {
  uint64_t r = 0;
  for (uint64_t bit = 1ull << 16; bit; bit >>= 1)
    if ((r + bit) * (r + bit) <= x) r += bit;
  return (uint32_t)r;
}

}  // namespace gpc
