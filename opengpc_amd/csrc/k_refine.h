// k_refine.h -- sub-pixel refinement and photometric cost of matches (gpc_hip_refine_*).  include/gpc_hip.h has the rule in
// full; it is made of integers only.  A record's cost is the sum of absolute differences between the (2r+1)^2 window around
// its source in the left image and the window around its target in the right one; the costs at the target shifted by one
// pixel either way give a parabola per axis, whose minimum is the sub-pixel shift in 1/256 pixel.
//   k_refine<CORR, R>   one lane per record.  A window row is ONE buffer load per side: the 2R+1 source bytes from x - R,
//                       the 2R+3 target bytes from tx - R - 1, whatever their alignment.  The image of the pair is the
//                       buffer (base, size W * H), so a load never leaves it; one that would reach past its end comes back
//                       as zeros and is made again byte by byte (rf_load_row).  v_qsad_pk_u16_u8 gives the sums of a
//                       4-byte chunk of the source row against the target row at byte shifts 0 .. 3 in one instruction:
//                       shifts 0, 1, 2 are the three x positions.  The row's last 1 or 3 bytes (2R+1 is odd) go through
//                       v_sad_u8 on words masked to those bytes -- masked AFTER the shift, so no byte the rule does not
//                       name reaches a sum, and a pixel that is 0 counts like any other.  A correspondence runs the same
//                       row step for the targets one row up and down (only their middle shift is used; the compiler drops
//                       the rest).  Everything is unrolled over R: the loads of a record are all in flight before the
//                       first sum needs one.
#pragma once
#include "gpc_device.h"
#include "k_consensus.h"  // ConsRec, cs_count

#define RF_THREADS 256
#define RF_MAX_RADIUS 6
#define RF_NOT_EVALUATED 0x0000FFFFu  // cost 0xFFFF, flags 0: the second word of the result of a record that is not evaluated

namespace gpc {

typedef uint32_t rf_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t rf_u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t rf_u32x4 __attribute__((ext_vector_type(4)));

// NB bytes of the image from byte `off` on, in v[0 .. (NB + 3) / 4) (the rest 0).  The bytes asked for lie inside the image
// (the caller has checked the window); the dwords that hold them may reach past its end, by 3 bytes at the most.
template <int NB>
__device__ __forceinline__ void rf_load_row(const __amdgpu_buffer_rsrc_t img, uint32_t n, uint32_t off, uint32_t (&v)[4]) {
  constexpr int ND = (NB + 3) / 4;
  v[0] = v[1] = v[2] = v[3] = 0u;
  if constexpr (ND == 1) {
    v[0] = __builtin_amdgcn_raw_buffer_load_b32(img, off, 0, 0);
  } else if constexpr (ND == 2) {
    const rf_u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y;
  } else if constexpr (ND == 3) {
    const rf_u32x3 q = __builtin_amdgcn_raw_buffer_load_b96(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z;
  } else {
    const rf_u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  if (off + 4u * ND > n) {  // (off < n <= 2^30.)  The load was refused as a whole: the last window of the image, few lanes
    v[0] = v[1] = v[2] = v[3] = 0u;
#pragma unroll
    for (int i = 0; i < NB; ++i) v[i / 4] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(img, off + (uint32_t)i, 0, 0) << (8 * (i % 4));
  }
}

// One window row: l = the source row from x - R, t = the target row from tx - R - 1.  q's 16-bit fields 0, 1, 2 gather the
// full chunks' sums at the x shifts -1, 0, +1 (field 3 is not read), tl[0 .. 2] the tail's.
template <int R>
__device__ __forceinline__ void rf_row(const uint32_t (&l)[4], const uint32_t (&t)[4], uint64_t& q, uint32_t (&tl)[3]) {
  constexpr int C = (2 * R + 1) / 4, TAIL = (2 * R + 1) % 4;  // TAIL is 1 or 3
  constexpr uint32_t TM = TAIL == 1 ? 0xFFu : 0xFFFFFFu;
#pragma unroll
  for (int c = 0; c < C; ++c)
    q = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)t[c + 1] << 32) | t[c], l[c], q);
  const uint32_t lt = l[C] & TM, lo = t[C], hi = C + 1 < 4 ? t[(C + 1) & 3] : 0u;  // (R = 6: the tail byte and its shifts lie in t[3])
  tl[0] = __builtin_amdgcn_sad_u8(lo & TM, lt, tl[0]);
  tl[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 1) & TM, lt, tl[1]);
  tl[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 2) & TM, lt, tl[2]);
}

__device__ __forceinline__ uint32_t rf_cost(uint64_t q, const uint32_t (&tl)[3], int s) {
  return ((uint32_t)(q >> (16 * s)) & 0xFFFFu) + tl[s];
}

// The parabola through the costs at the target's shifts -1, 0, +1: true iff the axis has a minimum; q8 = the target's
// sub-pixel shift in 1/256 pixel, sgn(n) * ((256 |n| + a) div 2a), |q8| <= 128.  The quotient is the compiler's exact
// unsigned division: one or two per record, beside some hundred instructions of loads and sums.
__device__ __forceinline__ bool rf_axis(uint32_t cm, uint32_t c0, uint32_t cp, int& q8) {
  const int a = (int)(cm + cp) - 2 * (int)c0, n = (int)cm - (int)cp;
  q8 = 0;
  if (!(c0 <= cm && c0 <= cp && a > 0)) return false;
  const uint32_t an = (uint32_t)(n < 0 ? -n : n);
  const int q = (int)((256u * an + (uint32_t)a) / (2u * (uint32_t)a));
  q8 = n < 0 ? -q : q;
  return true;
}

// source (x, y) and target (tx, ty) of a record; false: it is not evaluated (a window, the target's with its shifts,
// leaves the image, or a support's d is no whole number below 2^24)
template <int R>
__device__ __forceinline__ bool rf_ends(const ConsRec<true>& r, int W, int H, int& x, int& y, int& tx, int& ty) {
  x = r.sx, y = r.sy, tx = r.tx, ty = r.ty;
  return x >= R && x <= W - 1 - R && y >= R && y <= H - 1 - R && tx >= R + 1 && tx <= W - 2 - R && ty >= R + 1 && ty <= H - 2 - R;
}
template <int R>
__device__ __forceinline__ bool rf_ends(const ConsRec<false>& r, int W, int H, int& x, int& y, int& tx, int& ty) {
  x = r.x, y = ty = r.y;
  const float d = r.d;
  const bool whole = d == truncf(d) && fabsf(d) < 16777216.f;
  const bool src = x >= R && x <= W - 1 - R && y >= R && y <= H - 1 - R;
  tx = (whole && src) ? x - (int)d : -1;  // (|x| < 2^30 and |d| < 2^24 here: no overflow)
  return whole && src && tx >= R + 1 && tx <= W - 2 - R;
}

// grid (x, P): ref[t][i] for the records i < m_t of pair t; out[t][i] (supports, optional) the record with the refined d.
// n = W * H: the images of pair t are imgL + t * n and imgR + t * n (a sequence passes its frames and its frames + n).
template <bool CORR, int R>
__global__ __launch_bounds__(RF_THREADS) void k_refine(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                       const int32_t* __restrict__ counts, const uint8_t* __restrict__ imgL,
                                                       const uint8_t* __restrict__ imgR, int W, int H,
                                                       uint2* __restrict__ ref, ConsRec<false>* __restrict__ out) {
  static_assert(R >= 1 && R <= RF_MAX_RADIUS, "a row of 2R+3 bytes fits one 16-byte load");
  constexpr int NL = 2 * R + 1, NT = 2 * R + 3;
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const uint32_t n = (uint32_t)W * (uint32_t)H;
  const ConsRec<CORR>* rp = rec + (long)t * cap;
  uint2* fp = ref + (long)t * cap;
  const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(imgL + (size_t)t * n), 0, (int)n, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(imgR + (size_t)t * n), 0, (int)n, 0x00020000);
  for (int i = blockIdx.x * RF_THREADS + threadIdx.x; i < m; i += gridDim.x * RF_THREADS) {
    const ConsRec<CORR> r = rp[i];
    int x, y, tx, ty;
    uint2 res = make_uint2(0u, RF_NOT_EVALUATED);
    int dx = 0;
    if (rf_ends<R>(r, W, H, x, y, tx, ty)) {
      const uint32_t offL = (uint32_t)(y - R) * (uint32_t)W + (uint32_t)(x - R);
      const uint32_t offT = (uint32_t)(ty - R) * (uint32_t)W + (uint32_t)(tx - R - 1);
      uint64_t q0 = 0, qu = 0, qd = 0;
      uint32_t t0[3] = {0u, 0u, 0u}, tu[3] = {0u, 0u, 0u}, td[3] = {0u, 0u, 0u};
      if (!CORR) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          uint32_t l[4], g[4];
          rf_load_row<NL>(rsL, n, offL + (uint32_t)j * (uint32_t)W, l);
          rf_load_row<NT>(rsT, n, offT + (uint32_t)j * (uint32_t)W, g);
          rf_row<R>(l, g, q0, t0);
        }
      } else {
        uint32_t l[NL][4];
#pragma unroll
        for (int j = 0; j < NL; ++j) rf_load_row<NL>(rsL, n, offL + (uint32_t)j * (uint32_t)W, l[j]);
        // target row k = -1 .. NL of the window at (tx, ty): source row k against it is the shift 0 in y, source row k + 1
        // the target one row up, source row k - 1 the target one row down
#pragma unroll
        for (int k = -1; k <= NL; ++k) {
          uint32_t g[4];
          rf_load_row<NT>(rsT, n, offT + (uint32_t)(k * W), g);  // (k = -1: ty - R - 1 >= 0, the sum does not wrap below 0)
          if (k >= 0 && k < NL) rf_row<R>(l[k], g, q0, t0);
          if (k + 1 < NL) rf_row<R>(l[k + 1], g, qu, tu);
          if (k - 1 >= 0) rf_row<R>(l[k - 1], g, qd, td);
        }
      }
      const uint32_t c0 = rf_cost(q0, t0, 1);
      int dy = 0;
      uint32_t flags = 1u;
      if (rf_axis(rf_cost(q0, t0, 0), c0, rf_cost(q0, t0, 2), dx)) flags |= 2u;
      if (CORR && rf_axis(rf_cost(qu, tu, 1), c0, rf_cost(qd, td, 1), dy)) flags |= 4u;
      res.x = ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16);
      res.y = c0 | (flags << 16);
    }
    fp[i] = res;
    if constexpr (!CORR) {
      if (out) {
        ConsRec<false> o = r;
        // (dx = 0 leaves d as it is, bit for bit: d - 0 for a whole d, and the d of a record that is not evaluated)
        if (dx != 0) o.d = __fsub_rn(o.d, __fmul_rn((float)dx, 0.00390625f));
        (out + (long)t * cap)[i] = o;
      }
    }
  }
}

}  // namespace gpc
