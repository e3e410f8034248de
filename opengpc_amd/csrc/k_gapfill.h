// k_gapfill.h -- closing holes of a dense field along scanlines from the background side (gpc_hip_gapfill_*).
// include/gpc_hip.h has the rule in full; it is made of integers only.  Two directional scans and a choice:
//   k_gapfill_rows      a wave per row.  It walks the row in chunks of 64 pixels with the valued mask from __ballot: a hole's
//                       distance to the valued pixel on its left is the leading set bit of the mask below its lane, or comes
//                       from the last valued x of earlier chunks, carried in a scalar.  The distances to the right take a
//                       second walk from the other end (the row's second read comes out of the cache).
//   k_gapfill_cols      a lane per column, a workgroup per band of gf_band(max_gap) rows and 256 columns, reads coalesced
//                       across the lanes and independent of the carry.  A band finds the state it starts in by looking back
//                       over at most max_gap rows above it (below it for the walk up): a valued pixel further away than that
//                       closes no run, and the distances behind it are stored as GF_FAR.
//                       Both write uint16 planes: 0 at a valued pixel, the distance at a hole, GF_NO_END where the border
//                       comes first.  They read only channel 0 of the field.
//   k_gapfill_choose<C, SEL>  a lane per pixel, no carry at all.  It reads the four distances, decides which axis is usable
//                       and shorter, reads the two ends of that axis alone -- pixels valued on input, which no launch ever
//                       writes: this is what makes out == field safe, and with out == field a valued pixel is not written
//                       either -- and applies the rule.  The stats are counted per wave by ballot, then at most four atomics
//                       a workgroup.
#pragma once
#include "gapfill_host.h"
#include "gpc_device.h"

namespace gpc {

constexpr int32_t GF_NONE = (-2147483647 - 1);

// grid (ceil(H / 4), P), 256 lanes: four rows.  f0 of pair t is field + t * pair_stride.
__global__ __launch_bounds__(GF_THREADS) void k_gapfill_rows(const int32_t* __restrict__ field, size_t pair_stride, int W, int H,
                                                             uint16_t* __restrict__ dl, uint16_t* __restrict__ dr) {
  const int lane = threadIdx.x & 63, y = blockIdx.x * (GF_THREADS / 64) + (threadIdx.x >> 6);
  if (y >= H) return;  // (a whole wave)
  const size_t n = (size_t)W * H, at = (size_t)y * W;
  const int32_t* row = field + (size_t)blockIdx.y * pair_stride + at;
  uint16_t* pl = dl + (size_t)blockIdx.y * n + at;
  uint16_t* pr = dr + (size_t)blockIdx.y * n + at;
  int carry = -1;  // the last valued x of the chunks walked so far
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + lane;
    const bool v = x < W && row[x] != GF_NONE;
    const unsigned long long m = __ballot(v), below = m & ((1ull << lane) - 1ull);
    const int last = below ? x0 + 63 - __clzll(below) : carry;
    if (x < W) pl[x] = (uint16_t)(v ? 0u : (last >= 0 ? (uint32_t)(x - last) : GF_NO_END));
    if (m) carry = x0 + 63 - __clzll(m);
  }
  carry = -1;  // the first valued x of the chunks walked so far, from the right
  for (int x0 = ((W - 1) >> 6) << 6; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    const bool v = x < W && row[x] != GF_NONE;
    const unsigned long long m = __ballot(v), above = m & ~((2ull << lane) - 1ull);
    const int next = above ? x0 + __ffsll((long long)above) - 1 : carry;
    if (x < W) pr[x] = (uint16_t)(v ? 0u : (next >= 0 ? (uint32_t)(next - x) : GF_NO_END));
    if (m) carry = x0 + __ffsll((long long)m) - 1;
  }
}

// the state of a column walk: the row of the last valued pixel, or one of these
constexpr int GF_S_BORDER = -1;  // none up to the border
constexpr int GF_S_FAR = -2;     // none within max_gap rows: whatever lies beyond closes no run

__device__ __forceinline__ uint16_t gf_dist(bool valued, int state, int d) {
  return (uint16_t)(valued ? 0u : (state >= 0 ? (uint32_t)d : (state == GF_S_BORDER ? GF_NO_END : GF_FAR)));
}

// grid (ceil(W / 256), bands, P), 256 lanes: 256 columns of one band of `band` rows.
__global__ __launch_bounds__(GF_THREADS) void k_gapfill_cols(const int32_t* __restrict__ field, size_t pair_stride, int W, int H,
                                                             int band, int max_gap, uint16_t* __restrict__ du,
                                                             uint16_t* __restrict__ dd) {
  const int x = blockIdx.x * GF_THREADS + threadIdx.x;
  if (x >= W) return;
  const size_t n = (size_t)W * H;
  const int32_t* col = field + (size_t)blockIdx.z * pair_stride + x;
  uint16_t* pu = du + (size_t)blockIdx.z * n + x;
  uint16_t* pd = dd + (size_t)blockIdx.z * n + x;
  const int y0 = blockIdx.y * band, y1 = min(H, y0 + band);
  // down: the distance to the valued pixel above
  int state = GF_S_FAR;
  {
    int yy = y0 - 1;
    const int stop = max(0, y0 - max_gap);  // the last row looked at
    for (; yy >= stop; --yy)
      if (col[(size_t)yy * W] != GF_NONE) break;
    state = yy >= stop ? yy : (stop == 0 ? GF_S_BORDER : GF_S_FAR);
  }
#pragma unroll 4
  for (int y = y0; y < y1; ++y) {
    const bool v = col[(size_t)y * W] != GF_NONE;
    pu[(size_t)y * W] = gf_dist(v, state, y - state);
    state = v ? y : state;
  }
  // up: the distance to the valued pixel below
  {
    int yy = y1;
    const int stop = min(H - 1, y1 - 1 + max_gap);
    for (; yy <= stop; ++yy)
      if (col[(size_t)yy * W] != GF_NONE) break;
    state = yy <= stop ? yy : (stop == H - 1 ? GF_S_BORDER : GF_S_FAR);
  }
#pragma unroll 4
  for (int y = y1 - 1; y >= y0; --y) {
    const bool v = col[(size_t)y * W] != GF_NONE;
    pd[(size_t)y * W] = gf_dist(v, state, state - y);
    state = v ? y : state;
  }
}

// One axis of a hole at coordinate u of an extent of E pixels, from its two stored distances: whether it is usable, the
// length of its run and the distances to its ends.
struct GfAxis {
  bool usable, a_valued, b_valued;
  int n, da, db;
};

__device__ __forceinline__ GfAxis gf_axis(uint32_t sa, uint32_t sb, int u, int E, int max_gap, int border) {
  GfAxis r;
  r.a_valued = sa < GF_FAR, r.b_valued = sb < GF_FAR;
  // (an end stored as GF_FAR also takes the distance to the border here: da, db and n then mean nothing, and `far` below
  // makes the axis unusable whatever they are)
  r.da = r.a_valued ? (int)sa : u + 1;
  r.db = r.b_valued ? (int)sb : E - u;
  r.n = r.da + r.db - 1;
  const bool far = sa == GF_FAR || sb == GF_FAR;
  r.usable = !far && r.n <= max_gap && ((r.a_valued && r.b_valued) || ((r.a_valued || r.b_valued) && border != 0));
  return r;
}

// grid (ceil(W * H / 256), P), 256 lanes: a pixel each.  dist: the four planes, P * W * H elements each, in the order left,
// right, up, down.  copy_valued: out is not the field, so the valued pixels are written too.
template <int C, int SEL>
__global__ __launch_bounds__(GF_THREADS) void k_gapfill_choose(const int32_t* field, const uint8_t* __restrict__ guide,
                                                               const uint16_t* __restrict__ dist, size_t plane, int W, int H,
                                                               int max_gap, int discon, int border, int copy_valued,
                                                               int32_t* out, uint8_t* __restrict__ how,
                                                               int32_t* __restrict__ stats) {
  static_assert((C == 1 || C == 2) && (SEL == 0 || SEL == 1), "channels and the selector");
  __shared__ int s_stats[4];
  const int tid = threadIdx.x, p = blockIdx.y;
  const uint32_t n = (uint32_t)W * (uint32_t)H, i = blockIdx.x * (uint32_t)GF_THREADS + (uint32_t)tid;
  if (tid < 4) s_stats[tid] = 0;
  __syncthreads();
  int cat = -1;  // 0 continuous, 1 discontinuous, 2 border, 3 a hole that is left
  if (i < n) {
    const int y = (int)(i / (uint32_t)W), x = (int)(i - (uint32_t)y * (uint32_t)W);
    const int32_t* pf = field + (size_t)p * C * n;
    int32_t* po = out + (size_t)p * C * n;
    const size_t px = (size_t)p * n + i;
    const int32_t f0 = pf[i];
    if (f0 != GF_NONE) {
      if (copy_valued) {
        po[i] = f0;
        if (C == 2) po[i + n] = pf[i + n];
      }
      if (how) how[px] = 0;
    } else {
      const GfAxis h = gf_axis(dist[px], dist[plane + px], x, W, max_gap, border);
      const GfAxis v = gf_axis(dist[2 * plane + px], dist[3 * plane + px], y, H, max_gap, border);
      int32_t o0 = GF_NONE, o1 = GF_NONE;
      uint32_t code = 255u;
      cat = 3;
      if (h.usable || v.usable) {
        const bool vert = !h.usable || (v.usable && v.n < h.n);
        const GfAxis a = vert ? v : h;
        const size_t step = vert ? (size_t)W : 1;
        const size_t ia = i - (size_t)a.da * step, ib = i + (size_t)a.db * step;  // read only where the end is valued
        if (!a.a_valued || !a.b_valued) {
          const size_t ie = a.a_valued ? ia : ib;
          o0 = pf[ie];
          if (C == 2) o1 = pf[ie + n];
          cat = 2;
        } else {
          const int64_t a0 = pf[ia], b0 = pf[ib], a1 = C == 2 ? pf[ia + n] : 0, b1 = C == 2 ? pf[ib + n] : 0;
          const int64_t d0 = a0 > b0 ? a0 - b0 : b0 - a0, d1 = a1 > b1 ? a1 - b1 : b1 - a1;
          if (d0 <= discon && d1 <= discon) {
            const int64_t N = a.da + a.db;
            const int64_t s0 = a0 * a.db + b0 * a.da, s1 = a1 * a.db + b1 * a.da;
            const uint64_t q0 = (2ull * (uint64_t)(s0 < 0 ? -s0 : s0) + (uint64_t)N) / (2ull * (uint64_t)N);
            o0 = (int32_t)(s0 < 0 ? -(int64_t)q0 : (int64_t)q0);
            if (C == 2) {
              const uint64_t q1 = (2ull * (uint64_t)(s1 < 0 ? -s1 : s1) + (uint64_t)N) / (2ull * (uint64_t)N);
              o1 = (int32_t)(s1 < 0 ? -(int64_t)q1 : (int64_t)q1);
            }
            cat = 0;
          } else {
            const uint64_t ma = (uint64_t)(a0 * a0) + (uint64_t)(a1 * a1), mb = (uint64_t)(b0 * b0) + (uint64_t)(b1 * b1);
            bool take_b = mb < ma || (mb == ma && a.db < a.da);
            if (SEL == 1) {
              const uint8_t* pg = guide + (size_t)p * n;
              const int ip = pg[i], ga = abs(ip - (int)pg[ia]), gb = abs(ip - (int)pg[ib]);
              take_b = gb < ga || (gb == ga && take_b);
            }
            o0 = (int32_t)(take_b ? b0 : a0);
            o1 = (int32_t)(take_b ? b1 : a1);
            cat = 1;
          }
        }
        code = (uint32_t)(cat + 1 + (vert ? 3 : 0));
      }
      po[i] = o0;
      if (C == 2) po[i + n] = o1;
      if (how) how[px] = (uint8_t)code;
    }
  }
  if (stats) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long m = __ballot(cat == k);
      if ((tid & 63) == 0 && m) atomicAdd(&s_stats[k], __popcll(m));
    }
    __syncthreads();
    if (tid < 4 && s_stats[tid]) atomicAdd(stats + (size_t)p * 4 + tid, s_stats[tid]);
  }
}

}  // namespace gpc
