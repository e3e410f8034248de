// k_dense.h -- dense disparity maps and flow fields from sparse matches (gpc_hip_densify_*): a hierarchical fill.
// include/gpc_hip.h has the rule in full; it is made of integers only.  A pixel that is the source of a participating
// record keeps that record's value (the lowest input index where several meet); every other pixel takes the mean of the
// values in the smallest aligned block around it (its own level-l cell, or the 3x3 cells around that) that holds min_count
// of them.  Values are Q8 (1/256 pixel), one channel for supports, two for correspondences.
//   k_dense_claim   one lane per record: does it participate; atomicMin of its input index into the owner plane (4 bytes
//                   per pixel, 0xFFFFFFFF = nobody: the host clears it with a memset);
//   k_dense_pull    one workgroup per 32x32 pixel tile: reads the tile's owners, gathers their records' values, writes
//                   value rows (GPC_DENSE_NONE where nobody owns the pixel), and reduces the tile's levels 1 .. 5 in LDS --
//                   count and exact 64-bit sum per cell -- into the pair's cell pyramid in global memory;
//   k_dense_top     one workgroup per pair: the levels above the tile, 6 .. top, each from the one below.  A level is read
//                   by other waves than wrote it, inside one launch: the cells are written and read at agent scope, with a
//                   fence and a barrier between two levels;
//   k_dense_push    one workgroup per tile.  Every pixel without an owner inside one level-1 cell takes the same value (the
//                   cell fixes all its ancestors), so one lane per level-1 cell walks upward -- counts of its cell or 3x3
//                   cells per level, sums and one division at the level that qualifies -- and leaves the answer in LDS; then
//                   the tile's rows are read (the values k_dense_pull wrote), filled where they are none, and written with
//                   their levels, 32 consecutive pixels per half wave.
// The division: 2 |sum| + N fits 32 bits for all but the largest blocks (N <= 36 at level 1), where it is one v_rcp-based
// 32-bit quotient; the exact 64-bit one is taken only where it does not.
#pragma once
#include "dense_host.h"
#include "gpc_device.h"
#include "k_consensus.h"  // ConsRec, cs_count, cs_ends

#define DN_THREADS 256
#define DN_TILE 32                  // pixels per tile edge: level 5 is one cell of it
#define DN_TILE_LEVELS 5
#define DN_NOBODY 0xFFFFFFFFu       // owner plane: no participating record has this pixel as its source
#define DN_NONE ((int32_t)0x80000000)  // GPC_DENSE_NONE
#define DN_LDS_CELLS 341            // 256 + 64 + 16 + 4 + 1 cells of a tile's levels 1 .. 5

namespace gpc {

// does record i take part under the cost ceiling (ref may be null; flags bit 0 = evaluated)
__device__ __forceinline__ bool dn_admitted(const uint2* __restrict__ ref, long at, int max_cost) {
  if (!ref || max_cost >= 0xFFFF) return true;
  const uint32_t w = ref[at].y;
  return ((w >> 16) & 1u) != 0u && (int)(w & 0xFFFFu) <= max_cost;
}

// the sub-pixel shift of record `at`: 0 without ref or when the record was not evaluated
__device__ __forceinline__ void dn_shift(const uint2* __restrict__ ref, long at, int& dx, int& dy) {
  dx = dy = 0;
  if (!ref) return;
  const uint2 f = ref[at];
  if (!((f.y >> 16) & 1u)) return;
  dx = (int)(int16_t)(f.x & 0xFFFFu), dy = (int)(int16_t)(f.x >> 16);
}

// the value of a record that participates (its ends lie in the image: every term stays below 2^24)
__device__ __forceinline__ void dn_value(const ConsRec<false>& r, int dx, int, int32_t (&v)[1]) { v[0] = 256 * (int)r.d - dx; }
__device__ __forceinline__ void dn_value(const ConsRec<true>& r, int dx, int dy, int32_t (&v)[2]) {
  v[0] = 256 * (r.tx - r.sx) + dx, v[1] = 256 * (r.ty - r.sy) + dy;
}

// sgn(s) * ((2 |s| + n) div (2 n)), n >= 1: the mean rounded half away from zero.  n <= 2^30 (the cells of a sum are
// disjoint blocks of one image), |s| < 2^54.
__device__ __forceinline__ int32_t dn_mean(int64_t s, int32_t n) {
  const uint64_t a = (uint64_t)(s < 0 ? -s : s), num = 2u * a + (uint32_t)n;
  const uint32_t den = 2u * (uint32_t)n;
  const uint32_t q = (num >> 32) == 0 ? (uint32_t)num / den : (uint32_t)(num / den);
  return s < 0 ? -(int32_t)q : (int32_t)q;
}

// grid (x, P): owner[t][sy * W + sx] = min(.., i) over the participating records i < m_t of pair t
template <bool CORR>
__global__ __launch_bounds__(DN_THREADS) void k_dense_claim(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                            const int32_t* __restrict__ counts, const uint2* __restrict__ ref,
                                                            int max_cost, int W, int H, uint32_t* __restrict__ owner) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const long base = (long)t * cap;
  uint32_t* ow = owner + (size_t)t * (size_t)W * (size_t)H;
  for (int i = blockIdx.x * DN_THREADS + threadIdx.x; i < m; i += gridDim.x * DN_THREADS) {
    int sx, sy, tx, ty;
    if (!cs_ends(rec[base + i], W, H, sx, sy, tx, ty)) continue;
    if (!dn_admitted(ref, base + i, max_cost)) continue;
    atomicMin(&ow[(size_t)sy * (size_t)W + (size_t)sx], (uint32_t)i);  // (0 <= sx < W, 0 <= sy < H: cs_ends)
  }
}

// first cell of level l (2 .. 5) among a tile's cells in LDS
__device__ __forceinline__ int dn_lds_off(int l) { return l == 1 ? 0 : l == 2 ? 256 : l == 3 ? 320 : l == 4 ? 336 : 340; }

// grid (tiles in x, tiles in y, P): value[t][c][y][x] of the tile's pixels, and the tile's cells of levels 1 .. min(5, top)
template <bool CORR>
__global__ __launch_bounds__(DN_THREADS) void k_dense_pull(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                           const uint2* __restrict__ ref, const uint32_t* __restrict__ owner,
                                                           DnGeom g, long cells, int32_t* __restrict__ value,
                                                           int32_t* __restrict__ pn, int64_t* __restrict__ ps) {
  constexpr int C = CORR ? 2 : 1;
  __shared__ int32_t s_val[C][DN_TILE][DN_TILE];
  __shared__ int32_t s_n[DN_LDS_CELLS];
  __shared__ int64_t s_s[C][DN_LDS_CELLS];
  const int t = blockIdx.z, tid = threadIdx.x;
  const size_t npix = (size_t)g.W * (size_t)g.H;
  const uint32_t* ow = owner + (size_t)t * npix;
  int32_t* val = value + (size_t)t * C * npix;
  const long rbase = (long)t * cap;
  {
    const int xx = tid & 31, x = blockIdx.x * DN_TILE + xx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * DN_TILE + yy;
      int32_t v[C];
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = DN_NONE;
      if (x < g.W && y < g.H) {
        const size_t at = (size_t)y * (size_t)g.W + (size_t)x;
        const uint32_t o = ow[at];
        if (o != DN_NOBODY) {  // (o < m_t <= cap: k_dense_claim wrote it)
          int dx, dy;
          dn_shift(ref, rbase + (long)o, dx, dy);
          dn_value(rec[rbase + (long)o], dx, dy, v);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) val[(size_t)c * npix + at] = v[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) s_val[c][yy][xx] = v[c];
    }
  }
  __syncthreads();
  int32_t* gn = pn + (size_t)t * (size_t)cells;
  int64_t* gs = ps + (size_t)t * (size_t)cells * C;
  {  // level 1: a lane per cell of 2x2 pixels
    const int cx = tid & 15, cy = tid >> 4;
    int32_t n = 0;
    int64_t s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (s_val[0][2 * cy + j][2 * cx + i] == DN_NONE) continue;
        ++n;
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] += s_val[c][2 * cy + j][2 * cx + i];
      }
    s_n[tid] = n;
#pragma unroll
    for (int c = 0; c < C; ++c) s_s[c][tid] = s[c];
    const int X = blockIdx.x * 16 + cx, Y = blockIdx.y * 16 + cy;
    if (X < g.gw[1] && Y < g.gh[1]) {  // (top >= 1 always)
      const size_t at = (size_t)g.off[1] + (size_t)Y * (size_t)g.gw[1] + (size_t)X;
      gn[at] = n;
#pragma unroll
      for (int c = 0; c < C; ++c) gs[at * C + c] = s[c];
    }
  }
  __syncthreads();
#pragma unroll
  for (int l = 2; l <= DN_TILE_LEVELS; ++l) {
    const int side = DN_TILE >> l, below = dn_lds_off(l - 1), here = dn_lds_off(l);
    if (tid < side * side) {
      const int i = tid & (side - 1), j = tid >> (DN_TILE_LEVELS - l);  // (side = 2^(5 - l))
      int32_t n = 0;
      int64_t s[C];
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = below + (2 * j + (q >> 1)) * (2 * side) + 2 * i + (q & 1);
        n += s_n[ch];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] += s_s[c][ch];
      }
      s_n[here + tid] = n;
#pragma unroll
      for (int c = 0; c < C; ++c) s_s[c][here + tid] = s[c];
      const int X = blockIdx.x * side + i, Y = blockIdx.y * side + j;
      if (l <= g.top && X < g.gw[l] && Y < g.gh[l]) {
        const size_t at = (size_t)g.off[l] + (size_t)Y * (size_t)g.gw[l] + (size_t)X;
        gn[at] = n;
#pragma unroll
        for (int c = 0; c < C; ++c) gs[at * C + c] = s[c];
      }
    }
    __syncthreads();
  }
}

// grid (P): levels 6 .. top of pair t, each cell the sum of its (up to) four children
template <int C>
__global__ __launch_bounds__(DN_THREADS) void k_dense_top(DnGeom g, long cells, int32_t* pn, int64_t* ps) {
  const int t = blockIdx.x;
  int32_t* gn = pn + (size_t)t * (size_t)cells;
  int64_t* gs = ps + (size_t)t * (size_t)cells * C;
  for (int l = DN_TILE_LEVELS + 1; l <= g.top; ++l) {
    const int w = g.gw[l], h = g.gh[l], cw = g.gw[l - 1], ch = g.gh[l - 1];
    for (int idx = threadIdx.x; idx < w * h; idx += DN_THREADS) {
      const int Y = idx / w, X = idx - Y * w;
      int32_t n = 0;
      int64_t s[C];
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x = 2 * X + (q & 1), y = 2 * Y + (q >> 1);
        if (x >= cw || y >= ch) continue;
        const size_t at = (size_t)g.off[l - 1] + (size_t)y * (size_t)cw + (size_t)x;
        n += __hip_atomic_load(&gn[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] += __hip_atomic_load(&gs[at * C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const size_t at = (size_t)g.off[l] + (size_t)idx;
      __hip_atomic_store(&gn[at], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int c = 0; c < C; ++c) __hip_atomic_store(&gs[at * C + c], s[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();
    __syncthreads();
  }
}

// grid (tiles in x, tiles in y, P): value and level of every pixel of the tile
template <int C>
__global__ __launch_bounds__(DN_THREADS) void k_dense_push(DnGeom g, long cells, const int32_t* __restrict__ pn,
                                                           const int64_t* __restrict__ ps, int32_t* __restrict__ value,
                                                           uint8_t* __restrict__ level) {
  __shared__ int32_t s_ans[C][DN_THREADS];
  __shared__ int32_t s_lev[DN_THREADS];
  const int t = blockIdx.z, tid = threadIdx.x;
  const int32_t* gn = pn + (size_t)t * (size_t)cells;
  const int64_t* gs = ps + (size_t)t * (size_t)cells * C;
  {
    const int X1 = blockIdx.x * 16 + (tid & 15), Y1 = blockIdx.y * 16 + (tid >> 4);
    int32_t ans[C];
#pragma unroll
    for (int c = 0; c < C; ++c) ans[c] = DN_NONE;
    int lev = 255;
    if (X1 < g.gw[1] && Y1 < g.gh[1]) {
      for (int l = 1; l <= g.top; ++l) {
        const int X = X1 >> (l - 1), Y = Y1 >> (l - 1), w = g.gw[l], h = g.gh[l];
        const int x0 = max(X - g.spread, 0), x1 = min(X + g.spread, w - 1), y0 = max(Y - g.spread, 0), y1 = min(Y + g.spread, h - 1);
        const size_t lb = (size_t)g.off[l];
        int32_t n = 0;  // (the cells are disjoint blocks of one image: at most 2^30)
        for (int y = y0; y <= y1; ++y)
          for (int x = x0; x <= x1; ++x) n += gn[lb + (size_t)y * (size_t)w + (size_t)x];
        if (n < g.min_count) continue;
        int64_t s[C];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = 0;
        for (int y = y0; y <= y1; ++y)
          for (int x = x0; x <= x1; ++x) {
            const size_t at = (lb + (size_t)y * (size_t)w + (size_t)x) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] += gs[at + c];
          }
#pragma unroll
        for (int c = 0; c < C; ++c) ans[c] = dn_mean(s[c], n);
        lev = l;
        break;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) s_ans[c][tid] = ans[c];
    s_lev[tid] = lev;
  }
  __syncthreads();
  const size_t npix = (size_t)g.W * (size_t)g.H;
  int32_t* val = value + (size_t)t * C * npix;
  uint8_t* lv = level ? level + (size_t)t * npix : nullptr;
  const int xx = tid & 31, x = blockIdx.x * DN_TILE + xx;
  if (x >= g.W) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * DN_TILE + yy;
    if (y >= g.H) continue;
    const size_t at = (size_t)y * (size_t)g.W + (size_t)x;
    const int cell = (yy >> 1) * 16 + (xx >> 1);
    const bool own = val[at] != DN_NONE;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int32_t v = val[(size_t)c * npix + at];
      val[(size_t)c * npix + at] = own ? v : s_ans[c][cell];
    }
    if (lv) lv[at] = (uint8_t)(own ? 0 : s_lev[cell]);
  }
}

}  // namespace gpc
