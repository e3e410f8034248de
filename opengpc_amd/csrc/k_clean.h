// k_clean.h -- cleaning a dense field (gpc_hip_clean_*): the left-right check, the removal of small connected segments
// and a small median.  include/gpc_hip.h has the rule in full; it is made of integers only.
//   k_clean_flip     one lane per record: the record read from its target's side (slot i to slot i; in place is allowed);
//   k_clean_check    one lane per pixel: does it have a value, does it pass the check against the backward field.  The
//                    label plane starts as the pixel's own index (-1 where the pixel is out), the size plane as 0;
//   k_clean_tile     one workgroup per 32x32 tile: a union-find in LDS.  Row runs first -- a ballot of "belongs to my left
//                    neighbour" per half wave gives every pixel its run's first pixel without a single union -- then one
//                    union per pair of runs that touch vertically (a pixel whose left neighbour makes the same union is
//                    skipped), then every pixel finds its root and writes it as a GLOBAL pixel index;
//   k_clean_border   one lane per pixel on an inner tile edge: find / atomicMin on the global plane until the two roots are
//                    one (Komura; Playne & Hawick).  A parent is always a lower index than its child, so every find and every
//                    retry moves to a lower index and ends; nobody waits for anybody;
//   k_clean_flatten  one lane per pixel: the root of its tree, which is the lowest index of its component;
//   k_clean_sizes    one workgroup per tile: run heads add their run's length to a 128-slot table in LDS keyed by root (a
//                    tile mostly sees a handful of roots), the table's entries go to the size plane with one atomic each;
//   k_clean_apply    one workgroup per tile: states and kept flags of the tile and its halo staged in LDS with the values,
//                    the lower median by counting ranks (for each candidate of the window, how many kept values are below
//                    it and how many equal it), the outputs, and the four state counts reduced by ballots.
// Sums and differences are taken in 64 bits: any int32 but GPC_DENSE_NONE in channel 0 is a value.
#pragma once
#include "clean_host.h"
#include "gpc_device.h"
#include "k_consensus.h"  // ConsRec, cs_count

#define CL_THREADS 256
#define CL_NONE ((int32_t)0x80000000)  // GPC_DENSE_NONE
#define CL_TAB 128                     // slots of the size kernel's table of roots
#define CL_CHECK_W 64                  // k_clean_check, k_clean_flatten: a workgroup is 64 x 4 pixels
#define CL_CHECK_H 4

namespace gpc {

__device__ __forceinline__ bool cl_near(int32_t a, int32_t b, int32_t diff) {
  const int64_t d = (int64_t)a - (int64_t)b;
  return (d < 0 ? -d : d) <= (int64_t)diff;
}

// sgn(f) * ((|f| + 128) >> 8): the whole-pixel shift, rounded half away from zero
__device__ __forceinline__ int64_t cl_round(int32_t f) {
  const int64_t a = f < 0 ? -(int64_t)f : (int64_t)f, r = (a + 128) >> 8;
  return f < 0 ? -r : r;
}

__device__ __forceinline__ ConsRec<true> cl_flipped(const ConsRec<true>& r) { return ConsRec<true>{r.tx, r.ty, r.sx, r.sy}; }
__device__ __forceinline__ ConsRec<false> cl_flipped(const ConsRec<false>& r) {
  const float d = r.d;
  // (NaN fails the first comparison, +-inf the second)
  if (!(d == truncf(d) && fabsf(d) < 16777216.f)) return ConsRec<false>{-1, -1, 0.f};
  return ConsRec<false>{(int32_t)((uint32_t)r.x - (uint32_t)(int)d), r.y, -d};
}

// grid (x, P): rec_out[t][i] = the reverse of rec[t][i], ref_out[t][i] = ref[t][i] with its shifts negated, i < m_t.
// rec_out == rec and ref_out == ref are allowed: a lane reads its slot before it writes it, and no other lane touches it.
template <bool CORR>
__global__ __launch_bounds__(CL_THREADS) void k_clean_flip(const ConsRec<CORR>* rec, const uint2* ref, int cap,
                                                           const int32_t* __restrict__ counts, ConsRec<CORR>* rec_out,
                                                           uint2* ref_out) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const long base = (long)t * cap;
  for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < m; i += gridDim.x * CL_THREADS) {
    const ConsRec<CORR> r = rec[base + i];
    rec_out[base + i] = cl_flipped(r);
    if (ref_out) {
      uint2 f = ref[base + i];
      const uint32_t dx = (0u - (f.x & 0xFFFFu)) & 0xFFFFu, dy = (0u - (f.x >> 16)) & 0xFFFFu;
      f.x = dx | (dy << 16);
      ref_out[base + i] = f;
    }
  }
}

// grid (W / 64, H / 4, P): label[t][p] = p where pixel p has a value and passes the check (tol >= 0), else -1; size[t][p]
// = 0 where a size plane is given
template <int C>
__global__ __launch_bounds__(CL_THREADS) void k_clean_check(const int32_t* __restrict__ fwd, const int32_t* __restrict__ bwd,
                                                            int W, int H, int tol, int32_t* __restrict__ label,
                                                            int32_t* __restrict__ size) {
  const int x = blockIdx.x * CL_CHECK_W + (threadIdx.x & (CL_CHECK_W - 1));
  const int y = blockIdx.y * CL_CHECK_H + (threadIdx.x / CL_CHECK_W);
  if (x >= W || y >= H) return;
  const size_t npix = (size_t)W * (size_t)H, at = (size_t)y * (size_t)W + (size_t)x;
  const size_t pair = (size_t)blockIdx.z * npix;
  const int32_t* F = fwd + pair * C;
  int32_t f[C];
#pragma unroll
  for (int c = 0; c < C; ++c) f[c] = F[(size_t)c * npix + at];
  bool ok = f[0] != CL_NONE;
  if (ok && tol >= 0) {
    const int64_t qx = C == 1 ? (int64_t)x - cl_round(f[0]) : (int64_t)x + cl_round(f[0]);
    const int64_t qy = C == 1 ? (int64_t)y : (int64_t)y + cl_round(f[C - 1]);
    ok = qx >= 0 && qx < W && qy >= 0 && qy < H;
    if (ok) {
      const int32_t* G = bwd + pair * C;
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      int32_t g[C];
#pragma unroll
      for (int c = 0; c < C; ++c) g[c] = G[(size_t)c * npix + q];
      ok = g[0] != CL_NONE;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t s = (int64_t)f[c] + (int64_t)g[c];
        ok = ok && (s < 0 ? -s : s) <= (int64_t)tol;
      }
    }
  }
  label[pair + at] = ok ? (int32_t)at : -1;
  if (size) size[pair + at] = 0;
}

__device__ __forceinline__ int cl_lds_find(int32_t* lab, int a) {
  for (;;) {  // (a parent is a lower index than its child)
    const int p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void cl_lds_union(int32_t* lab, int a, int b) {
  for (;;) {
    a = cl_lds_find(lab, a), b = cl_lds_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b, b = s;
    }
    const int old = atomicMin(&lab[a], b);  // the higher root takes the lower one as its parent, if it still is a root
    if (old == a) return;
    a = old;  // (old < a: somebody gave it a parent; that parent and b still have to meet)
  }
}

// grid (tiles in x, tiles in y, P): label[t][p] = the lowest index of p's component WITHIN its tile
template <int C>
__global__ __launch_bounds__(CL_THREADS) void k_clean_tile(const int32_t* __restrict__ fwd, int W, int H, int diff,
                                                           int32_t* __restrict__ label) {
  __shared__ int32_t s_val[C][CL_TILE * CL_TILE];
  __shared__ int32_t s_lab[CL_TILE * CL_TILE];
  __shared__ uint32_t s_rm[CL_TILE];  // per row: bit x = pixel x belongs to pixel x - 1
  const int tid = threadIdx.x, xx = tid & 31, x = blockIdx.x * CL_TILE + xx;
  const size_t npix = (size_t)W * (size_t)H, pair = (size_t)blockIdx.z * npix;
  const int32_t* F = fwd + pair * C;
  int32_t* L = label + pair;
  int32_t v[4][C];
  bool valid[4], cl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * CL_TILE + yy;
    const bool inside = x < W && y < H;
    const size_t at = inside ? (size_t)y * (size_t)W + (size_t)x : 0;
    valid[k] = inside && L[at] >= 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      v[k][c] = valid[k] ? F[(size_t)c * npix + at] : 0;
      s_val[c][yy * CL_TILE + xx] = v[k][c];
    }
    bool conn = __shfl_up((int)valid[k], 1, 32) != 0;
#pragma unroll
    for (int c = 0; c < C; ++c) conn = cl_near(v[k][c], __shfl_up(v[k][c], 1, 32), diff) && conn;
    conn = conn && valid[k] && xx > 0;
    cl[k] = conn;
    const unsigned long long b = __ballot(conn);
    const uint32_t m = (tid & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
    const uint32_t open = ~m & (0xFFFFFFFFu >> (31 - xx));  // (bit 0 is always set: pixel 0 starts a run)
    s_lab[yy * CL_TILE + xx] = valid[k] ? yy * CL_TILE + (31 - __clz(open)) : -1;
    if (xx == 0) s_rm[yy] = m;
  }
  __syncthreads();
  bool todo[4];  // (decided for all four rows before the first union: the shuffles see whole waves)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k, up = (yy > 0 ? yy - 1 : 0) * CL_TILE + xx;
    bool cu = yy > 0 && valid[k] && s_lab[up] >= 0;
#pragma unroll
    for (int c = 0; c < C; ++c) cu = cu && cl_near(v[k][c], s_val[c][up], diff);
    // my left neighbour makes the same union when it is joined to me, to its upper neighbour, and that one to mine
    const bool left_up = __shfl_up((int)cu, 1, 32) != 0;
    const bool same = cl[k] && left_up && yy > 0 && ((s_rm[yy > 0 ? yy - 1 : 0] >> xx) & 1u);
    todo[k] = cu && !same;
  }
  __syncthreads();  // (every run label is read above before a union changes one)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k;
    if (todo[k]) cl_lds_union(s_lab, yy * CL_TILE + xx, (yy - 1) * CL_TILE + xx);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * CL_TILE + yy;
    if (!valid[k]) continue;
    const int r = cl_lds_find(s_lab, yy * CL_TILE + xx);
    const int ry = blockIdx.y * CL_TILE + (r >> 5), rx = blockIdx.x * CL_TILE + (r & 31);
    L[(size_t)y * (size_t)W + (size_t)x] = ry * W + rx;  // (below 2^30)
  }
}

__device__ __forceinline__ int cl_find(int32_t* lab, int a) {
  for (;;) {
    const int p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void cl_union(int32_t* lab, int a, int b) {
  for (;;) {
    a = cl_find(lab, a), b = cl_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b, b = s;
    }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ bool cl_joined(const int32_t* __restrict__ F, size_t npix, int C, size_t p, size_t q, int diff) {
  bool j = true;
  for (int c = 0; c < C; ++c) j = j && cl_near(F[(size_t)c * npix + p], F[(size_t)c * npix + q], diff);
  return j;
}

// grid (lanes / 256, 1, P): lane i < (tiles_x - 1) * H is the pixel (32 (i / H + 1), i % H) and its left neighbour, the others
// the pixel (j % W, 32 (j / W + 1)), j = i - (tiles_x - 1) * H, and its upper neighbour
template <int C>
__global__ __launch_bounds__(CL_THREADS) void k_clean_border(const int32_t* __restrict__ fwd, int W, int H, int diff, int nv,
                                                             int lanes, int32_t* label) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= lanes) return;
  const size_t npix = (size_t)W * (size_t)H, pair = (size_t)blockIdx.z * npix;
  const int32_t* F = fwd + pair * C;
  int32_t* L = label + pair;
  int x, y, along;  // `along`: the step to the previous pixel on the same tile edge
  int q;            // the neighbour across the edge
  bool first;       // no previous pixel on this edge of the tile
  if (i < nv) {
    const int b = i / H;
    y = i - b * H, x = (b + 1) * CL_TILE;
    q = y * W + x - 1, along = -W, first = (y & (CL_TILE - 1)) == 0;
  } else {
    const int j = i - nv, b = j / W;
    x = j - b * W, y = (b + 1) * CL_TILE;
    q = (y - 1) * W + x, along = -1, first = (x & (CL_TILE - 1)) == 0;
  }
  const int p = y * W + x;
  // (whether a pixel is in or out never changes after k_clean_check: a plain read of the sign is enough)
  if (L[p] < 0 || L[q] < 0 || !cl_joined(F, npix, C, (size_t)p, (size_t)q, diff)) return;
  if (!first) {  // the previous pixel on this edge makes the same union when the four are joined round (inside the tiles)
    const int p2 = p + along, q2 = q + along;
    if (L[p2] >= 0 && L[q2] >= 0 && cl_joined(F, npix, C, (size_t)p, (size_t)p2, diff) &&
        cl_joined(F, npix, C, (size_t)q, (size_t)q2, diff) && cl_joined(F, npix, C, (size_t)p2, (size_t)q2, diff))
      return;
  }
  cl_union(L, p, q);
}

// grid (W / 64, H / 4, P): label[t][p] = the root of p's tree
__global__ __launch_bounds__(CL_THREADS) void k_clean_flatten(int W, int H, int32_t* label) {
  const int x = blockIdx.x * CL_CHECK_W + (threadIdx.x & (CL_CHECK_W - 1));
  const int y = blockIdx.y * CL_CHECK_H + (threadIdx.x / CL_CHECK_W);
  if (x >= W || y >= H) return;
  int32_t* L = label + (size_t)blockIdx.z * (size_t)W * (size_t)H;
  const int p = y * W + x;
  const int l = __hip_atomic_load(&L[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (l < 0 || l == p) return;
  // (another lane may overwrite a word on the way with its root: that is the same root, a step early)
  __hip_atomic_store(&L[p], cl_find(L, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (tiles in x, tiles in y, P): size[t][root] += the tile's pixels of that root
__global__ __launch_bounds__(CL_THREADS) void k_clean_sizes(const int32_t* __restrict__ label, int W, int H,
                                                            int32_t* __restrict__ size) {
  __shared__ int32_t s_key[CL_TAB];
  __shared__ int32_t s_cnt[CL_TAB];
  const int tid = threadIdx.x, xx = tid & 31, x = blockIdx.x * CL_TILE + xx;
  const size_t pair = (size_t)blockIdx.z * (size_t)W * (size_t)H;
  const int32_t* L = label + pair;
  int32_t* S = size + pair;
  if (tid < CL_TAB) s_key[tid] = -1, s_cnt[tid] = 0;
  __syncthreads();
  int labs[4], runs[4];  // (all four rows before the first insertion: shuffles and ballots see whole waves)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = blockIdx.y * CL_TILE + (tid >> 5) + 8 * k;
    const int lab = x < W && y < H ? L[(size_t)y * (size_t)W + (size_t)x] : -1;
    const int left = __shfl_up(lab, 1, 32);
    const bool cont = xx > 0 && lab >= 0 && left == lab;
    const unsigned long long b = __ballot(cont);
    const uint32_t m = (tid & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
    // a run's head: the run ends before the first pixel above x that does not continue it (bit 32 stops the search)
    const unsigned long long stop = ((unsigned long long)(~m) | (1ull << 32)) >> (xx + 1);
    labs[k] = cont ? -1 : lab;
    runs[k] = __ffsll(stop);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int lab = labs[k], n = runs[k];
    if (lab < 0) continue;
    uint32_t h = ((uint32_t)lab * 2654435761u) >> 25;
    bool placed = false;
    for (int tries = 0; tries < CL_TAB && !placed; ++tries, h = (h + 1) & (CL_TAB - 1)) {
      const int old = atomicCAS(&s_key[h], -1, lab);
      if (old == -1 || old == lab) {
        atomicAdd(&s_cnt[h], n);
        placed = true;
      }
    }
    if (!placed) atomicAdd(&S[lab], n);  // more roots than slots in this tile
  }
  __syncthreads();
  if (tid < CL_TAB && s_key[tid] >= 0) atomicAdd(&S[s_key[tid]], s_cnt[tid]);
}

// grid (tiles in x, tiles in y, P): out, state and stats of the tile's pixels.  R = median_radius.
template <int C, int R>
__global__ __launch_bounds__(CL_THREADS) void k_clean_apply(const int32_t* __restrict__ fwd, const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ size, int W, int H, int smin,
                                                            int32_t* __restrict__ out, uint8_t* __restrict__ state,
                                                            int32_t* __restrict__ stats) {
  constexpr int E = CL_TILE + 2 * R, N = (2 * R + 1) * (2 * R + 1);
  __shared__ int32_t s_v[C][E * E];
  __shared__ uint8_t s_st[E * E];  // the state; 1 outside the image
  __shared__ int32_t s_n[4];
  const int tid = threadIdx.x;
  const size_t npix = (size_t)W * (size_t)H, pair = (size_t)blockIdx.z * npix;
  const int32_t* F = fwd + pair * C;
  const int32_t* L = label + pair;
  const int32_t* S = size ? size + pair : nullptr;
  if (tid < 4) s_n[tid] = 0;
  for (int i = tid; i < E * E; i += CL_THREADS) {
    const int ly = i / E, lx = i - ly * E;
    const int gx = blockIdx.x * CL_TILE - R + lx, gy = blockIdx.y * CL_TILE - R + ly;
    int st = 1;
    int32_t f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t at = (size_t)gy * (size_t)W + (size_t)gx;
#pragma unroll
      for (int c = 0; c < C; ++c) f[c] = F[(size_t)c * npix + at];
      const int lab = L[at];
      if (lab < 0) st = f[0] == CL_NONE ? 1 : 2;
      else st = (smin > 1 && S[lab] < smin) ? 3 : 0;
    }
    s_st[i] = (uint8_t)st;
#pragma unroll
    for (int c = 0; c < C; ++c) s_v[c][i] = f[c];
  }
  __syncthreads();
  const int xx = tid & 31, x = blockIdx.x * CL_TILE + xx;
  int32_t* O = out + pair * C;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // the state counts, by whole waves
    const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * CL_TILE + yy;
    const int st = x < W && y < H ? (int)s_st[(yy + R) * E + xx + R] : 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const unsigned long long b = __ballot(st == s);
      if ((tid & 63) == 0 && b) atomicAdd(&s_n[s], __popcll(b));
    }
  }
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int yy = (tid >> 5) + 8 * k, y = blockIdx.y * CL_TILE + yy;
    const bool inside = x < W && y < H;
    const int centre = (yy + R) * E + xx + R;
    const int st = inside ? (int)s_st[centre] : 4;
    if (!inside) continue;
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    if (state) state[pair + at] = (uint8_t)st;
    if (st != 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) O[(size_t)c * npix + at] = CL_NONE;
      continue;
    }
    if (R == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) O[(size_t)c * npix + at] = s_v[c][centre];
      continue;
    }
    uint32_t kept = 0;  // bit j: window element j is a kept pixel
#pragma unroll
    for (int j = 0; j < N; ++j)
      kept |= (uint32_t)(s_st[(yy + j / (2 * R + 1)) * E + xx + j % (2 * R + 1)] == 0) << j;
    const int target = (__popc(kept) - 1) >> 1;  // (the centre is kept: at least one)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      int32_t w[N];  // (only ever indexed by unrolled constants: registers)
#pragma unroll
      for (int j = 0; j < N; ++j) w[j] = s_v[c][(yy + j / (2 * R + 1)) * E + xx + j % (2 * R + 1)];
      int32_t med = w[N / 2];
#pragma unroll 1
      for (int i = 0; i < N; ++i) {  // the candidate comes from LDS, so that no register array is indexed by i
        if (!((kept >> i) & 1u)) continue;
        const int32_t cand = s_v[c][(yy + i / (2 * R + 1)) * E + xx + i % (2 * R + 1)];
        int lo = 0, eq = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const int in = (int)((kept >> j) & 1u);
          lo += in & (int)(w[j] < cand);
          eq += in & (int)(w[j] == cand);
        }
        if (lo <= target && target < lo + eq) med = cand;
      }
      O[(size_t)c * npix + at] = med;
    }
  }
  __syncthreads();
  if (stats && tid < 4 && s_n[tid]) atomicAdd(&stats[(size_t)blockIdx.z * 4 + tid], s_n[tid]);
}

}  // namespace gpc
