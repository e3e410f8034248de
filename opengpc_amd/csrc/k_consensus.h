// k_consensus.h -- grid motion consensus (gpc_hip_consensus_*): a record is kept when enough records around its source
// move the same way.  include/gpc_hip.h has the rule in full; it is made of integers only.  Under a grid of cells of edge c
// (offset by half a cell in x, y or both for the grids 1 .. 3) a record has a source cell A and a displacement class D =
// cell(target) - cell(source); S counts the records of the 3x3 cells around A with the same class, T all records there,
// k the cells there, and the record passes when S^2 * k * alpha_den^2 > alpha_num^2 * T.
// One grid at a time, every launch a step of its own (nothing waits across workgroups inside a launch):
//   k_cons_cells    per record: does it take part, its source cell; histogram of the cells (global integer adds); grid 0
//                   also clears the keep mask of the records read;
//   k_cons_scan     one workgroup per pair: exclusive scan of the pair's histogram -> the cells' first positions (and the
//                   scatter's cursors); also used for the chunk counts of the compaction;
//   k_cons_scatter  counting sort by source cell: (class, record index) to the cell's positions.  The order inside a cell
//                   is whichever thread came first -- nothing below depends on it;
//   k_cons_count    one workgroup per occupied source cell: the classes of the 3x3 neighbourhood (three runs of sorted
//                   positions, a cell row each) are counted in an open-addressing table in LDS (claim the key with a
//                   compare-and-swap, add to its count: integer atomics, the same sums in any order), the cell's own
//                   records read their S, T and k come from the cells' first positions, the test sets the grid's bit.
//                   A neighbourhood with more distinct classes than the table takes is counted in 2, 4, 8 ... passes,
//                   pass p over the classes whose hash falls in slice p; the result never depends on the table's size;
//   k_cons_blocks   kept records per chunk of 2048; k_cons_scan makes them offsets and a pair's total;
//   k_cons_write    the kept records and their input indices, in input order.
#pragma once
#include "gpc_device.h"

#define CS_THREADS 256
#define CS_CHUNK (CS_THREADS * 8)   // records per workgroup of the compaction kernels
#define CS_TAB 2048                 // slots of the class table (16 KiB of LDS)
#define CS_TAB_LIMIT 1536           // distinct classes a pass may claim: every thread may claim one more before it sees the
                                    // flag, 1536 + 256 < 2048, so a probe always meets a free slot
#define CS_NOKEY 0xFFFFFFFFu        // free slot / a record that takes no part (a class is below 2^26)

namespace gpc {

template <bool CORR> struct ConsRec;
template <> struct ConsRec<true> {  // gpc_correspondence
  int32_t sx, sy, tx, ty;
};
template <> struct ConsRec<false> {  // gpc_support
  int32_t x, y;
  float d;
};

// one grid of the call; made on the host
struct ConsGrid {
  int W, H;
  int ox, oy;        // the grid's offset: 0 or c / 2
  int gx, gy;        // columns, rows
  int ncell;         // gx * gy
  uint32_t kw;       // 2 * gx - 1: classes per row of the class plane
  GpcDivW dc;        // division by the cell edge (coordinates + offset stay below 2^31)
  GpcDivW dgx;       // division of a cell index by gx (gx > 1)
  uint32_t bit;      // the grid's bit of the keep mask
  uint32_t kq;       // alpha_den^2 (<= 4096)
  uint32_t an2;      // alpha_num^2 (<= 2^20)
};

__device__ __forceinline__ int cs_count(const int32_t* __restrict__ counts, int t, int cap) {
  const int m = counts[t];
  return m < 0 ? 0 : (m > cap ? cap : m);
}

// source and target of a record; false: it takes no part
__device__ __forceinline__ bool cs_ends(const ConsRec<true>& r, int W, int H, int& sx, int& sy, int& tx, int& ty) {
  sx = r.sx, sy = r.sy, tx = r.tx, ty = r.ty;
  return (uint32_t)sx < (uint32_t)W && (uint32_t)sy < (uint32_t)H && (uint32_t)tx < (uint32_t)W && (uint32_t)ty < (uint32_t)H;
}
__device__ __forceinline__ bool cs_ends(const ConsRec<false>& r, int W, int H, int& sx, int& sy, int& tx, int& ty) {
  sx = r.x, sy = r.y, ty = r.y;
  const float d = r.d;
  // (NaN fails the first comparison, +-inf the second; a d below 2^24 in magnitude that equals its truncation is an int)
  const bool whole = d == truncf(d) && fabsf(d) < 16777216.f;
  tx = whole ? (int)((uint32_t)sx - (uint32_t)(int)d) : -1;  // (wraps for an x far outside the image, which fails below anyway)
  return whole && (uint32_t)sx < (uint32_t)W && (uint32_t)sy < (uint32_t)H && (uint32_t)tx < (uint32_t)W;
}

// source cell (row-major) and class of a record that takes part.  Cell coordinates and gx stay below 2^24: 24-bit multiplies.
__device__ __forceinline__ void cs_classify(const ConsGrid& g, int sx, int sy, int tx, int ty, uint32_t& cell, uint32_t& key) {
  const int scx = divw((uint32_t)(sx + g.ox), g.dc), scy = divw((uint32_t)(sy + g.oy), g.dc);
  const int tcx = divw((uint32_t)(tx + g.ox), g.dc), tcy = divw((uint32_t)(ty + g.oy), g.dc);
  cell = __umul24((uint32_t)scy, (uint32_t)g.gx) + (uint32_t)scx;
  key = __umul24((uint32_t)(tcy - scy + g.gy - 1), g.kw) + (uint32_t)(tcx - scx + g.gx - 1);
}

// grid (x, P): hist[t][cell] += 1 for every record of pair t that takes part
template <bool CORR>
__global__ __launch_bounds__(CS_THREADS) void k_cons_cells(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                           const int32_t* __restrict__ counts, ConsGrid g,
                                                           int32_t* __restrict__ hist, uint8_t* __restrict__ keep) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const ConsRec<CORR>* r = rec + (long)t * cap;
  int32_t* h = hist + (long)t * g.ncell;
  uint8_t* kp = keep + (long)t * cap;
  for (int i = blockIdx.x * CS_THREADS + threadIdx.x; i < m; i += gridDim.x * CS_THREADS) {
    int sx, sy, tx, ty;
    if (g.bit == 1u) kp[i] = 0;
    if (cs_ends(r[i], g.W, g.H, sx, sy, tx, ty)) {
      uint32_t cell, key;
      cs_classify(g, sx, sy, tx, ty, cell, key);
      atomicAdd(&h[cell], 1);
    }
  }
}

// grid (P), 1024 threads: start[t * sstride + j] = sum of cnt[t * cstride + 0 .. j); TAIL: start[t * sstride + n] = the
// sum; CURSOR: cnt[..][j] gets the same offsets (the scatter's cursors); total[t] = the sum where total is given.
// cnt == start with equal strides is allowed (every word is read before it is written, by the same thread).
template <bool TAIL, bool CURSOR>
__global__ __launch_bounds__(1024) void k_cons_scan(int32_t* cnt, long cstride, int n, int32_t* start, long sstride,
                                                    int32_t* __restrict__ total) {
  __shared__ int s_w[16];
  __shared__ int s_carry;
  const int t = blockIdx.x;
  int32_t* in = cnt + (long)t * cstride;
  int32_t* out = start + (long)t * sstride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const int x = i < n ? in[i] : 0;
    const int incl = (int)wave_incl_scan((uint32_t)x);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    const int carry = s_carry;
    if (i < n) {
      const int ex = carry + woff + incl - x;
      out[i] = ex;
      if (CURSOR) in[i] = ex;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (TAIL) out[n] = s_carry;
    if (total) total[t] = s_carry;
  }
}

// grid (x, P): record i of a cell goes to the next free position of that cell
template <bool CORR>
__global__ __launch_bounds__(CS_THREADS) void k_cons_scatter(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                             const int32_t* __restrict__ counts, ConsGrid g,
                                                             int32_t* __restrict__ cursor, uint32_t* __restrict__ skey,
                                                             int32_t* __restrict__ sidx) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const ConsRec<CORR>* r = rec + (long)t * cap;
  int32_t* cur = cursor + (long)t * g.ncell;
  uint32_t* sk = skey + (long)t * cap;
  int32_t* si = sidx + (long)t * cap;
  for (int i = blockIdx.x * CS_THREADS + threadIdx.x; i < m; i += gridDim.x * CS_THREADS) {
    int sx, sy, tx, ty;
    if (cs_ends(r[i], g.W, g.H, sx, sy, tx, ty)) {
      uint32_t cell, key;
      cs_classify(g, sx, sy, tx, ty, cell, key);
      const int pos = atomicAdd(&cur[cell], 1);  // (below the pair's number of records that take part, so below cap)
      sk[pos] = key;
      si[pos] = i;
    }
  }
}

// Hash of a class (below 2^26) with one 24-bit multiply: the low 32 bits of (low 24 bits of the class) * an odd constant
// -- one value per 24-bit input -- with the class's bits 24 and 25 folded into the top, so at most four classes share a
// value.  The table slot is the product's top 11 bits; the slice of a pass is taken from cs_slice's low bits, which fold
// the product's upper half onto its lower one, so the classes of one slice still spread over every slot.
__device__ __forceinline__ uint32_t cs_hash(uint32_t key) { return __umul24(key & 0xFFFFFFu, 0x9E3779u) ^ ((key >> 24) << 30); }
__device__ __forceinline__ uint32_t cs_slice(uint32_t h) { return h ^ (h >> 15); }
__device__ __forceinline__ uint32_t cs_slot(uint32_t h) { return h >> 21; }
static_assert(CS_TAB == 2048, "cs_slot takes 11 bits");

// grid (ncell, P): the source cell blockIdx.x of pair blockIdx.y.  start[t][0 .. ncell] are the cells' first sorted
// positions.  The table: tab[2 * slot] = class, tab[2 * slot + 1] = count.
__global__ __launch_bounds__(CS_THREADS) void k_cons_count(int cap, ConsGrid g, const int32_t* __restrict__ start,
                                                           const uint32_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                           uint8_t* __restrict__ keep) {
  const int a = blockIdx.x, t = blockIdx.y;
  const int32_t* st = start + (long)t * (g.ncell + 1);
  const int own0 = st[a], own1 = st[a + 1];
  if (own0 == own1) return;  // (uniform over the workgroup)
  const int cy = g.gx > 1 ? divw((uint32_t)a, g.dgx) : a;
  const int cx = a - (int)__umul24((uint32_t)cy, (uint32_t)g.gx);
  __shared__ uint32_t tab[2 * CS_TAB];
  __shared__ int s_distinct, s_over;
  const uint32_t* sk = skey + (long)t * cap;
  const int32_t* si = sidx + (long)t * cap;
  uint8_t* kp = keep + (long)t * cap;
  const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.gx ? cx + 1 : g.gx - 1;
  const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < g.gy ? cy + 1 : g.gy - 1;
  // the neighbourhood: one run of sorted positions per cell row (an absent row is an empty run)
  const int ra0 = st[(int)__umul24((uint32_t)y0, (uint32_t)g.gx) + x0], ra1 = st[(int)__umul24((uint32_t)y0, (uint32_t)g.gx) + x1 + 1];
  const bool two = y0 + 1 <= y1, three = y0 + 2 <= y1;
  const int rb0 = two ? st[(int)__umul24((uint32_t)(y0 + 1), (uint32_t)g.gx) + x0] : 0;
  const int rb1 = two ? st[(int)__umul24((uint32_t)(y0 + 1), (uint32_t)g.gx) + x1 + 1] : 0;
  const int rc0 = three ? st[(int)__umul24((uint32_t)(y0 + 2), (uint32_t)g.gx) + x0] : 0;
  const int rc1 = three ? st[(int)__umul24((uint32_t)(y0 + 2), (uint32_t)g.gx) + x1 + 1] : 0;
  const uint32_t T = (uint32_t)((ra1 - ra0) + (rb1 - rb0) + (rc1 - rc0));
  const uint32_t kcells = (uint32_t)((x1 - x0 + 1) * (y1 - y0 + 1));
  // S * S * k * alpha_den^2 > alpha_num^2 * T: S, T < 2^24, k * alpha_den^2 < 2^16, alpha_num^2 <= 2^20
  const unsigned long long rhs = (unsigned long long)g.an2 * (unsigned long long)T;
  const uint32_t kq = __umul24(kcells, g.kq);

  for (uint32_t np = 1;; np <<= 1) {  // passes: a power of two, doubled until every pass fits the table
    bool over = false;
    for (uint32_t p = 0; p < np && !over; ++p) {
      __syncthreads();  // (the table's last readers are done)
      for (int j = threadIdx.x; j < 2 * CS_TAB; j += CS_THREADS) tab[j] = (j & 1) ? 0u : CS_NOKEY;
      if (threadIdx.x == 0) s_distinct = 0, s_over = 0;
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < 3; ++k) {
        const int lo = k == 0 ? ra0 : (k == 1 ? rb0 : rc0), hi = k == 0 ? ra1 : (k == 1 ? rb1 : rc1);
#pragma unroll 1
        for (int j = lo + (int)threadIdx.x; j < hi; j += CS_THREADS) {
          const uint32_t key = sk[j];
          const uint32_t h = cs_hash(key);
          if ((cs_slice(h) & (np - 1u)) != p) continue;
          if (__hip_atomic_load(&s_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          uint32_t slot = cs_slot(h);
          for (int n = 0; n < CS_TAB; ++n) {  // (a free slot exists: CS_TAB_LIMIT)
            uint32_t seen = __hip_atomic_load(&tab[2 * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (seen == CS_NOKEY) {
              seen = atomicCAS(&tab[2 * slot], CS_NOKEY, key);
              if (seen == CS_NOKEY) {
                if (atomicAdd(&s_distinct, 1) >= CS_TAB_LIMIT) s_over = 1;
                seen = key;
              }
            }
            if (seen == key) {
              atomicAdd(&tab[2 * slot + 1], 1u);
              break;
            }
            slot = (slot + 1u) & (CS_TAB - 1u);
          }
        }
      }
      __syncthreads();
      over = s_over != 0;  // (uniform: read behind the barrier)
      if (over) break;
      // the cell's own records of this slice read their S
#pragma unroll 1
      for (int j = own0 + (int)threadIdx.x; j < own1; j += CS_THREADS) {
        const uint32_t key = sk[j];
        const uint32_t h = cs_hash(key);
        if ((cs_slice(h) & (np - 1u)) != p) continue;
        uint32_t slot = cs_slot(h);
        uint32_t S = 0;
        for (int n = 0; n < CS_TAB; ++n) {
          const uint32_t seen = tab[2 * slot];
          if (seen == key) {
            S = tab[2 * slot + 1];
            break;
          }
          if (seen == CS_NOKEY) break;  // (cannot happen: the record itself was counted)
          slot = (slot + 1u) & (CS_TAB - 1u);
        }
        const uint32_t s24 = S & 0xFFFFFFu;
        const unsigned long long lhs = (unsigned long long)s24 * s24 * (unsigned long long)kq;
        if (lhs > rhs) {
          const int i = si[j];
          kp[i] = (uint8_t)(kp[i] | g.bit);  // (a record has one source cell: nobody else touches its byte in this launch)
        }
      }
    }
    if (!over) break;
    // (bits set by the passes that ran stay: they are final, and the repeat sets the same ones again)
  }
}

// grid (nchunk, P): blkcnt[t * nchunk + b] = kept records of chunk b of pair t
__global__ __launch_bounds__(CS_THREADS) void k_cons_blocks(int cap, const int32_t* __restrict__ counts,
                                                            const uint8_t* __restrict__ keep, int32_t* __restrict__ blkcnt,
                                                            int nchunk) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const int i0 = blockIdx.x * CS_CHUNK;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int kept = 0;
  const uint8_t* kp = keep + (long)t * cap;
#pragma unroll 1
  for (int k = 0; k < CS_CHUNK / CS_THREADS; ++k) {
    const int i = i0 + k * CS_THREADS + threadIdx.x;
    if (i < m && kp[i] != 0) ++kept;
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&s_n, kept);
  __syncthreads();
  if (threadIdx.x == 0) blkcnt[(long)t * nchunk + blockIdx.x] = s_n;
}

// grid (nchunk, P): the kept records of chunk b of pair t go to out[t][blkoff[t * nchunk + b] + rank in record order]
template <bool CORR>
__global__ __launch_bounds__(CS_THREADS) void k_cons_write(const ConsRec<CORR>* __restrict__ rec, int cap,
                                                           const int32_t* __restrict__ counts, const uint8_t* __restrict__ keep,
                                                           const int32_t* __restrict__ blkoff, int nchunk,
                                                           ConsRec<CORR>* __restrict__ out, int cap_out,
                                                           int32_t* __restrict__ index) {
  const int t = blockIdx.y;
  const int m = cs_count(counts, t, cap);
  const int i0 = blockIdx.x * CS_CHUNK;
  if (i0 >= m) return;  // (uniform over the workgroup)
  const ConsRec<CORR>* r = rec + (long)t * cap;
  const uint8_t* kp = keep + (long)t * cap;
  ConsRec<CORR>* o = out + (long)t * cap_out;
  int32_t* ix = index ? index + (long)t * cap_out : nullptr;
  __shared__ int s_w[CS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pos = blkoff[(long)t * nchunk + blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < CS_CHUNK / CS_THREADS; ++k) {
    const int i = i0 + k * CS_THREADS + threadIdx.x;
    const bool kept = i < m && kp[i] != 0;
    const unsigned long long mk = __ballot(kept);
    if (lane == 0) s_w[wave] = __popcll(mk);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < CS_THREADS / 64; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    if (kept) {
      const int n = pos + woff + __popcll(mk & ((1ull << lane) - 1ull));
      if (n < cap_out) {
        o[n] = r[i];
        if (ix) ix[n] = i;
      }
    }
    pos += tot;
    __syncthreads();
  }
}

}  // namespace gpc
