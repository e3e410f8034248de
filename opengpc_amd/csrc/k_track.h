// k_track.h -- point tracks over a frame sequence (gpc_hip_track_*): the correspondences of consecutive pairs chained on
// the device.  Record i of pair t continues in record J of pair t + 1 when J is the lowest record of pair t + 1 whose
// source pixel is i's target pixel, and i is the lowest record of pair t with that J (include/gpc_hip.h has the rule in
// full).  A record with an end outside the image takes no part.  Every launch is a step of its own; nothing waits
// across workgroups inside a launch, and the only atomics are integer minima, so the result is the same in any order.
//   k_track_fill     the per-pixel planes of pairs 1 .. P-1 to TR_NONE (a minimum needs a start value);
//   k_track_scatter  plane[t][source pixel] = min record index of pair t (t >= 1); pred[t][i] = TR_NONE for every record;
//   k_track_link     record i of pair t looks its target pixel up in plane[t + 1]: the candidate J goes to next[t][i]
//                    and i into pred[t + 1][J] with a minimum;
//   k_track_settle   next[t][i] stays only where pred[t + 1][J] == i; heads (pred[t][i] == TR_NONE) counted per chunk;
//   k_track_scan     exclusive scan of the chunk counts in (pair, chunk) order, the total into *n_tracks;
//   k_track_walk     every head numbers itself (chunk offset + rank), follows its chain of at most P records, writes
//                    the track id along it and its table row.
#pragma once
#include "gpc_device.h"

#define TR_THREADS 256
#define TR_CHUNK (TR_THREADS * 8)  // records per workgroup of the settle and walk kernels
#define TR_NONE 0x7FFFFFFF         // no record: above every index (an index is below cap <= INT_MAX)

namespace gpc {

struct TrRec {  // gpc_correspondence
  int32_t sx, sy, tx, ty;
};
struct TrRow {  // gpc_track
  int32_t first_pair, first_record, length, last_record;
};

// records of pair t the kernels look at: min(counts[t], cap), a negative count read as 0
__device__ __forceinline__ int tr_count(const int32_t* __restrict__ counts, int t, int cap) {
  const int m = counts[t];
  return m < 0 ? 0 : (m > cap ? cap : m);
}

__device__ __forceinline__ bool tr_inside(const TrRec& r, int W, int H) {
  return (uint32_t)r.sx < (uint32_t)W && (uint32_t)r.sy < (uint32_t)H && (uint32_t)r.tx < (uint32_t)W &&
         (uint32_t)r.ty < (uint32_t)H;
}

// n16 16-byte groups of TR_NONE
__global__ __launch_bounds__(TR_THREADS) void k_track_fill(int4* __restrict__ plane, long n16) {
  const int4 v = make_int4(TR_NONE, TR_NONE, TR_NONE, TR_NONE);
  for (long i = (long)blockIdx.x * TR_THREADS + threadIdx.x; i < n16; i += (long)gridDim.x * TR_THREADS) plane[i] = v;
}

// grid (x, P): pair blockIdx.y, records strided over blockIdx.x.  plane[t - 1] belongs to pair t (pair 0 has none).
__global__ __launch_bounds__(TR_THREADS) void k_track_scatter(const TrRec* __restrict__ corr, int cap,
                                                              const int32_t* __restrict__ counts, int W, int H,
                                                              int32_t* __restrict__ plane, int32_t* __restrict__ pred) {
  const int t = blockIdx.y;
  const int m = tr_count(counts, t, cap);
  const TrRec* rec = corr + (long)t * cap;
  int32_t* pr = pred + (long)t * cap;
  int32_t* pl = plane + (long)(t >= 1 ? t - 1 : 0) * W * H;  // (written for t >= 1 only)
  for (int i = blockIdx.x * TR_THREADS + threadIdx.x; i < m; i += gridDim.x * TR_THREADS) {
    const TrRec r = rec[i];
    pr[i] = TR_NONE;
    if (t >= 1 && tr_inside(r, W, H)) atomicMin(&pl[r.sy * W + r.sx], i);
  }
}

// grid (x, P): next[t][i] = the successor candidate of record i (-1: none), pred[t + 1][J] = min over the i that want J
__global__ __launch_bounds__(TR_THREADS) void k_track_link(const TrRec* __restrict__ corr, int cap,
                                                           const int32_t* __restrict__ counts, int W, int H, int P,
                                                           const int32_t* __restrict__ plane, int32_t* __restrict__ pred,
                                                           int32_t* __restrict__ next) {
  const int t = blockIdx.y;
  const int m = tr_count(counts, t, cap);
  const bool last = t + 1 >= P;
  const int m1 = last ? 0 : tr_count(counts, t + 1, cap);
  const TrRec* rec = corr + (long)t * cap;
  const int32_t* pl = plane + (long)t * W * H;  // (pair t + 1's plane; not touched for the last pair)
  int32_t* pr1 = pred + (long)(t + 1) * cap;
  int32_t* nx = next + (long)t * cap;
  for (int i = blockIdx.x * TR_THREADS + threadIdx.x; i < m; i += gridDim.x * TR_THREADS) {
    int J = -1;
    if (!last) {
      const TrRec r = rec[i];
      if (tr_inside(r, W, H)) {
        const int j = pl[r.ty * W + r.tx];
        if ((uint32_t)j < (uint32_t)m1) {
          J = j;
          atomicMin(&pr1[j], i);
        }
      }
    }
    nx[i] = J;
  }
}

// grid (nchunk, P): chunk blockIdx.x of pair blockIdx.y.  A candidate that another record of the pair won is taken back;
// blkcnt[t * nchunk + b] = heads of the chunk.
__global__ __launch_bounds__(TR_THREADS) void k_track_settle(int cap, const int32_t* __restrict__ counts, int P,
                                                             const int32_t* __restrict__ pred, int32_t* __restrict__ next,
                                                             int32_t* __restrict__ blkcnt, int nchunk) {
  const int t = blockIdx.y;
  const int m = tr_count(counts, t, cap);
  const int i0 = blockIdx.x * TR_CHUNK;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int heads = 0;
  if (i0 < m) {
    const int32_t* pr = pred + (long)t * cap;
    const int32_t* pr1 = pred + (long)(t + 1) * cap;  // (read only behind a candidate, which the last pair never has)
    int32_t* nx = next + (long)t * cap;
#pragma unroll 1
    for (int k = 0; k < TR_CHUNK / TR_THREADS; ++k) {
      const int i = i0 + k * TR_THREADS + threadIdx.x;
      if (i < m) {
        const int J = nx[i];
        if (J >= 0 && pr1[J] != i) nx[i] = -1;
        if (pr[i] == TR_NONE) ++heads;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o);
  if ((threadIdx.x & 63) == 0 && heads) atomicAdd(&s_n, heads);
  __syncthreads();
  if (threadIdx.x == 0) blkcnt[(long)t * nchunk + blockIdx.x] = s_n;
}

// one workgroup (of whole waves, at most 1024 threads): exclusive scan of N counts in place, the total into *n_tracks
__device__ __forceinline__ void tr_scan_block(int32_t* __restrict__ blkcnt, long N, int32_t* __restrict__ n_tracks) {
  __shared__ int s_w[16];
  __shared__ int s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (long base = 0; base < N; base += blockDim.x) {
    const long i = base + threadIdx.x;
    const int x = i < N ? blkcnt[i] : 0;
    int incl = x;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    const int carry = s_carry;
    if (i < N) blkcnt[i] = carry + woff + incl - x;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_tracks = s_carry;
}

// one workgroup: exclusive scan of the N chunk counts in place, the total into *n_tracks
__global__ __launch_bounds__(1024) void k_track_scan(int32_t* __restrict__ blkcnt, long N, int32_t* __restrict__ n_tracks) {
  tr_scan_block(blkcnt, N, n_tracks);
}

// grid (nchunk, P): the heads of chunk b of pair t are tracks blkoff[t * nchunk + b] + their rank in record order
__global__ __launch_bounds__(TR_THREADS) void k_track_walk(int cap, const int32_t* __restrict__ counts, int P,
                                                           const int32_t* __restrict__ pred, const int32_t* __restrict__ next,
                                                           const int32_t* __restrict__ blkoff, int nchunk,
                                                           int32_t* __restrict__ track_id, TrRow* __restrict__ tracks,
                                                           int track_cap) {
  const int t = blockIdx.y;
  const int m = tr_count(counts, t, cap);
  const int i0 = blockIdx.x * TR_CHUNK;
  if (i0 >= m) return;  // (uniform over the workgroup)
  const int32_t* pr = pred + (long)t * cap;
  __shared__ int s_w[TR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pos = blkoff[(long)t * nchunk + blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < TR_CHUNK / TR_THREADS; ++k) {
    const int i = i0 + k * TR_THREADS + threadIdx.x;
    const bool head = i < m && pr[i] == TR_NONE;
    const unsigned long long mk = __ballot(head);
    if (lane == 0) s_w[wave] = __popcll(mk);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TR_THREADS / 64; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    if (head) {
      const int id = pos + woff + __popcll(mk & ((1ull << lane) - 1ull));
      int tt = t, ii = i, len = 0;
      for (;;) {  // (a link leads from pair tt to pair tt + 1: at most P - t records)
        track_id[(long)tt * cap + ii] = id;
        ++len;
        if (tt + 1 >= P) break;
        const int nx = next[(long)tt * cap + ii];
        if (nx < 0) break;
        ++tt;
        ii = nx;
      }
      if (id < track_cap) {
        TrRow row;
        row.first_pair = t;
        row.first_record = i;
        row.length = len;
        row.last_record = ii;
        tracks[id] = row;
      }
    }
    pos += tot;
    __syncthreads();
  }
}

}  // namespace gpc
