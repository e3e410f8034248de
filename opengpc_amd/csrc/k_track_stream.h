// k_track_stream.h -- point tracks over a video that arrives in pushes (gpc_hip_track_stream_*): the six steps of
// k_track.h over the WINDOW of a push, [the carried pair (the last pair of the push before, if any), the k new pairs].
// Window pair w is the carried pair for w < c (c = 0 | 1) and new pair w - c otherwise.  The carried pair's records, its
// count and its track ids live in the stream (crec, cm, cid); the new pairs' in the caller's arrays, [k][cap].
//   k_trs_fill     the per-pixel planes of the k new pairs to TR_NONE;
//   k_trs_scatter  plane[j][source pixel] = min record index of new pair j; pred[j][i] = TR_NONE (the carried pair is
//                 nobody's successor: it has neither a plane nor a pred);
//   k_trs_link     record i of window pair w looks its target pixel up in the plane of window pair w + 1;
//   k_trs_settle   next[w][i] stays only where pred of the successor agrees; heads counted per chunk of the NEW pairs;
//   k_trs_scan     exclusive scan of the chunk counts that starts from the total so far (*total) and leaves the new total
//                 there: one workgroup reads and writes the word, no host read;
//   k_trs_walk     heads of the new pairs number themselves and write their row with the GLOBAL pair index; carried records
//                 with a successor walk on with their carried id and then update length and last_record of their row (one
//                 writer per row in both cases: a carried id is below the old total, a new head's is not, and a track
//                 has one record per pair).  The pass also writes prev[j][i] = pred[j][i], -1 for TR_NONE;
//   k_trs_save     the last new pair's records, count and ids into the carry.
// As in k_track.h nothing waits across workgroups and the only atomics are integer minima.
#pragma once
#include "k_track.h"

namespace gpc {

// records of window pair w the kernels look at (cm[0] is stored clamped)
__device__ __forceinline__ int trs_count(const int32_t* __restrict__ cm, const int32_t* __restrict__ counts, int w, int c, int cap) {
  return w < c ? cm[0] : tr_count(counts, w - c, cap);
}

// n16 16-byte groups of TR_NONE (k_track_fill under a name of its own, so that a stream's fill is told from the offline one)
__global__ __launch_bounds__(TR_THREADS) void k_trs_fill(int4* __restrict__ plane, long n16) {
  const int4 v = make_int4(TR_NONE, TR_NONE, TR_NONE, TR_NONE);
  for (long i = (long)blockIdx.x * TR_THREADS + threadIdx.x; i < n16; i += (long)gridDim.x * TR_THREADS) plane[i] = v;
}

// grid (x, k): new pair blockIdx.y
__global__ __launch_bounds__(TR_THREADS) void k_trs_scatter(const TrRec* __restrict__ corr, int cap,
                                                           const int32_t* __restrict__ counts, int W, int H,
                                                           int32_t* __restrict__ plane, int32_t* __restrict__ pred) {
  const int j = blockIdx.y;
  const int m = tr_count(counts, j, cap);
  const TrRec* rec = corr + (long)j * cap;
  int32_t* pr = pred + (long)j * cap;
  int32_t* pl = plane + (long)j * W * H;
  for (int i = blockIdx.x * TR_THREADS + threadIdx.x; i < m; i += gridDim.x * TR_THREADS) {
    const TrRec r = rec[i];
    pr[i] = TR_NONE;
    if (tr_inside(r, W, H)) atomicMin(&pl[r.sy * W + r.sx], i);
  }
}

// grid (x, c + k): window pair blockIdx.y.  next is [c + k][cap] (window), plane and pred [k][cap] (new pairs)
__global__ __launch_bounds__(TR_THREADS) void k_trs_link(const TrRec* __restrict__ crec, const int32_t* __restrict__ cm, int c,
                                                        const TrRec* __restrict__ corr, int cap,
                                                        const int32_t* __restrict__ counts, int W, int H, int k,
                                                        const int32_t* __restrict__ plane, int32_t* __restrict__ pred,
                                                        int32_t* __restrict__ next) {
  const int w = blockIdx.y;
  const int m = trs_count(cm, counts, w, c, cap);
  const int j1 = w + 1 - c;  // the successor pair among the new ones
  const bool last = j1 >= k;
  const int m1 = last ? 0 : tr_count(counts, j1, cap);
  const TrRec* rec = w < c ? crec : corr + (long)(w - c) * cap;
  const int32_t* pl = plane + (long)(last ? 0 : j1) * W * H;
  int32_t* pr1 = pred + (long)(last ? 0 : j1) * cap;
  int32_t* nx = next + (long)w * cap;
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

// grid (nchunk, c + k): chunk blockIdx.x of window pair blockIdx.y; blkcnt[(w - c) * nchunk + b] = heads of a new pair's chunk
__global__ __launch_bounds__(TR_THREADS) void k_trs_settle(const int32_t* __restrict__ cm, int c, int cap,
                                                          const int32_t* __restrict__ counts, int k,
                                                          const int32_t* __restrict__ pred, int32_t* __restrict__ next,
                                                          int32_t* __restrict__ blkcnt, int nchunk) {
  const int w = blockIdx.y;
  const int m = trs_count(cm, counts, w, c, cap);
  const int i0 = blockIdx.x * TR_CHUNK;
  const int j1 = w + 1 - c;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int heads = 0;
  if (i0 < m) {
    const int32_t* pr = pred + (long)(w < c ? 0 : w - c) * cap;   // (read for the new pairs only)
    const int32_t* pr1 = pred + (long)(j1 < k ? j1 : 0) * cap;    // (read only behind a candidate, which the last pair never has)
    int32_t* nx = next + (long)w * cap;
#pragma unroll 1
    for (int q = 0; q < TR_CHUNK / TR_THREADS; ++q) {
      const int i = i0 + q * TR_THREADS + threadIdx.x;
      if (i < m) {
        const int J = nx[i];
        if (J >= 0 && pr1[J] != i) nx[i] = -1;
        if (w >= c && pr[i] == TR_NONE) ++heads;
      }
    }
  }
  if (w < c) return;  // (uniform over the workgroup; the barrier below is then met by nobody)
  for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o);
  if ((threadIdx.x & 63) == 0 && heads) atomicAdd(&s_n, heads);
  __syncthreads();
  if (threadIdx.x == 0) blkcnt[(long)(w - c) * nchunk + blockIdx.x] = s_n;
}

// one workgroup: exclusive scan of the N chunk counts in place, starting from *total; the new total back into *total
__global__ __launch_bounds__(1024) void k_trs_scan(int32_t* __restrict__ blkcnt, long N, int32_t* __restrict__ total) {
  __shared__ int s_w[16];
  __shared__ int s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (threadIdx.x == 0) s_carry = *total;
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
  if (threadIdx.x == 0) *total = s_carry;
}

// grid (nchunk, c + k).  pair0: the global index of new pair 0.  track_id and prev are the caller's [k][cap].
__global__ __launch_bounds__(TR_THREADS) void k_trs_walk(const int32_t* __restrict__ cm, const int32_t* __restrict__ cid, int c,
                                                        int cap, const int32_t* __restrict__ counts, int k,
                                                        const int32_t* __restrict__ pred, const int32_t* __restrict__ next,
                                                        const int32_t* __restrict__ blkoff, int nchunk, int pair0,
                                                        int32_t* __restrict__ track_id, int32_t* __restrict__ prev,
                                                        TrRow* __restrict__ tracks, int track_cap) {
  const int w = blockIdx.y;
  const int m = trs_count(cm, counts, w, c, cap);
  const int i0 = blockIdx.x * TR_CHUNK;
  if (i0 >= m) return;  // (uniform over the workgroup)
  const int P = c + k;
  if (w < c) {
    // carried records with a successor: the chain goes on under the carried id
#pragma unroll 1
    for (int q = 0; q < TR_CHUNK / TR_THREADS; ++q) {
      const int i = i0 + q * TR_THREADS + threadIdx.x;
      if (i >= m) continue;
      int ii = next[i];
      if (ii < 0) continue;
      const int id = cid[i];
      int tt = 1, len = 0;
      for (;;) {
        track_id[(long)(tt - c) * cap + ii] = id;
        ++len;
        if (tt + 1 >= P) break;
        const int nx = next[(long)tt * cap + ii];
        if (nx < 0) break;
        ++tt;
        ii = nx;
      }
      if (id < track_cap) {
        tracks[id].length += len;
        tracks[id].last_record = ii;
      }
    }
    return;
  }
  const int j = w - c;
  const int32_t* pr = pred + (long)j * cap;
  int32_t* pv = prev + (long)j * cap;
  __shared__ int s_w[TR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pos = blkoff[(long)j * nchunk + blockIdx.x];
#pragma unroll 1
  for (int q = 0; q < TR_CHUNK / TR_THREADS; ++q) {
    const int i = i0 + q * TR_THREADS + threadIdx.x;
    const int p = i < m ? pr[i] : 0;
    const bool head = i < m && p == TR_NONE;
    if (i < m) pv[i] = head ? -1 : p;
    const unsigned long long mk = __ballot(head);
    if (lane == 0) s_w[wave] = __popcll(mk);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int v = 0; v < TR_THREADS / 64; ++v) {
      if (v < wave) woff += s_w[v];
      tot += s_w[v];
    }
    if (head) {
      const int id = pos + woff + __popcll(mk & ((1ull << lane) - 1ull));
      int tt = w, ii = i, len = 0;
      for (;;) {
        track_id[(long)(tt - c) * cap + ii] = id;
        ++len;
        if (tt + 1 >= P) break;
        const int nx = next[(long)tt * cap + ii];
        if (nx < 0) break;
        ++tt;
        ii = nx;
      }
      if (id < track_cap) {
        TrRow row;
        row.first_pair = pair0 + j;
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

// the candidate count of each of a push's nframes frames, out of their statistics words (k_seq_stats does this for a
// whole sequence; here frame 0 of the layout may be the carried one, which the push before has reported)
__global__ void k_trs_ncand(const int32_t* __restrict__ fstats, int32_t* __restrict__ ncand, int nframes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nframes) ncand[i] = fstats[i * GPC_STAT_STRIDE + GPC_STAT_NCAND];
}

// the carry of the next push: records, ids and the (clamped) count of the last new pair (corr, track_id, counts point at it)
__global__ __launch_bounds__(TR_THREADS) void k_trs_save(const TrRec* __restrict__ corr, const int32_t* __restrict__ track_id,
                                                        const int32_t* __restrict__ counts, int cap, TrRec* __restrict__ crec,
                                                        int32_t* __restrict__ cid, int32_t* __restrict__ cm) {
  const int m = tr_count(counts, 0, cap);
  for (int i = blockIdx.x * TR_THREADS + threadIdx.x; i < m; i += gridDim.x * TR_THREADS) {
    crec[i] = corr[i];
    cid[i] = track_id[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) cm[0] = m;
}

}  // namespace gpc
