// k_union.h -- the union of the groups' results in group mode (gpc_hip_set_forest_groups).
//
// The joins run over VIRTUAL pairs: group g of pair p is virtual pair v = p * G + g, whose records (at most one per left
// pixel under the sort matcher) lie in vout[v][0 .. min(vcnt[v], vcap)).  The union of pair p is group 0's records in
// their order, then group 1's records that no earlier group emitted, and so on; supports are compared by (x, y, d),
// correspondences by (src_x, src_y, tar_x, tar_y).  Because a group has at most one record per left pixel, "an earlier
// group emitted it" is a lookup in per-pixel planes: plane[v][y * W + x] = the record's key (the bits of d, or the target
// pixel's index), all ones where group g has no record (the host fills the planes with 0xFF first).
//   k_group_union_scatter  the planes of every virtual pair;
//   k_group_union_count    keep flags of a chunk of UN_CHUNK records -> the chunk's count;
//   k_group_union_scan     per pair, group-major exclusive scan of the chunk counts; the pair's true total and candidates;
//   k_group_union          the keep flags again, ballot-scanned in record order, and the kept records stored at their place.
#pragma once
#include "gpc_device.h"

#define UN_THREADS 256
#define UN_CHUNK (UN_THREADS * 8)  // records per workgroup of the count and compaction kernels

namespace gpc {

template <bool CORR>
struct UnRec;
template <>
struct UnRec<false> {  // gpc_support
  int32_t x, y;
  float d;
};
template <>
struct UnRec<true> {  // gpc_correspondence
  int32_t sx, sy, tx, ty;
};

template <bool CORR>
__device__ __forceinline__ void un_key(const UnRec<CORR>& r, int W, uint32_t& pix, uint32_t& key);
template <>
__device__ __forceinline__ void un_key<false>(const UnRec<false>& r, int W, uint32_t& pix, uint32_t& key) {
  pix = (uint32_t)(r.y * W + r.x);
  key = __float_as_uint(r.d);
}
template <>
__device__ __forceinline__ void un_key<true>(const UnRec<true>& r, int W, uint32_t& pix, uint32_t& key) {
  pix = (uint32_t)(r.sy * W + r.sx);
  key = (uint32_t)(r.ty * W + r.tx);
}

// grid (x, npv): virtual pair blockIdx.y, records strided over blockIdx.x
template <bool CORR>
__global__ __launch_bounds__(UN_THREADS) void k_group_union_scatter(const UnRec<CORR>* __restrict__ vout,
                                                                    const int32_t* __restrict__ vcnt, long vcap, int W, int H,
                                                                    uint32_t* __restrict__ plane, int G) {
  const int v = blockIdx.y;
  if (v % G == G - 1) return;  // (no later group reads the last group's plane)
  const int n = (int)min((long)vcnt[v], vcap);
  const UnRec<CORR>* rec = vout + (long)v * vcap;
  uint32_t* pl = plane + (long)v * W * H;
  for (int i = blockIdx.x * UN_THREADS + threadIdx.x; i < n; i += gridDim.x * UN_THREADS) {
    uint32_t pix, key;
    un_key<CORR>(rec[i], W, pix, key);
    if (pix < (uint32_t)(W * H)) pl[pix] = key;
  }
}

// is record i of virtual pair v = p * G + g new (no group before g emitted it)?
template <bool CORR>
__device__ __forceinline__ bool un_keep(const UnRec<CORR>& r, int W, int H, const uint32_t* __restrict__ plane, int p, int g,
                                        int G) {
  uint32_t pix, key;
  un_key<CORR>(r, W, pix, key);
  if (pix >= (uint32_t)(W * H)) return true;
  bool keep = true;
  for (int h = 0; h < g; ++h) keep = keep && plane[(long)(p * G + h) * W * H + pix] != key;
  return keep;
}

// grid (nchunk, npv): blkcnt[v * nchunk + b] = records kept in chunk b of virtual pair v
template <bool CORR>
__global__ __launch_bounds__(UN_THREADS) void k_group_union_count(const UnRec<CORR>* __restrict__ vout,
                                                                  const int32_t* __restrict__ vcnt, long vcap, int W, int H,
                                                                  const uint32_t* __restrict__ plane, int G,
                                                                  int32_t* __restrict__ blkcnt, int nchunk) {
  const int v = blockIdx.y, p = v / G, g = v - p * G;
  const int n = (int)min((long)vcnt[v], vcap);
  const int i0 = blockIdx.x * UN_CHUNK;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int kept = 0;
  if (i0 < n) {
    const UnRec<CORR>* rec = vout + (long)v * vcap;
#pragma unroll 1
    for (int k = 0; k < UN_CHUNK / UN_THREADS; ++k) {
      const int i = i0 + k * UN_THREADS + threadIdx.x;
      if (i < n && (g == 0 || un_keep<CORR>(rec[i], W, H, plane, p, g, G))) ++kept;
    }
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&s_n, kept);
  __syncthreads();
  if (threadIdx.x == 0) blkcnt[(long)v * nchunk + blockIdx.x] = s_n;
}

// one workgroup per pair: exclusive scan of its G * nchunk chunk counts in group-major order (in place), the true total
// into counts[p], the candidate counts (group 0's virtual images: every group has the same) into ncand[2p], ncand[2p+1]
__global__ __launch_bounds__(1024) void k_group_union_scan(int32_t* __restrict__ blkcnt, int nchunk, int G,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ ncand,
                                                           const int32_t* __restrict__ vstats) {
  const int p = blockIdx.x;
  const long N = (long)G * nchunk;
  int32_t* a = blkcnt + (long)p * N;
  __shared__ int s_w[16];
  __shared__ int s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (long base = 0; base < N; base += blockDim.x) {
    const long i = base + threadIdx.x;
    const int x = i < N ? a[i] : 0;
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
    if (i < N) a[i] = carry + woff + incl - x;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[p] = s_carry;
    if (ncand) {
      const int v0 = p * G * 2;
      ncand[2 * p + 0] = vstats[(v0 + 0) * GPC_STAT_STRIDE + GPC_STAT_NCAND];
      ncand[2 * p + 1] = vstats[(v0 + 1) * GPC_STAT_STRIDE + GPC_STAT_NCAND];
    }
  }
}

// grid (nchunk, npv): the kept records of chunk b of virtual pair v go to out[p][blkoff + their rank], those below cap
template <bool CORR>
__global__ __launch_bounds__(UN_THREADS) void k_group_union(const UnRec<CORR>* __restrict__ vout, const int32_t* __restrict__ vcnt,
                                                            long vcap, int W, int H, const uint32_t* __restrict__ plane, int G,
                                                            const int32_t* __restrict__ blkoff, int nchunk,
                                                            UnRec<CORR>* __restrict__ out, long cap) {
  const int v = blockIdx.y, p = v / G, g = v - p * G;
  const int n = (int)min((long)vcnt[v], vcap);
  const int i0 = blockIdx.x * UN_CHUNK;
  if (i0 >= n) return;  // (uniform over the workgroup)
  const UnRec<CORR>* rec = vout + (long)v * vcap;
  UnRec<CORR>* o = out + (long)p * cap;
  __shared__ int s_w[UN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pos = blkoff[(long)v * nchunk + blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < UN_CHUNK / UN_THREADS; ++k) {
    const int i = i0 + k * UN_THREADS + threadIdx.x;
    UnRec<CORR> r;
    bool keep = false;
    if (i < n) {
      r = rec[i];
      keep = g == 0 || un_keep<CORR>(r, W, H, plane, p, g, G);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < UN_THREADS / 64; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    const long at = (long)pos + woff + rank;
    if (keep && at < cap) o[at] = r;
    pos += tot;
    __syncthreads();
  }
}

}  // namespace gpc
