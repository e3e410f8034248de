// k_inpaint.h -- completing a cleaned dense field, guided by the image (gpc_hip_inpaint_*): a hole takes the weighted mean of
// the valued pixels in its window, a neighbour's weight halving with its grey-level distance in the guide; passes, each a
// function of the one before.  include/gpc_hip.h has the rule in full; it is made of integers only.
//   k_inpaint_begin  one workgroup per 32x32 tile: the field copied to out (a hole gets GPC_DENSE_NONE in every channel), the
//                    pass plane started (0 valued, 255 hole), the tile's hole count, the pair's holes into the stats;
//   k_inpaint_pass   one launch per pass k, in place in out, one workgroup per tile.  The pass plane is the version stamp:
//                    a pixel is a source iff its pass byte is below k.  Whatever another workgroup fills during this launch
//                    reads as 255 or as k and is ignored either way, so nobody waits for anybody and there is no second
//                    buffer.  A tile without holes leaves after one read of its count, a launch whose predecessor filled
//                    nothing after one read of that pass's count (a device word; the host never reads it).  Otherwise the
//                    tile and a halo of r are staged in LDS -- values, guide byte, source and hole flags -- the tile's holes
//                    are compacted into a list by ballot, and the (2 r + 1)^2 loop runs over the list with full waves: the
//                    weight sum in 32 bits, the value sums in 64, one 64-bit division per filled pixel and channel.
#pragma once
#include "gpc_device.h"
#include "inpaint_host.h"

#define IP_THREADS 256
#define IP_NONE ((int32_t)0x80000000)  // GPC_DENSE_NONE
#define IP_EMAX (IP_TILE + 2 * IP_MAX_RADIUS)
#define IP_SRC 256u   // staged flags beside the guide byte: the pixel is a source of this pass
#define IP_HOLE 512u  //   the pixel lies in the image and is a hole of this pass

namespace gpc {

// sgn(S) * ((2 |S| + Wt) div (2 Wt)); |S| < 2^49, 1 <= Wt < 2^18
__device__ __forceinline__ int32_t ip_mean_dev(int64_t S, uint32_t Wt) {
  const uint64_t a = S < 0 ? (uint64_t)0 - (uint64_t)S : (uint64_t)S, q = (2 * a + Wt) / (uint64_t)(2 * Wt);
  return (int32_t)(S < 0 ? -(int64_t)q : (int64_t)q);
}

__device__ __forceinline__ int ip_tile_index() { return (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x); }

// grid (tiles in x, tiles in y, P).  out may be field: a lane reads its pixel before it writes it, and no other lane touches it.
template <int C>
__global__ __launch_bounds__(IP_THREADS) void k_inpaint_begin(const int32_t* field, int W, int H, int32_t* out, uint8_t* pass,
                                                              int32_t* __restrict__ tile_holes, int32_t* __restrict__ stats) {
  __shared__ int32_t s_n;
  const int tid = threadIdx.x;
  const size_t npix = (size_t)W * (size_t)H, pair = (size_t)blockIdx.z * npix;
  const int32_t* F = field + pair * C;
  int32_t* O = out + pair * C;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const int x = blockIdx.x * IP_TILE + (tid & 31);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = blockIdx.y * IP_TILE + (tid >> 5) + 8 * k;
    bool hole = false;
    if (x < W && y < H) {
      const size_t at = (size_t)y * (size_t)W + (size_t)x;
      const int32_t f0 = F[at];
      hole = f0 == IP_NONE;
      O[at] = f0;
      if (C == 2) O[npix + at] = hole ? IP_NONE : F[npix + at];
      pass[pair + at] = hole ? (uint8_t)255 : (uint8_t)0;
    }
    const unsigned long long b = __ballot(hole);
    if ((tid & 63) == 0 && b) atomicAdd(&s_n, __popcll(b));
  }
  __syncthreads();
  if (tid == 0) {
    tile_holes[ip_tile_index()] = s_n;
    if (s_n) atomicAdd(&stats[(size_t)blockIdx.z * 2 + 1], s_n);
  }
}

// grid (tiles in x, tiles in y, P): pass k (1 .. 254) over out and the pass plane, in place.  filled[k] counts what the
// launch fills; stats[t] = {filled, holes left} of pair t.
template <int C>
__global__ __launch_bounds__(IP_THREADS) void k_inpaint_pass(int32_t* out, uint8_t* pass, const uint8_t* __restrict__ guide, int W,
                                                             int H, int r, int shift, int minw, int k, int32_t* tile_holes,
                                                             int32_t* filled, int32_t* stats) {
  __shared__ int32_t s_v[C][IP_EMAX * IP_EMAX];
  __shared__ uint16_t s_gk[IP_EMAX * IP_EMAX];  // guide byte | IP_SRC | IP_HOLE; 0 outside the image
  __shared__ uint16_t s_list[IP_TILE * IP_TILE];
  __shared__ int32_t s_cnt[2];  // holes listed, pixels filled
  if (k > 1 && filled[k - 1] == 0) return;  // (the same word for every lane of the launch)
  const int tile = ip_tile_index();
  if (tile_holes[tile] == 0) return;
  const int tid = threadIdx.x, E = IP_TILE + 2 * r;
  const size_t npix = (size_t)W * (size_t)H, pair = (size_t)blockIdx.z * npix;
  int32_t* O = out + pair * C;
  uint8_t* Pz = pass + pair;
  const uint8_t* G = guide + pair;
  if (tid < 2) s_cnt[tid] = 0;
  for (int i = tid; i < E * E; i += IP_THREADS) {
    const int ly = i / E, lx = i - ly * E;
    const int gx = blockIdx.x * IP_TILE - r + lx, gy = blockIdx.y * IP_TILE - r + ly;
    uint32_t gk = 0;
    int32_t f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t at = (size_t)gy * (size_t)W + (size_t)gx;
      const int pz = Pz[at];
      gk = G[at];
      if (pz < k) {
        gk |= IP_SRC;
#pragma unroll
        for (int c = 0; c < C; ++c) f[c] = O[(size_t)c * npix + at];
      } else {
        gk |= IP_HOLE;
      }
    }
    s_gk[i] = (uint16_t)gk;
#pragma unroll
    for (int c = 0; c < C; ++c) s_v[c][i] = f[c];
  }
  __syncthreads();
  // the tile's holes, compacted (their order does not matter)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int centre = ((tid >> 5) + 8 * q + r) * E + (tid & 31) + r;
    const bool hole = (s_gk[centre] & IP_HOLE) != 0;
    const unsigned long long b = __ballot(hole);
    int base = 0;
    if ((tid & 63) == 0 && b) base = atomicAdd(&s_cnt[0], __popcll(b));
    base = __shfl(base, 0);
    if (hole) s_list[base + __popcll(b & lanemask_lt())] = (uint16_t)centre;
  }
  __syncthreads();
  const int n = s_cnt[0];
  for (int i = tid; i < n; i += IP_THREADS) {
    const int centre = s_list[i];
    const int g0 = s_gk[centre] & 255;
    uint32_t Wt = 0;
    int64_t S[C];
#pragma unroll
    for (int c = 0; c < C; ++c) S[c] = 0;
    for (int dy = -r; dy <= r; ++dy) {
      const int row = centre + dy * E;
      for (int dx = -r; dx <= r; ++dx) {
        const uint32_t gk = s_gk[row + dx];
        const int d = g0 - (int)(gk & 255u), s = (d < 0 ? -d : d) >> shift;
        const uint32_t w = (gk & IP_SRC) >> (s < 8 ? s : 8);  // 0 where the pixel is no source
        Wt += w;
#pragma unroll
        for (int c = 0; c < C; ++c) S[c] += (int64_t)w * (int64_t)s_v[c][row + dx];
      }
    }
    if (Wt >= (uint32_t)minw) {
      const int ly = centre / E, lx = centre - ly * E;
      const size_t at = (size_t)(blockIdx.y * IP_TILE - r + ly) * (size_t)W + (size_t)(blockIdx.x * IP_TILE - r + lx);
#pragma unroll
      for (int c = 0; c < C; ++c) O[(size_t)c * npix + at] = ip_mean_dev(S[c], Wt);
      Pz[at] = (uint8_t)k;
      atomicAdd(&s_cnt[1], 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int f = s_cnt[1];
    if (f) {
      tile_holes[tile] = n - f;
      atomicAdd(&filled[k], f);
      atomicAdd(&stats[(size_t)blockIdx.z * 2], f);
      atomicSub(&stats[(size_t)blockIdx.z * 2 + 1], f);
    }
  }
}

}  // namespace gpc
