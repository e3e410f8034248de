// k_score.h -- matches scored against ground truth on the device (gpc_hip_score_*, include/gpc_hip.h).
//
//   k_score_records<CORR>          one streaming pass over a pair's records ([P][cap], count read on the device): every record
//                                  gathers truth (and the ignore byte) at its source pixel and is counted as ignored / without
//                                  truth / judged, and within each threshold;
//   k_score_matchable<FLOW, BITS>  one pass over the left candidate image and the truth planes: the candidates, and those of
//                                  them whose true target is a candidate of the right image (the recall denominator).
//
// Every output is an integer count.  A counter is reduced in the wave (ballot + popcount; the error sum by a wave
// reduction), then across the workgroup's waves through LDS, and leaves the workgroup as ONE 64-bit integer atomic add
// per counter (agent scope: the workgroups of a pair run on several XCDs).  No float atomics: the result does not depend
// on the order in which workgroups arrive.
//
// The error arithmetic is float32 with one rounding per operation; hipcc contracts a * b + c into a fused multiply-add by
// default, which rounds once, so contraction is switched off in the two kernels (the pragma is function-local: the other
// kernels of the translation unit compile as before).
#pragma once
#include "gpc_device.h"

#define SC_THREADS 256
#define SC_PER_THREAD 8
#define SC_CHUNK (SC_THREADS * SC_PER_THREAD)  // records per workgroup and trip of k_score_records
#define SC_MAX_THR 8                           // GPC_SCORE_MAX_THR
#define SC_PX 4                                // pixels per lane of k_score_matchable (one 16-byte load per truth plane)

namespace gpc {

// == gpc_score (include/gpc_hip.h), as the 64-bit words the atomics add into
struct ScoreDev {
  unsigned long long n_records, n_ignored, n_no_truth, n_judged, n_within[SC_MAX_THR], sum_e2_q8, n_candidates, n_matchable;
};
#define SC_WORDS 15            // words of ScoreDev
#define SC_WORD_CANDIDATES 13  // n_candidates, then n_matchable
static_assert(sizeof(ScoreDev) == 8 * SC_WORDS, "gpc_score is fifteen 64-bit counters");

// squared thresholds fl(thr * thr); entries beyond n_thr hold -1 (no e2 is <= -1: those counters stay 0)
struct ScoreThr {
  float t2[SC_MAX_THR];
};

template <bool CORR>
struct ScRec;
template <>
struct ScRec<false> {  // gpc_support
  int32_t x, y;
  float d;
};
template <>
struct ScRec<true> {  // gpc_correspondence
  int32_t sx, sy, tx, ty;
};

// truth the rules can judge: finite and below the .flo "unknown" magnitude (false for NaN and +-inf)
__device__ __forceinline__ bool sc_usable(float t) { return fabsf(t) < 1e9f; }

// sum of v over the wave's 64 lanes (every lane gets it)
__device__ __forceinline__ unsigned long long sc_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// s_part[wave][w] holds every wave's partial sums: thread w < NW adds word w of all waves into dst[w], one atomic each
template <int NW>
__device__ __forceinline__ void sc_flush(unsigned long long (*s_part)[NW], unsigned long long* __restrict__ dst) {
  __syncthreads();
  if (threadIdx.x < NW) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < SC_THREADS / 64; ++w) t += s_part[w][threadIdx.x];
    if (t) __hip_atomic_fetch_add(dst + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (chunks of records, pairs); a workgroup walks the pair's chunks blockIdx.x, blockIdx.x + gridDim.x, ...
// rec [P][cap], counts [P] (true counts: may exceed cap), tu / tv / ign [P][H][W] (tv: CORR only; ign may be null)
template <bool CORR>
__global__ __launch_bounds__(SC_THREADS) void k_score_records(const ScRec<CORR>* __restrict__ rec, long cap,
                                                              const int32_t* __restrict__ counts, int W, int H,
                                                              const float* __restrict__ tu, const float* __restrict__ tv,
                                                              const uint8_t* __restrict__ ign, ScoreThr thr,
                                                              ScoreDev* __restrict__ scores) {
#pragma clang fp contract(off)
  const int p = blockIdx.y;
  const long cnt = counts[p];
  const int n = (int)(cnt < 0 ? 0 : (cnt < cap ? cnt : cap));
  if ((long)blockIdx.x * SC_CHUNK >= n) return;  // (uniform over the workgroup)
  const ScRec<CORR>* r = rec + (long)p * cap;
  const long npx = (long)W * H;
  const float* pu = tu + (long)p * npx;
  const float* pv = CORR ? tv + (long)p * npx : nullptr;
  const uint8_t* pi = ign ? ign + (long)p * npx : nullptr;

  // wave-uniform counters (ballot + popcount), the error sum per lane
  uint32_t c_rec = 0, c_ign = 0, c_not = 0, c_jud = 0, c_in[SC_MAX_THR];
#pragma unroll
  for (int k = 0; k < SC_MAX_THR; ++k) c_in[k] = 0;
  unsigned long long q_sum = 0;

  for (long i0 = (long)blockIdx.x * SC_CHUNK; i0 < n; i0 += (long)gridDim.x * SC_CHUNK) {
#pragma unroll 2
    for (int k = 0; k < SC_PER_THREAD; ++k) {
      const long i = i0 + k * SC_THREADS + threadIdx.x;  // consecutive lanes, consecutive records
      const bool live = i < n;
      bool ignored = false, judged = false;
      float e2 = 0.f;
      if (live) {
        const ScRec<CORR> a = r[i];
        int sx, sy;
        if constexpr (CORR) {
          sx = a.sx;
          sy = a.sy;
        } else {
          sx = a.x;
          sy = a.y;
        }
        if ((unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H) {  // (outside the image: invalid input, counted as no truth)
          const long at = (long)sy * W + sx;
          ignored = pi && pi[at] != 0;
          if (!ignored) {
            const float u = pu[at];
            if constexpr (CORR) {
              const float v = pv[at];
              if (sc_usable(u) && sc_usable(v)) {
                judged = true;
                const float ex = (float)(a.tx - a.sx) - u, ey = (float)(a.ty - a.sy) - v;
                const float xx = ex * ex, yy = ey * ey;
                e2 = xx + yy;
              }
            } else {
              if (sc_usable(u)) {
                judged = true;
                const float ex = a.d - u;
                e2 = ex * ex;
              }
            }
          }
        }
      }
      c_rec += (uint32_t)__popcll(__ballot(live));
      c_ign += (uint32_t)__popcll(__ballot(ignored));
      c_jud += (uint32_t)__popcll(__ballot(judged));
      c_not += (uint32_t)__popcll(__ballot(live && !ignored && !judged));
#pragma unroll
      for (int t = 0; t < SC_MAX_THR; ++t) c_in[t] += (uint32_t)__popcll(__ballot(judged && e2 <= thr.t2[t]));
      if (judged) {
        const float m = fminf(e2, 1048576.f);  // (fminf: an e2 that is NaN or +inf gives the clamp, as include/gpc_hip.h says)
        const float s = m * 256.f;
        q_sum += (uint32_t)(s + 0.5f);  // (at most 2^28: the 32-bit conversion gives what the 64-bit one would)
      }
    }
  }

  constexpr int NW = SC_WORD_CANDIDATES;  // n_records .. sum_e2_q8: the first 13 words of ScoreDev
  __shared__ unsigned long long s_part[SC_THREADS / 64][NW];
  const unsigned long long q_wave = sc_wave_sum(q_sum);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_part[wave][0] = c_rec;
    s_part[wave][1] = c_ign;
    s_part[wave][2] = c_not;
    s_part[wave][3] = c_jud;
#pragma unroll
    for (int t = 0; t < SC_MAX_THR; ++t) s_part[wave][4 + t] = c_in[t];
    s_part[wave][4 + SC_MAX_THR] = q_wave;
  }
  sc_flush<NW>(s_part, reinterpret_cast<unsigned long long*>(scores + p));
}

// is pixel `at` of a gradient image set?  BITS: k_preprocess's bit image (byte at / 8, bit at % 8), else its byte image
template <bool BITS>
__device__ __forceinline__ bool sc_grad(const uint8_t* __restrict__ g, long at) {
  return BITS ? ((g[at >> 3] >> (at & 7)) & 1u) != 0u : g[at] != 0;
}

// grid (blocks over the pixel groups of the candidate rows, pairs).  grad: the gradient images the pipeline left, image
// p * lstride is the pair's left image, the next one its right image (lstride 2: batches, 1: frame sequences).
// tu / tv / ign as above.  W % 16 == 0: a lane's SC_PX pixels share a row, and the bit image's bytes do not straddle rows.
template <bool FLOW, bool BITS>
__global__ __launch_bounds__(SC_THREADS) void k_score_matchable(const uint8_t* __restrict__ grad, int lstride, int W, int H,
                                                                GpcDivW dw, const float* __restrict__ tu,
                                                                const float* __restrict__ tv, const uint8_t* __restrict__ ign,
                                                                ScoreDev* __restrict__ scores) {
#pragma clang fp contract(off)
  const int p = blockIdx.y;
  const long npx = (long)W * H;
  const long gimg = BITS ? npx / 8 : npx;
  const uint8_t* gl = grad + (long)p * lstride * gimg;
  const uint8_t* gr = gl + gimg;
  const float* pu = tu + (long)p * npx;
  const float* pv = FLOW ? tv + (long)p * npx : nullptr;
  const uint8_t* pi = ign ? ign + (long)p * npx : nullptr;
  // the candidate rows GPC_R .. H - GPC_R - 1 only, as groups of SC_PX pixels
  const uint32_t first = (uint32_t)(GPC_R * W) / SC_PX, last = (uint32_t)((H - GPC_R) * W) / SC_PX;
  uint32_t n_cand = 0, n_match = 0;
  for (uint32_t q = first + blockIdx.x * SC_THREADS + threadIdx.x; q < last; q += gridDim.x * SC_THREADS) {
    const uint32_t at = q * SC_PX;
    const int y = divw(at, dw), x0 = (int)at - y * W;
    uint32_t gm;  // this lane's four gradient flags
    if (BITS) {
      gm = ((uint32_t)gl[at >> 3] >> (at & 4u)) & 0xFu;
    } else {
      const uint32_t w4 = *reinterpret_cast<const uint32_t*>(gl + at);
      gm = (w4 & 0xFFu ? 1u : 0u) | (w4 & 0xFF00u ? 2u : 0u) | (w4 & 0xFF0000u ? 4u : 0u) | (w4 & 0xFF000000u ? 8u : 0u);
    }
#pragma unroll
    for (int j = 0; j < SC_PX; ++j)
      if (x0 + j < GPC_R || x0 + j >= W - GPC_R) gm &= ~(1u << j);
    n_cand += __popc(gm);
    if (!gm) continue;
    const float4 u4 = *reinterpret_cast<const float4*>(pu + at);
    float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (FLOW) v4 = *reinterpret_cast<const float4*>(pv + at);
    const uint32_t i4 = pi ? *reinterpret_cast<const uint32_t*>(pi + at) : 0u;
    const float uu[SC_PX] = {u4.x, u4.y, u4.z, u4.w}, vv[SC_PX] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < SC_PX; ++j) {
      if (!((gm >> j) & 1u) || ((i4 >> (8 * j)) & 0xFFu)) continue;
      if (!sc_usable(uu[j]) || (FLOW && !sc_usable(vv[j]))) continue;
      // R = roundf (half away from zero); |truth| < 1e9 fits an int
      const int tx = FLOW ? x0 + j + (int)roundf(uu[j]) : x0 + j - (int)roundf(uu[j]);
      const int ty = FLOW ? y + (int)roundf(vv[j]) : y;
      if (tx < GPC_R || tx >= W - GPC_R || ty < GPC_R || ty >= H - GPC_R) continue;
      if (sc_grad<BITS>(gr, (long)ty * W + tx)) ++n_match;
    }
  }
  constexpr int NW = 2;
  __shared__ unsigned long long s_part[SC_THREADS / 64][NW];
  const unsigned long long a = sc_wave_sum(n_cand), b = sc_wave_sum(n_match);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_part[wave][0] = a;
    s_part[wave][1] = b;
  }
  sc_flush<NW>(s_part, reinterpret_cast<unsigned long long*>(scores + p) + SC_WORD_CANDIDATES);
}

}  // namespace gpc
