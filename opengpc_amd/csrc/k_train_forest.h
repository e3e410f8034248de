// k_train_forest.h -- a whole FOREST trained over one resident training set (gpc_hip_train_forest).
//
// The reference trains every fern on a bootstrap of the set: sampleFraction * N triplets drawn with replacement and
// COPIED (training.hpp:113-121).  Copies of one triplet agree in every byte and, because marks are only ever derived from
// the bytes, in every mark; so a bootstrap is the set itself with a multiplicity per triplet, and the counts of
// Fern::evalSplit over the copies are sums of multiplicities.  Per fern f of a group of G ferns the device holds
//   flags[f][np]  the TSF_* bits of k_train.h (the set's own flags are neither read nor written),
//   mult[f][np]   how often the fern drew the triplet, one byte; 0 for triplets it did not draw and for padding,
//   lim[f]        one past the last triplet with a multiplicity, rounded up to the 4 triplets of a lane: the reference
//                 draws from the first sampleFraction * N triplets only, so the rest of the set is not even read.
// All ferns of the group advance level by level in the same launches; blockIdx.y runs over (fern, candidate) in the
// evaluation and over the ferns elsewhere.  Counts are exact integers: a fern's counts sum to at most its number of draws,
// an int.
#pragma once
#include "k_train.h"

namespace gpc {

// start of every fern of the group: no level committed, all marks cleared.  grid (np / 256, G)
__global__ __launch_bounds__(TS_THREADS) void k_tf_begin(uint8_t* __restrict__ flags, int n, long np) {
  const long t = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  if (t >= np) return;
  flags[(long)blockIdx.y * np + t] = (uint8_t)(t >= n ? (TSF_PAD | TSF_POS | TSF_NEG | TSF_EQ) : TSF_EQ);
}

// ---- candidates of ONE level of every fern: tp / fp per (fern, candidate, tau), weighted by the multiplicities.
// blockIdx.y = fern * ncand + candidate; blockIdx.x = chunk of iters * 1024 triplets, as in k_ts_eval_level.
// cand: the group's hyperplanes of this level, fern f's at cand[f * cand_stride + k].  tp[(f * ncand + k) * ntau + q]
// and fp[...] must be zero on entry.
// A lane sums its own weighted counts over the whole chunk (at most 64 * 4 * 255) and the wave adds them up once at the
// end; only the edges of the tau path go to the LDS difference arrays as they come, +-multiplicity instead of +-1.  A
// triplet of multiplicity 0 counts nothing and issues no atomic, like a padding entry.
__global__ __launch_bounds__(TS_THREADS) void k_tf_eval(const uint8_t* __restrict__ planes, const uint8_t* __restrict__ flags,
                                                        const uint8_t* __restrict__ mult, const int32_t* __restrict__ lim,
                                                        long np, const GpcSplit* __restrict__ cand, int cand_stride,
                                                        int ncand, int taulo, int ntau, int iters,
                                                        int32_t* __restrict__ tp, int32_t* __restrict__ fp) {
  __shared__ int s_tp[TS_MAXTAU], s_fp[TS_MAXTAU];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < TS_MAXTAU) { s_tp[tid] = 0; s_fp[tid] = 0; }
  __syncthreads();
  const int fern = blockIdx.y / ncand;
  const GpcSplit cd = cand[(long)fern * cand_stride + (blockIdx.y - fern * ncand)];
  const uint8_t* ri = planes + (long)cd.i * np;
  const uint8_t* rj = planes + (long)cd.j * np;
  const uint8_t* pi = ri + (long)TS_PATCH * np;
  const uint8_t* pj = rj + (long)TS_PATCH * np;
  const uint8_t* ni = pi + (long)TS_PATCH * np;
  const uint8_t* nj = pj + (long)TS_PATCH * np;
  const uint8_t* fl_f = flags + (long)fern * np;
  const uint8_t* mu_f = mult + (long)fern * np;
  const long end = lim[fern];                          // a multiple of 4, <= np
  const long c0 = (long)blockIdx.x * iters * TS_ITER;  // a workgroup owns `iters` x 1024 consecutive triplets
  const long left = (end - c0 + TS_ITER - 1) / TS_ITER;  // iterations up to the fern's last drawn triplet
  const int my_iters = left <= 0 ? 0 : (left < iters ? (int)left : iters);
  int acc_tp = 0, acc_fp = 0;  // this lane's weighted counts at the first intercept
#pragma unroll 1
  for (int it = 0; it < my_iters; ++it) {
    const long t = c0 + ((long)it * TS_THREADS + tid) * 4;  // 4 triplets per lane
    uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, d0 = 0, d1 = 0, fl = 0x03030303u, mw = 0;
    if (t < end) {
      a0 = *reinterpret_cast<const uint32_t*>(ri + t);
      a1 = *reinterpret_cast<const uint32_t*>(rj + t);
      b0 = *reinterpret_cast<const uint32_t*>(pi + t);
      b1 = *reinterpret_cast<const uint32_t*>(pj + t);
      d0 = *reinterpret_cast<const uint32_t*>(ni + t);
      d1 = *reinterpret_cast<const uint32_t*>(nj + t);
      fl = *reinterpret_cast<const uint32_t*>(fl_f + t);
      mw = *reinterpret_cast<const uint32_t*>(mu_f + t);
    }
    int dr[4], dp[4], dn[4], m[4];
    bool counted[4], eq[4], ne[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int sh = 8 * b;
      dr[b] = (int)((a0 >> sh) & 0xFFu) - (int)((a1 >> sh) & 0xFFu);
      dp[b] = (int)((b0 >> sh) & 0xFFu) - (int)((b1 >> sh) & 0xFFu);
      dn[b] = (int)((d0 >> sh) & 0xFFu) - (int)((d1 >> sh) & 0xFFu);
      const uint32_t f = (fl >> sh) & 0xFFu;
      m[b] = (int)((mw >> sh) & 0xFFu);
      counted[b] = m[b] != 0 && !((f & TSF_POS) && (f & TSF_NEG));  // Fern.hpp:239, over the copies the fern holds
      eq[b] = (f & TSF_EQ) != 0;
      ne[b] = (f & TSF_NE) != 0;
    }
    if (ntau == 1) {  // zero optimizer: one intercept
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool r = dr[b] < taulo, p = dp[b] < taulo, q = dn[b] < taulo;  // Feature::getDecisions, Feature.hpp:101-109
        const bool e = eq[b] && (r == p), d = ne[b] || (r != q);
        acc_tp += (counted[b] && e && d) ? m[b] : 0;    // ref == pos, ref != neg
        acc_fp += (counted[b] && !e && !d) ? m[b] : 0;  // ref != pos, ref == neg
      }
    } else {
      // all intercepts at once, as in k_ts_eval_level: class masks over the index k (tau = taulo + k), their edges at
      // k >= 1 into the difference arrays, the value at k = 0 into the lane's own sums
      const unsigned long long valid = (ntau >= 64) ? ~0ull : ((1ull << ntau) - 1ull);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        auto step = [&](int diff) -> unsigned long long {
          const int k = diff - taulo + 1;  // first index whose intercept exceeds diff
          return k <= 0 ? ~0ull : (k >= 64 ? 0ull : (~0ull << k));
        };
        const unsigned long long rm = step(dr[b]), pm = step(dp[b]), qm = step(dn[b]);
        const unsigned long long am = rm ^ pm, bm = rm ^ qm;  // ref != pos ; ref != neg on this level
        unsigned long long tpm = 0ull, fpm = 0ull;
        if (counted[b]) {
          const unsigned long long e = eq[b] ? ~am : 0ull, d = ne[b] ? ~0ull : bm;
          tpm = (e & d) & valid;
          fpm = (~e & ~d) & valid;
        }
        acc_tp += (tpm & 1ull) ? m[b] : 0;
        acc_fp += (fpm & 1ull) ? m[b] : 0;
        unsigned long long up = tpm & ~(tpm << 1) & ~1ull, dn_ = ~tpm & (tpm << 1) & valid;
        while (up) { atomicAdd(&s_tp[__builtin_ctzll(up)], m[b]); up &= up - 1ull; }
        while (dn_) { atomicAdd(&s_tp[__builtin_ctzll(dn_)], -m[b]); dn_ &= dn_ - 1ull; }
        up = fpm & ~(fpm << 1) & ~1ull;
        dn_ = ~fpm & (fpm << 1) & valid;
        while (up) { atomicAdd(&s_fp[__builtin_ctzll(up)], m[b]); up &= up - 1ull; }
        while (dn_) { atomicAdd(&s_fp[__builtin_ctzll(dn_)], -m[b]); dn_ &= dn_ - 1ull; }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {  // (every lane of the workgroup is here: my_iters is the same for all of them)
    acc_tp += __shfl_xor(acc_tp, o);
    acc_fp += __shfl_xor(acc_fp, o);
  }
  if (lane == 0) {
    if (acc_tp) atomicAdd(&s_tp[0], acc_tp);
    if (acc_fp) atomicAdd(&s_fp[0], acc_fp);
  }
  __syncthreads();
  if (ntau > 1 && tid < 2) {  // difference arrays -> counts per intercept
    int* a = tid ? s_fp : s_tp;
    int acc = 0;
    for (int k = 0; k < ntau; ++k) {
      acc += a[k];
      a[k] = acc;
    }
  }
  __syncthreads();
  if (tid < ntau) {
    if (s_tp[tid]) atomicAdd(&tp[(long)blockIdx.y * ntau + tid], s_tp[tid]);
    if (s_fp[tid]) atomicAdd(&fp[(long)blockIdx.y * ntau + tid], s_fp[tid]);
  }
}

// copies evalSplit counts at all, per fern: the multiplicities of the triplets with !(pos.split && neg.split)
// (tot[f] zero on entry).  grid (at most 32, G): a workgroup strides over the fern's triplets and adds its sum once --
// one atomic per wave on the same few words, as k_ts_tot issues them, took longer here than the evaluation itself.
__global__ __launch_bounds__(TS_THREADS) void k_tf_tot(const uint8_t* __restrict__ flags, const uint8_t* __restrict__ mult,
                                                       const int32_t* __restrict__ lim, long np, int32_t* __restrict__ tot) {
  __shared__ int s_c[TS_THREADS / 64];
  const int fern = blockIdx.y;
  const long end = lim[fern];
  int c = 0;
  for (long t = ((long)blockIdx.x * TS_THREADS + threadIdx.x) * 4; t < end; t += (long)gridDim.x * TS_THREADS * 4) {
    const uint32_t fl = *reinterpret_cast<const uint32_t*>(flags + (long)fern * np + t);
    const uint32_t mw = *reinterpret_cast<const uint32_t*>(mult + (long)fern * np + t);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t f = (fl >> (8 * b)) & 0xFFu;
      c += ((f & TSF_POS) && (f & TSF_NEG)) ? 0 : (int)((mw >> (8 * b)) & 0xFFu);
    }
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < TS_THREADS / 64; ++w) sum += s_c[w];
    if (sum) atomicAdd(&tot[fern], sum);
  }
}

// every fern's winner of the level joins its fixed levels, as k_ts_commit does for one fern: best[f] is fern f's.
// Triplets the fern did not draw are left alone (nothing ever counts them).  grid (np / 256, G)
__global__ __launch_bounds__(TS_THREADS) void k_tf_commit(const uint8_t* __restrict__ planes, uint8_t* __restrict__ flags,
                                                          const uint8_t* __restrict__ mult, const int32_t* __restrict__ lim,
                                                          long np, const GpcSplit* __restrict__ best, int mark_split) {
  const int fern = blockIdx.y;
  const long t = (long)blockIdx.x * TS_THREADS + threadIdx.x;
  if (t >= lim[fern] || mult[(long)fern * np + t] == 0) return;  // lim <= np, and padding has multiplicity 0
  const GpcSplit w = best[fern];
  uint32_t f = flags[(long)fern * np + t];
  if (mark_split) {
    if (f & TSF_EQ) f |= TSF_POS;
    if (f & TSF_NE) f |= TSF_NEG;
  }
  const long oi = (long)w.i * np + t, oj = (long)w.j * np + t;
  const long pp = (long)TS_PATCH * np;
  const bool r = ts_dec(planes[oi], planes[oj], w.tau);
  const bool p = ts_dec(planes[oi + pp], planes[oj + pp], w.tau);
  const bool q = ts_dec(planes[oi + 2 * pp], planes[oj + 2 * pp], w.tau);
  if (r != p) f &= ~TSF_EQ;
  if (r != q) f |= TSF_NE;
  flags[(long)fern * np + t] = (uint8_t)f;
}

}  // namespace gpc
