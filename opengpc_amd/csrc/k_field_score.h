// k_field_score.h -- dense fields scored against ground truth on the device (gpc_hip_score_fields*, include/gpc_hip.h has
// the rule): one streaming pass, 8 C + 1 bytes read per pixel (+ 1 with a class plane), 2 written with the error plane.
//
//   k_field_score<C, BINS>   a persistent grid of at most FS_MAX_GROUPS workgroups strides over the launch's items; an item
//                            is one chunk (FS_SLOTS slots of four pixels) of one pair.  A slot is the four pixels behind a
//                            16-byte boundary of the pair's first field plane: a plane whose own four elements there lie
//                            on its natural boundary too is read with one vector load (16 bytes of int32 / float, 4 of
//                            uint8; 8 bytes of uint16 written), every other plane, and the slots that the pair's first or
//                            last pixel cuts, element by element.  Both ways fill the same registers and one piece of
//                            code judges them: the result does not depend on the way a pixel took.
//
// Counting: without bins every count is a wave's ballot and popcount, and the two sums are 64-bit per lane.  With bins
// (BINS: a class plane or speed bounds) a lane keeps each count as four 16-bit fields of one 64-bit word, one field per
// bin -- the add is one shifted 1 -- and the sums per bin; FS_FLUSH_CHUNKS bounds what a field collects.  When the pair
// changes (and at the end) the workgroup flushes: a wave reduction, every wave's 64 words into LDS, and thread w adds word
// w of all waves into the pair's gpc_field_score with at most one 64-bit integer atomic (agent scope) per nonzero word.
// Integer sums do not depend on the order of arrival: the bytes are deterministic.
//
// The square root: e2 <= 2^32 goes through v_sqrt_f32 (1 ulp) of its float; conversion and root together are off by
// less than 2^-22 relative, 0.02 absolute at 65536, so the truncated estimate is within 1 of the floor and one step either
// way, decided in integers, makes it exact.
#pragma once
#include "field_score_host.h"
#include "gpc_device.h"
#include "k_score.h"

#define FS_NONE (-2147483647 - 1)  // GPC_DENSE_NONE

namespace gpc {

// four elements of a plane at pixels i0 .. i0 + 3 of n: one load where `vec`, else the pixels inside the plane one by one
__device__ __forceinline__ void fs_load4(const int32_t* __restrict__ p, long i0, long n, bool vec, int32_t (&o)[4]) {
  if (vec) {
    const int4 v = *reinterpret_cast<const int4*>(p + i0);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (i0 + j >= 0 && i0 + j < n) ? p[i0 + j] : 0;
  }
}
__device__ __forceinline__ void fs_load4(const float* __restrict__ p, long i0, long n, bool vec, float (&o)[4]) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p + i0);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (i0 + j >= 0 && i0 + j < n) ? p[i0 + j] : 0.f;
  }
}
// four bytes as one word, pixel j in byte j; a null plane reads as zeros
__device__ __forceinline__ uint32_t fs_load4(const uint8_t* __restrict__ p, long i0, long n, bool vec) {
  if (!p) return 0u;
  if (vec) return *reinterpret_cast<const uint32_t*>(p + i0);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i0 + j >= 0 && i0 + j < n) w |= (uint32_t)p[i0 + j] << (8 * j);
  return w;
}

// floor(sqrt(x)), x <= 2^32
__device__ __forceinline__ uint32_t fs_isqrt(unsigned long long x) {
  const float f = (x >> 32) ? 4294967296.f : (float)(uint32_t)x;
  uint32_t r = (uint32_t)__builtin_amdgcn_sqrtf(f);
  if ((unsigned long long)r * r > x) --r;
  else if ((unsigned long long)(r + 1) * (r + 1) <= x) ++r;
  return r;
}

// a packed count (four 16-bit fields) as two words of two 32-bit fields, summed over the wave: bins 0 | 1 and 2 | 3
__device__ __forceinline__ void fs_unpack_sum(unsigned long long x, unsigned long long (&bin)[4]) {
  const unsigned long long s01 = sc_wave_sum((x & 0xFFFFull) | (((x >> 16) & 0xFFFFull) << 32));
  const unsigned long long s23 = sc_wave_sum(((x >> 32) & 0xFFFFull) | ((x >> 48) << 32));
  bin[0] = s01 & 0xFFFFFFFFull, bin[1] = s01 >> 32, bin[2] = s23 & 0xFFFFFFFFull, bin[3] = s23 >> 32;
}

// what a workgroup holds between two flushes
template <bool BINS>
struct FsAcc;
template <>
struct FsAcc<false> {
  uint32_t head[4], jud, in[8], out;  // wave-uniform counts
  unsigned long long e, e2;           // per lane
};
template <>
struct FsAcc<true> {
  uint32_t head[4];                   // wave-uniform counts
  unsigned long long jud, in[8], out; // per lane: four 16-bit fields, bin b at bit 16 b
  unsigned long long e[4], e2[4];     // per lane, per bin
};

template <bool BINS>
__device__ __forceinline__ void fs_clear(FsAcc<BINS>& a) {
#pragma unroll
  for (int k = 0; k < 4; ++k) a.head[k] = 0;
  a.jud = 0, a.out = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) a.in[k] = 0;
  if constexpr (BINS) {
#pragma unroll
    for (int b = 0; b < 4; ++b) a.e[b] = 0, a.e2[b] = 0;
  } else {
    a.e = 0, a.e2 = 0;
  }
}

// the workgroup's counts into the pair's score: every wave's words through LDS, one atomic per nonzero word
template <bool BINS>
__device__ __forceinline__ void fs_flush(const FsAcc<BINS>& a, unsigned long long (*s_part)[FS_WORDS],
                                         unsigned long long* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* row = s_part[wave];
  __syncthreads();  // (the rows may still be read by the flush before)
  row[lane] = 0;
  if constexpr (BINS) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) row[k] = a.head[k];
    }
#pragma unroll
    for (int w = 0; w < FS_TALLY_WORDS; ++w) {  // word by word, so that few totals are held at a time
      unsigned long long t[4];
      if (w == 0) fs_unpack_sum(a.jud, t);
      else if (w <= 8) fs_unpack_sum(a.in[w - 1], t);
      else if (w == 9) fs_unpack_sum(a.out, t);
      else {
#pragma unroll
        for (int b = 0; b < 4; ++b) t[b] = sc_wave_sum(w == 10 ? a.e[b] : a.e2[b]);
      }
      if (lane == 0) {
        row[FS_WORD_ALL + w] = t[0] + t[1] + t[2] + t[3];
#pragma unroll
        for (int b = 0; b < 4; ++b) row[FS_WORD_BIN + FS_TALLY_WORDS * b + w] = t[b];
      }
    }
  } else {
    const unsigned long long e = sc_wave_sum(a.e), e2 = sc_wave_sum(a.e2);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) row[k] = a.head[k];
#pragma unroll
      for (int o = 0; o < 2; ++o) {  // `all`, and bin 0, which is all there is
        unsigned long long* t = row + (o ? FS_WORD_BIN : FS_WORD_ALL);
        t[0] = a.jud;
#pragma unroll
        for (int k = 0; k < 8; ++k) t[1 + k] = a.in[k];
        t[9] = a.out, t[10] = e, t[11] = e2;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < FS_WORDS) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < FS_THREADS / 64; ++w) t += s_part[w][threadIdx.x];
    if (t) __hip_atomic_fetch_add(dst + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// field [P][C][n], tu / tv / ign / cls / err [P][n] (tv: C == 2 only; ign, cls, err may be null), scores [P][FS_WORDS]
// cleared; chunks = fs_chunks per pair, items = chunks * P
template <int C, bool BINS>
__global__ __launch_bounds__(FS_THREADS) void k_field_score(const int32_t* __restrict__ field, const float* __restrict__ tu,
                                                            const float* __restrict__ tv, const uint8_t* __restrict__ ign,
                                                            const uint8_t* __restrict__ cls, long n, long chunks, long items,
                                                            FsPrm prm, unsigned long long* __restrict__ scores,
                                                            uint16_t* __restrict__ err) {
  __shared__ unsigned long long s_part[FS_THREADS / 64][FS_WORDS];
  FsAcc<BINS> acc;
  fs_clear(acc);
  long cur = -1;
  int held = 0;  // chunks since the last flush
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const long p = item / chunks, chunk = item - p * chunks;
    if (p != cur || held >= FS_FLUSH_CHUNKS) {  // (uniform over the workgroup)
      if (cur >= 0) fs_flush<BINS>(acc, s_part, scores + cur * FS_WORDS);
      fs_clear(acc);
      cur = p, held = 0;
    }
    ++held;
    const int32_t* pf = field + p * C * n;
    const float* pu = tu + p * n;
    const float* pv = C == 2 ? tv + p * n : nullptr;
    const uint8_t* pi = ign ? ign + p * n : nullptr;
    const uint8_t* pc = cls ? cls + p * n : nullptr;
    uint16_t* pe = err ? err + p * n : nullptr;
    // the slot phase: pixel 4 s - q is the first of slot s, and lies on a 16-byte boundary of the first field plane
    const int q = (int)(((uintptr_t)pf >> 2) & 3);
    const bool v_f1 = C == 2 && (int)(((uintptr_t)(pf + n) >> 2) & 3) == q;
    const bool v_u = (int)(((uintptr_t)pu >> 2) & 3) == q, v_v = C == 2 && (int)(((uintptr_t)pv >> 2) & 3) == q;
    const bool v_i = (int)((uintptr_t)pi & 3) == q, v_c = (int)((uintptr_t)pc & 3) == q;
    const bool v_e = (int)(((uintptr_t)pe >> 1) & 3) == q;

    int32_t f0[FS_UNROLL][4], f1[FS_UNROLL][4];
    float gu[FS_UNROLL][4], gv[FS_UNROLL][4];
    uint32_t gi[FS_UNROLL], gc[FS_UNROLL];
    long i0[FS_UNROLL];
    bool whole[FS_UNROLL];
#pragma unroll
    for (int s = 0; s < FS_UNROLL; ++s) {  // every load of the chunk before the first use
      i0[s] = (chunk * FS_SLOTS + s * FS_THREADS + threadIdx.x) * FS_PX - q;
      whole[s] = i0[s] >= 0 && i0[s] + FS_PX <= n;
      const bool live = i0[s] < n;  // (i0 + 3 >= 0 always)
      const long m = live ? n : 0;  // beyond the pair nothing is read
      fs_load4(pf, i0[s], m, whole[s], f0[s]);
      if constexpr (C == 2) {
        fs_load4(pf + n, i0[s], m, whole[s] && v_f1, f1[s]);
        fs_load4(pv, i0[s], m, whole[s] && v_v, gv[s]);
      }
      fs_load4(pu, i0[s], m, whole[s] && v_u, gu[s]);
      gi[s] = fs_load4(pi, i0[s], m, whole[s] && v_i);
      gc[s] = BINS ? fs_load4(pc, i0[s], m, whole[s] && v_c) : 0u;
    }
#pragma unroll
    for (int s = 0; s < FS_UNROLL; ++s) {
      uint32_t ev[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long i = i0[s] + j;
        const bool valid = i >= 0 && i < n;
        const bool ignored = valid && ((gi[s] >> (8 * j)) & 0xFFu) != 0;
        const float u = gu[s][j], v = C == 2 ? gv[s][j] : 0.f;
        const bool ok = fabsf(u) <= FS_TRUTH_MAX && fabsf(v) <= FS_TRUTH_MAX;  // (false for NaN)
        const bool rest = valid && !ignored;
        const bool notruth = rest && !ok, hole = rest && ok && f0[s][j] == FS_NONE;
        const bool judged = rest && ok && f0[s][j] != FS_NONE;
        const long long t0 = ok ? (long long)(int)rintf(256.f * u) : 0;
        const long long t1 = (C == 2 && ok) ? (long long)(int)rintf(256.f * v) : 0;
        const long long d0 = (long long)f0[s][j] - t0;
        const unsigned long long b0 = (unsigned long long)(d0 < 0 ? -d0 : d0);
        const uint32_t a0 = (uint32_t)(b0 < FS_AXIS_MAX ? b0 : FS_AXIS_MAX);
        unsigned long long e2 = (unsigned long long)a0 * a0;
        if constexpr (C == 2) {
          const long long d1 = (long long)f1[s][j] - t1;
          const unsigned long long b1 = (unsigned long long)(d1 < 0 ? -d1 : d1);
          const uint32_t a1 = (uint32_t)(b1 < FS_AXIS_MAX ? b1 : FS_AXIS_MAX);
          e2 += (unsigned long long)a1 * a1;
          e2 = e2 < FS_E2_MAX ? e2 : FS_E2_MAX;
        }
        const uint32_t e = fs_isqrt(e2);
        const unsigned long long m2 = (unsigned long long)(t0 * t0) + (unsigned long long)(t1 * t1);
        // thr_q8 and out_abs_q8 are at most 65535, so their squares lie below 2^32 - 1 and e2 is compared saturated, in 32 bits
        const uint32_t es = (e2 >> 32) ? 0xFFFFFFFFu : (uint32_t)e2;
        const bool outlier = judged && es > prm.abs2 && e2 * 1000000ull > m2 * prm.rel2;
        ev[j] = judged ? (e < 0xFFFEu ? e : 0xFFFEu) : 0xFFFFu;

        acc.head[0] += __popcll(__ballot(valid));
        acc.head[1] += __popcll(__ballot(ignored));
        acc.head[2] += __popcll(__ballot(notruth));
        acc.head[3] += __popcll(__ballot(hole));
        if constexpr (BINS) {
          int bin;
          if (pc) {
            const int c = (int)((gc[s] >> (8 * j)) & 0xFFu);
            bin = c < 3 ? c : 3;
          } else {
            bin = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) bin += (k < prm.n_speed && m2 >= prm.sp2[k]) ? 1 : 0;
          }
          const unsigned long long one = judged ? 1ull << (16 * bin) : 0ull;
          acc.jud += one;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k < prm.n_thr) acc.in[k] += es <= prm.thr2[k] ? one : 0ull;
          acc.out += outlier ? one : 0ull;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const bool mine = judged && bin == b;
            acc.e[b] += mine ? e : 0u;
            acc.e2[b] += mine ? e2 : 0ull;
          }
        } else {
          acc.jud += __popcll(__ballot(judged));
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k < prm.n_thr) acc.in[k] += __popcll(__ballot(judged && es <= prm.thr2[k]));
          acc.out += __popcll(__ballot(outlier));
          acc.e += judged ? e : 0u;
          acc.e2 += judged ? e2 : 0ull;
        }
      }
      if (pe) {
        if (whole[s] && v_e) {
          *reinterpret_cast<uint2*>(pe + i0[s]) = make_uint2(ev[0] | (ev[1] << 16), ev[2] | (ev[3] << 16));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i0[s] + j >= 0 && i0[s] + j < n) pe[i0[s] + j] = (uint16_t)ev[j];
        }
      }
    }
  }
  if (cur >= 0) fs_flush<BINS>(acc, s_part, scores + cur * FS_WORDS);
}

}  // namespace gpc
