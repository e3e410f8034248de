// k_hash.h -- fern hash codes: T <= 32 pixel-pair tests in a 27x27 window of `smooth`.
//
// Replaces ndb::gpcFilter / ndb::gpcFilterTau (filter.hpp:547-606, 619-683) plus the
// zero-filled code buffer and descriptor gather of Forest::evalFastMaskOnSubsetSSE
// (inference.hpp:274-290).
//
// Layout of the work (gfx950):
//   * a 512-thread workgroup owns a 256 x 32 output tile; the (256+32) x (32+26) smooth
//     window is staged once into LDS with 16-byte coalesced loads;
//   * a LANE owns 4 horizontally adjacent pixels, a WAVE one 256-pixel row segment in 4 consecutive rows.
//     The window is kept in LDS FOUR times, copy s shifted left by s bytes, so a tap for 4 pixels is ONE ALIGNED
//     dword of copy (dx & 3) at `lane base + scalar offset + row immediate` (unaligned LDS dwords work on gfx950 but
//     measured ~30x slower), and the compiler pairs the rows: two rows of a tap, 72 dwords apart, per ds_read2_b32 --
//     the cheapest LDS read form on this chip for this pattern (profiles/r03_ubench2_issue_rates.txt: a test's taps +
//     its 24 VALU take 8.7 ns per CU this way, 9.2-9.4 ns as aligned ds_read_b64 of row-interleaved storage, 11.4 ns as
//     eight ds_read_b32).  64 lanes read 256 contiguous bytes: conflict-free;
//   * the four unsigned byte compares of a test are done SWAR in 2 VALU ops (v_not, v_lerp_u8: swar_ge below) and shifted
//     into byte planes exactly like the reference's out[0..3] registers (2 more: 4 ops per test and 4 pixels,
//     + 2 address adds per test); the planes are transposed into 4 codes with v_perm_b32 at the end;
//   * the tests (packed LDS offsets, tau) are READ FROM DEVICE MEMORY with scalar loads, eight at a time (as a
//     by-value kernel argument the 64 words stayed live in SGPRs for the whole kernel and the allocator spilled 59 of
//     them); the test loop is fully unrolled, the taps of test t+1 are requested before test t is evaluated;
//   * what bounds the kernel: during the tests LDS reads (2 dwords per test and 4 pixels) and the 4 VALU per test add
//     up rather than overlap (52-56 % of a wave's time); the rest is waiting for the other waves at the two barriers
//     per tile, staging, candidate flags and stores (profiles/r03_a_phase_stamps.txt).
// No MFMA: this is gather/compare.
//
// Output is a dense code image (u32 per pixel): the code for candidates, GPC_NOCAND for
// everything else (DENSE=false), or exactly the reference's gpcstates buffer (DENSE=true,
// used by gpc_hip_hash_codes for parity checks).
#pragma once
#include "gpc_device.h"

namespace gpc {

// Diagnostic build only (-DGPC_STAMPS, tools/stamp_profile.py): s_memtime at the phase boundaries of a tile,
// summed per phase into a debug buffer nothing else reads.  No stamp executes in the product build.
#ifdef GPC_STAMPS
__device__ unsigned long long g_ht_stamps[16];
__device__ unsigned long long g_ht_wg[3 * 8192];  // per workgroup (flat block id < 8192): start, end (s_memrealtime), hardware id
#define HT_STAMP(i)                                                                         \
  do {                                                                                      \
    unsigned long long t_;                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    ht_acc[i] += t_ - ht_t0;                                                                \
    ht_t0 = t_;                                                                             \
  } while (0)
#define HT_STAMP_FLUSH()                                                                    \
  if (threadIdx.x == 0) { /* every workgroup: earliest start, latest start, latest end of the launch (s_memrealtime) */ \
    unsigned long long rt2_;                                                                  \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt2_)::"memory");         \
    atomicMax(&g_ht_stamps[8], (1ull << 62) - ht_rt0);                                        \
    atomicMax(&g_ht_stamps[9], ht_rt0);                                                       \
    atomicMax(&g_ht_stamps[10], rt2_);                                                        \
    const unsigned fb_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);      \
    if (fb_ < 8192u) {                                                                        \
      unsigned hw_, xcc_;                                                                     \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                       \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                     \
      g_ht_wg[3 * fb_] = ht_rt0;                                                              \
      g_ht_wg[3 * fb_ + 1] = rt2_;                                                            \
      g_ht_wg[3 * fb_ + 2] = ((unsigned long long)xcc_ << 32) | hw_;                          \
    }                                                                                         \
  }                                                                                           \
  if (threadIdx.x == 0 && ((blockIdx.x + blockIdx.y + blockIdx.z) & 31) == 5) {             \
    unsigned long long rt1_;                                                                  \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1_)::"memory");         \
    ht_acc[6] = rt1_ - ht_rt0; /* slot 6: the workgroup's life in s_memrealtime ticks (100 MHz) */ \
    ht_acc[7] = 1; /* slot 7: the number of workgroups that reported */                       \
    for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_ht_stamps[i_], ht_acc[i_]);                   \
  }
#define HT_STAMP_INIT()                                                                     \
  unsigned long long ht_t0;                                                                 \
  unsigned long long ht_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
  unsigned long long ht_rt0;                                                                \
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ht_rt0)::"memory");        \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ht_t0)::"memory")
#else
#define HT_STAMP(i)
#define HT_STAMP_INIT()
#define HT_STAMP_FLUSH()
#endif

#define HT_FAR 0x40000000   // a byte offset beyond every image (check_dims: at most 2^30 pixels)
#define SW_H 0x80808080u
#define SW_M 0x7F7F7F7Fu

// bit 7 of every byte: (b_byte >= a_byte), unsigned; the other bits are garbage
__device__ __forceinline__ uint32_t swar_ge(uint32_t a, uint32_t b) {
#ifdef HT_SWAR_SUB
  const uint32_t d = (b | SW_H) - (a & SW_M);  // per byte b_lo + 128 - a_lo: no borrow crosses bytes
  const uint32_t x = a ^ b;
  return (x & b) | (~x & d);                   // top bits differ -> b's top bit decides (v_bitop3_b32)
#else
  // v_lerp_u8 is a per-byte (x + y + (z & 1)) >> 1 with a 9-bit sum: (b + (255 - a) + 1) >> 1 = (b - a + 256) >> 1 has
  // bit 7 set exactly when b >= a.  Two instructions (v_not, v_lerp_u8 -- the latter issues at 1.6 times the cost of a
  // plain op, profiles/r03_ubench2_issue_rates.txt) where the subtract form takes four (or, and, sub, bitop3):
  // k_hash 432 -> 412-417 us per 256 pairs on one box.
  return __builtin_amdgcn_lerp(b, ~a, 0x01010101u);
#endif
}

// _mm_subs_epi8(b, tau) on 4 packed bytes: signed saturating subtract (filter.hpp:649-651).
// An int8 value placed in the HIGH byte of a 16-bit lane saturates under a saturating 16-bit
// subtract exactly when the int8 subtraction would (v_pk_sub_i16 with clamp), whatever the low
// byte holds: the lane is s * 256 + g with 0 <= g <= 255, minus tau * 256 it leaves [-32768, 32767]
// exactly when s - tau leaves [-128, 127], and a saturated lane (0x7FFF / 0x8000) has the saturated
// int8 in its high byte.  So the odd bytes are subtracted where they lie (the even byte below each is
// the garbage g), the even bytes after one shift (b1 below b2), and one permute picks the four high
// bytes: shl, pk_sub, pk_sub, perm = 4 VALU per 4 pixels (round 3 isolated both byte sets first: 5, two of
// them half-rate permutes).  tau_hi = (tau & 0xFF) << 8 in both 16-bit halves.
typedef short gpc_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t subs_epi8x4(uint32_t b, uint32_t tau_hi) {
  const uint32_t xe = b << 8;  // lanes [b0 : 0], [b2 : b1]
  gpc_short2 t, e, o;
  __builtin_memcpy(&t, &tau_hi, 4);
  __builtin_memcpy(&e, &xe, 4);
  __builtin_memcpy(&o, &b, 4);   // lanes [b1 : b0], [b3 : b2]
  e = __builtin_elementwise_sub_sat(e, t);
  o = __builtin_elementwise_sub_sat(o, t);
  uint32_t re, ro;
  __builtin_memcpy(&re, &e, 4);
  __builtin_memcpy(&ro, &o, 4);
  return __builtin_amdgcn_perm(ro, re, 0x07030501u);  // high bytes back in place: [e.1, o.1, e.3, o.3]
}

// ~_mm_subs_epi8(b, tau): the bytewise complement of the saturated difference.  ~s = -s - 1 maps [-128, 127] onto itself in
// reverse order, so ~clamp(s - tau) = clamp((tau - 1) - s): the same two packed subtracts with the constant as the minuend.
//   FORCE = false (forests without a tau of -128): the minuend is (tau - 1) * 256 + 255 in both halves and the byte below
//     the int8 stays as it lies (g): ((tau - 1) * 256 + 255) - (s * 256 + g) = (tau - 1 - s) * 256 + (255 - g) leaves
//     [-32768, 32767] exactly when tau - 1 - s leaves [-128, 127], and a saturated lane has the saturated int8 in its high
//     byte: shl, pk_sub, pk_sub, perm.  tau = -128 has no such minuend in 16 bits ((tau - 1) = -129).
//   FORCE = true (EVERY tau): the byte below the int8 is forced to 255 first (one OR; for the even bytes it rides in the
//     shift: v_lshl_or_b32) and the minuend is tau * 256: (tau * 256) - (s * 256 + 255) = (tau - 1 - s) * 256 + 1 -- two
//     operations more per test and row, taken only by forests that hold a tau of -128 (GpcForestDev::tau_m128; deciding it
//     per test cost every test of the kernel a three-way branch, ~20 scalar instructions).
// k = the minuend in both 16-bit halves.
template <bool FORCE>
__device__ __forceinline__ uint32_t subs_epi8x4_not(uint32_t b, uint32_t k) {
  const uint32_t xe = FORCE ? ((b << 8) | 0x00FF00FFu) : (b << 8);  // lanes [b0 : 255 / 0], [b2 : 255 / b1]
  const uint32_t xo = FORCE ? (b | 0x00FF00FFu) : b;                // lanes [b1 : 255 / b0], [b3 : 255 / b2]
  gpc_short2 t, e, o;
  __builtin_memcpy(&t, &k, 4);
  __builtin_memcpy(&e, &xe, 4);
  __builtin_memcpy(&o, &xo, 4);
  e = __builtin_elementwise_sub_sat(t, e);
  o = __builtin_elementwise_sub_sat(t, o);
  uint32_t re, ro;
  __builtin_memcpy(&re, &e, 4);
  __builtin_memcpy(&ro, &o, 4);
  return __builtin_amdgcn_perm(ro, re, 0x07030501u);
}

// unsigned saturating add of a uniform constant to 4 packed bytes (same high-byte argument: the lane x * 256 + g plus
// t * 256 passes 65535 exactly when x + t passes 255; v_pk_add_u16 clamp)
typedef unsigned short gpc_ushort2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t uaddsat_x4(uint32_t x, uint32_t t_hi) {
  const uint32_t xe = x << 8;
  gpc_ushort2 t, e, o;
  __builtin_memcpy(&t, &t_hi, 4);
  __builtin_memcpy(&e, &xe, 4);
  __builtin_memcpy(&o, &x, 4);
  e = __builtin_elementwise_add_sat(e, t);
  o = __builtin_elementwise_add_sat(o, t);
  uint32_t re, ro;
  __builtin_memcpy(&re, &e, 4);
  __builtin_memcpy(&ro, &o, 4);
  return __builtin_amdgcn_perm(ro, re, 0x07030501u);
}

// One test for RPW rows: shift the 4 compare bits of every row into its byte plane
// (new bit enters at bit 7, so the first test of a plane ends up on bit 0 after 8 steps).
// NAIVE (the reference's SSE=OFF build): the tau predicate is the plain integer a > b - tau
// (filter.hpp:276):  tau >= 1:  sat(a + tau - 1) >= b ;  tau <= 0:  a > sat(b - tau).
template <bool TAU, bool NAIVE, int RPW>
__device__ __forceinline__ void fern_test(const uint8_t* __restrict__ tile, int lanebase, int packed, int tau,
                                          uint32_t (&plane)[RPW]) {
  // packed: dword offsets (copy select + row + column) of the two taps
  const uint32_t* pa = reinterpret_cast<const uint32_t*>(tile + lanebase) + (int)(int16_t)(packed & 0xFFFF);
  const uint32_t* pb = reinterpret_cast<const uint32_t*>(tile + lanebase) + (packed >> 16);
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    uint32_t a = pa[r * (HT_STRIDE / 4)];
    uint32_t b = pb[r * (HT_STRIDE / 4)];
    uint32_t ge;  // bit 7 of each byte = NOT(code bit)
    if (TAU && NAIVE) {
      if (tau >= 1) {  // wave-uniform
        const uint32_t c = uaddsat_x4(a, (uint32_t)min(tau - 1, 255) * 0x01000100u);
        ge = ~swar_ge(b, c);  // code bit = (c >= b)
      } else {
        ge = swar_ge(a, uaddsat_x4(b, (uint32_t)min(-tau, 255) * 0x01000100u));
      }
    } else {
      if (TAU) b = subs_epi8x4(b, (uint32_t)(tau & 0xFF) * 0x01000100u);
      ge = swar_ge(a, b);
    }
    // bit 7 of every byte from ge, the rest from plane >> 1: one v_bitop3 (full rate; v_bfi / v_and_or
    // issue at half rate on gfx950, profiles/r02_ubench2_issue_rates.txt)
    plane[r] = __builtin_amdgcn_bitop3_b32(ge, plane[r] >> 1, SW_H, 0xE4);
  }
}

// N consecutive tests (slots t0 .. t0+N-1, the first `cnt` of them real) into one plane, software-pipelined: the taps
// of test i + HT_PIPE are requested before test i is evaluated, so HT_PIPE tests' LDS reads are in flight behind the
// 24 VALU operations of one.  (Left to itself the compiler requests one test ahead.)
#ifndef HT_PIPE
#define HT_PIPE 1   // measured per 256 pairs on one box: 0 (compiler's own order) 448 us, 1 -> 439, 2 -> 443, 3 -> 447
#endif
template <bool TAU, bool NAIVE, int RPW, int N, bool M128 = true>
__device__ __forceinline__ void fern_group(const uint8_t* __restrict__ tile, int lanebase,
                                           const GpcForestDev* __restrict__ fp, int t0, int cnt, uint32_t (&plane)[RPW]) {
#if HT_PIPE == 0
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (i < cnt) fern_test<TAU, NAIVE, RPW>(tile, lanebase, fp->off[t0 + i], TAU ? fp->tau[t0 + i] : 0, plane);
#else
  constexpr int D = HT_PIPE + 1;
  uint32_t a[D][RPW], b[D][RPW];
  const uint32_t* base = reinterpret_cast<const uint32_t*>(tile + lanebase);
#ifndef HT_PACKED_OFFS
  // the group's tap offsets (and, TAU, its tests' minuends) in one scalar load ahead of the tests: fetched where
  // each test needs them, the branches a TAU test takes keep the compiler from merging the loads, and every test then
  // waits out a scalar-cache round trip (s_load_dwordx2 + s_waitcnt lgkmcnt(0)) in front of its LDS reads.  boff[] has 64
  // entries and tauk[] 32 whatever T is, so slots past `cnt` are readable.
  uint32_t goff[2 * N];
#pragma unroll
  for (int i = 0; i < 2 * N; ++i) goff[i] = fp->boff[2 * t0 + i];
  // (SSE arithmetic: the minuend of each test's complemented subtract, 0 for a tau of 0 -- built by the host, gpc_hip_set_forest)
  uint32_t gk[N];
  if (TAU && !NAIVE) {
#pragma unroll
    for (int i = 0; i < N; ++i) gk[i] = (uint32_t)fp->tauk[t0 + i];
  }
#endif
  auto load = [&](int i, int slot) {
#ifndef HT_PACKED_OFFS  // (byte offsets, two words per test: 404-405 vs 408-414 us per 256 pairs against the packed dword offsets)
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base) + goff[2 * i]);
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base) + goff[2 * i + 1]);
#else
    const int packed = fp->off[t0 + i];
    const uint32_t* pa = base + (int)(int16_t)(packed & 0xFFFF);
    const uint32_t* pb = base + (packed >> 16);
#endif
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      a[slot][r] = pa[r * (HT_STRIDE / 4)];
      b[slot][r] = pb[r * (HT_STRIDE / 4)];
    }
  };
#pragma unroll
  for (int i = 0; i < HT_PIPE && i < N; ++i)
    if (i < cnt) load(i, i % D);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i + HT_PIPE < N && i + HT_PIPE < cnt) load(i + HT_PIPE, (i + HT_PIPE) % D);
    __builtin_amdgcn_sched_barrier(0);
    if (i < cnt) {
      // SSE arithmetic: the test's minuend; Naive: the int
#ifndef HT_PACKED_OFFS
      const uint32_t k = (TAU && !NAIVE) ? gk[i] : 0u;
#else
      const uint32_t k = (TAU && !NAIVE) ? (uint32_t)fp->tauk[t0 + i] : 0u;
#endif
      const int tau = (TAU && NAIVE) ? fp->tau[t0 + i] : 0;
      if (TAU && !NAIVE && k != 0u) {
        // k is wave-uniform (a scalar load) and the loop is unrolled, so this is a scalar branch per test (a test whose tau
        // is 0 -- _mm_subs_epi8(b, 0) = b, 7 of the 30 tests of defaultTauForest.txt -- takes the plain compare below).
        // The compare needs one operand complemented: here the saturating subtract delivers ~b' itself (no v_not),
        // v_lerp_u8(a, ~b', 0) has bit 7 = (a + 255 - b' >= 256) = (a > b') = the code bit, and the plane takes its
        // complement (the planes hold NOT(code bit), complemented once per row at the end).
        {
#pragma unroll
          for (int r = 0; r < RPW; ++r) {
            const uint32_t gt = __builtin_amdgcn_lerp(a[i % D][r], subs_epi8x4_not<M128>(b[i % D][r], k), 0u);
            // (the first test of a plane: see below)
            plane[r] = i == 0 ? ~gt : __builtin_amdgcn_bitop3_b32(gt, plane[r] >> 1, SW_H, 0x4E);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          uint32_t av = a[i % D][r], bv = b[i % D][r];
          uint32_t ge;
          if (TAU && NAIVE) {
            if (tau >= 1) {
              const uint32_t c = uaddsat_x4(av, (uint32_t)min(tau - 1, 255) * 0x01000100u);
              ge = ~swar_ge(bv, c);
            } else {
              ge = swar_ge(av, uaddsat_x4(bv, (uint32_t)min(-tau, 255) * 0x01000100u));
            }
          } else {
            ge = swar_ge(av, bv);
          }
          // The first test of a plane takes the compare word as it is (bits 0 .. 6 of its bytes are garbage): whatever lies
          // below bit 7 after the first step has left the byte after seven more, and the planes with fewer tests are read
          // through masks that keep only the tests' bits (q0: bit 7 of P8's bytes; q3: the n3 bits m3 selects after the shift
          // by 8 - n3) -- a shift and a v_bitop3 less per plane and row.
          plane[r] = i == 0 ? ge : __builtin_amdgcn_bitop3_b32(ge, plane[r] >> 1, SW_H, 0xE4);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#endif
}

#ifndef HT_NO_SETPRIO
#define HT_PRIO_STEP(l) ht_set_prio(min((l), prio_cap))
#else
#define HT_PRIO_STEP(l) do { } while (0)
#endif
// s_setprio takes an immediate: one scalar branch per level (lvl is wave-uniform)
__device__ __forceinline__ void ht_set_prio(int lvl) {
  if (lvl >= 3) __builtin_amdgcn_s_setprio(3);
  else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
  else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

// bit 7 of every byte of x that is not zero (SWAR)
__device__ __forceinline__ uint32_t swar_nonzero(uint32_t x) { return (((x & SW_M) + SW_M) | x) & SW_H; }

// smooth, grad, candmap: [nimg][H][W]; codes: [nimg][H][W] u32
// candmap == nullptr: candidate <=> grad != 0 inside the margin (preprocessImage's mask).
// NAIVE: gpcFilterNaive / gpcFilterTauNaive (filter.hpp:237-281) -- code bits MSB-first
// (test t on bit T-1-t), every candidate row hashed, no 16-pixel group skip.  The host passes the
// tests in reverse order (slot u = test T-1-u) so that slot u lands on bit u.
//
// Tiles start at row 13: rows above it (and from H-13 on) hold no candidate, the matchers never read
// them, and 410 candidate rows of a 436-row image are 13 tiles of 32 rows where the whole image is 14.
// (DENSE, the parity entry point: the host zero-fills the code image first.)
// The tests are read from memory (fp, 264 bytes every wave shares) with scalar loads, eight at a time: as
// a by-value kernel argument the 64 words stayed live in SGPRs for the whole kernel and the allocator spilled
// 59 of them to VGPR lanes (~100 v_readlane / v_writelane per tile).
#ifdef HT_WAVES_PER_EU   // tuning builds: a register budget for more workgroups per CU than the launch bounds alone give
#define HT_OCC __attribute__((amdgpu_waves_per_eu(HT_WAVES_PER_EU, HT_WAVES_PER_EU)))
#else
#define HT_OCC
#endif
// GBITS: `grad` is k_preprocess<..., BITS>'s bit image (one bit per pixel); a lane fetches the 16 bits of its 16-pixel group:
// "any gradient in the group" is that word != 0 (where the byte image needs two DPP permutes), its own nibble the candidates.
// TY: rows of a tile (HT_Y = 32; 40 for launches that fit ONE round of resident workgroups with the taller tile and two
// with the lower: a single 1920x1080 pair is 528 tiles of 32 rows for 512 slots, 432 of 40 rows).  The taps' LDS offsets
// depend on it (a shifted copy of the window is (TY + 26) rows): the host keeps one GpcForestDev per height.
template <bool TAU, bool DENSE, bool NAIVE, bool GBITS = false, int TY = HT_Y>
__global__ __launch_bounds__(HT_THREADS) HT_OCC void k_hash(const uint8_t* __restrict__ smooth,
                                              const uint8_t* __restrict__ grad,
                                              const uint8_t* __restrict__ candmap,
                                              uint32_t* __restrict__ codes, int W, int H,
                                              const GpcForestDev* __restrict__ fp, int32_t* __restrict__ img_stats,
                                              int tpw, int last_round_from) {
#define HT_GROUPS 0
#include "k_hash_body.h"
#undef HT_GROUPS
}

// INV: the OR of the codes from the last plane's complemented bytes (bits 24 .. 30; only the n3 bits m3 selects are code
// bits) and every lower bit the forest has: tests 0 .. 7 -> bits 0 .. 7, test 8 -> bit 0, tests 9 .. 24 -> bits 8 .. 23
// (k_hash_groups: per group and tile)
__device__ __forceinline__ uint32_t ht_inv_cor(uint32_t cor3, uint32_t m3, int T) {
  uint32_t t = cor3 & m3;
  t |= t >> 16;
  t |= t >> 8;
  const int lowbits = T <= 8 ? T : (T - 1 < 24 ? T - 1 : 24);
  return ((t & 0x7Fu) << 24) | ((1u << lowbits) - 1u);
}

// GROUPS: the forest is `ngroups` groups of <= 32 tests (gpc_hip_set_forest_groups), group g's tests in fp_groups[g].  The
// window is staged and the candidate flags are computed once per tile; then every group runs its tests, transposes its
// planes and stores its code plane, one group's planes in registers at a time.  Image img = 2p + s writes group g's codes
// and statistics as virtual image (p * ngroups + g) * 2 + s with gstep = 2 -- the layout [pair][group][side][H][W], in which
// group g of pair p is the virtual pair p * ngroups + g -- or, one image and gstep = 1, as image g ([group][H][W]).
template <bool TAU, bool DENSE, bool NAIVE, bool GBITS = false, int TY = HT_Y>
__global__ __launch_bounds__(HT_THREADS) HT_OCC void k_hash_groups(const uint8_t* __restrict__ smooth,
                                              const uint8_t* __restrict__ grad,
                                              const uint8_t* __restrict__ candmap,
                                              uint32_t* __restrict__ codes, int W, int H,
                                              const GpcForestDev* __restrict__ fp_groups, int32_t* __restrict__ img_stats,
                                              int tpw, int last_round_from, int ngroups, int gstep) {
#define HT_GROUPS 1
#include "k_hash_body.h"
#undef HT_GROUPS
}

// candmap[img][k] = 1 for every k of the caller's mask list (inside the margin)
__global__ void k_scatter_mask(const int32_t* __restrict__ mask, int n_mask, uint8_t* __restrict__ candmap,
                               int W, int H) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_mask) return;
  const int k = mask[i];
  if (k < 0 || k >= W * H) return;
  const int x = k % W, y = k / W;
  if (x >= GPC_R && x < W - GPC_R && y >= GPC_R && y < H - GPC_R) candmap[k] = 1;
}

}  // namespace gpc
