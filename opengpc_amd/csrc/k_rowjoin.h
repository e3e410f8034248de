// k_rowjoin.h -- epipolar-mode collision matching: per-row LDS hash join + counting rank.
//
// Replaces, for settings.epipolarMode_ == true, the descriptor build + `state |= y<<32`
// (inference.hpp:189-197), Forest::findCorrespondences (std::sort x2 + merge scan,
// inference.hpp:227-254) and the disparity filter of rectifiedMatch (inference.hpp:384-391).
// One image row per workgroup: with the row in the upper 32 state bits the reference's global
// sort is a per-row sort by code, and a source code can only meet target codes of its own row.
//
// What the reference's sort+merge decides for a row is, per code c:  cntL(c) == 1 and
// cntR(c) == 1  (with the tail-quirk variant cntR == 2 for the largest right code of the
// last populated right row); the sort is needed only for the ORDER of the output (ascending
// code).  So, entirely in LDS and without any compare-and-swap or sorting network:
//   1. the left row's codes are inserted into an ordered open-addressing table with
//      ds_max_rtn (Amble-Knuth ordered linear probing; a wave-level LDS CAS measured ~72
//      cycles of LDS pipe on MI355X, a returning ds_max ~8);
//   2. both rows look their code up (plain reads) and mark the slot: a returning ds_or sets the
//      side's SEEN flag, and a record that finds it already set adds the side's DUP flag; a right
//      record ORs its x into the (zeroed) low half of the same word with the same atomic: if the
//      right code is unique there was one writer, otherwise the value is not used;
//   3. every left record reads its slot: match iff neither side is DUP and the right side was
//      SEEN (+ disparity filter);
//   4. output position = rank of the code among the row's matches, by COUNTING on the top
//      bits the image's codes really use (k_hash ORs them into img_stats: bits a forest leaves
//      clear cost no resolution): one returning ds_add per match, an exclusive scan over the NT*SPT bucket counters
//      (DPP wave scan), and a look at the < 1 other matches sharing the bucket.
//      The thread still holds xL and xR, so it writes the packed support straight to its place.
//
// This header is the ONE-ROW-PER-WORKGROUP form: small launches, rows wider than 4096 pixels, the host entry point's gap-free
// packing (join + k_gather_rows as two launches) and, with VIRT, the partitions of the non-epipolar matcher.  Batched launches
// take k_rowjoin_fused.h: the same join as a persistent kernel that also writes the supports.
//
// 32-bit codes (WIDE): the SSE=OFF arithmetic with a 32-test forest sets bit 31, and the code
// 0xFFFFFFFF then collides with both sentinels (GPC_NOCAND in the code image, key 0 = code + 1
// in the table).  The WIDE instantiations read the candidate byte of such pixels to tell them
// apart and keep the one code that has no table key in three shared counters instead.
#pragma once
#include "gpc_device.h"

namespace gpc {

#define RJ_EMPTY 0xFFFFFFFFu
// flags of a table slot (high half of its word; the low half holds a right record's x)
#define RJ_LSEEN 0x00010000u
#define RJ_LDUP 0x00020000u
#define RJ_RSEEN 0x00040000u
#define RJ_RDUP 0x00080000u

// Diagnostic build only (-DGPC_STAMPS, tools/stamp_profile.py): s_memtime at phase boundaries,
// summed per phase into a debug buffer nothing else reads.  No stamp executes in the product build.
#ifdef GPC_STAMPS
__device__ unsigned long long g_rj_stamps[16];
#define RJ_STAMP(i)                                                                         \
  do {                                                                                      \
    unsigned long long t_;                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    rj_acc[i] = t_ - rj_t0;                                                                 \
    rj_t0 = t_;                                                                             \
  } while (0)
// one workgroup in 64 reports (uncontended atomics, issued after the last stamp)
#define RJ_STAMP_FLUSH()                                                                    \
  if (threadIdx.x == 0 && (blockIdx.x & 63) == 5)                                           \
    for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_rj_stamps[i_], rj_acc[i_])
#define RJ_STAMP_INIT()                                                                     \
  unsigned long long rj_t0;                                                                 \
  unsigned long long rj_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rj_t0)::"memory")
#else
#define RJ_STAMP(i)
#define RJ_STAMP_INIT()
#define RJ_STAMP_FLUSH()
#endif

__device__ __forceinline__ uint32_t rj_hash(uint32_t key, int shift) { return (key * 0x9E3779B1u) >> shift; }

// ---------------------------------------------------------------- the join table
// Measured on MI355X (profiles/r01_ubench_lds_valu_calibration.txt): a wave-level LDS
// compare-and-swap costs ~72 cycles of the CU's LDS pipe, a returning ds_max/ds_add ~8, a plain
// random ds_read ~3.  So the table is built WITHOUT CAS: ordered linear probing (Amble & Knuth)
// with ds_max_rtn -- a probe writes max(slot, key); if it displaced a smaller key it carries
// that key on to the next slot.  Within one insert phase this converges to the unique ordered
// table whatever the interleaving; lookups (after the barrier) are read-only and stop at the
// first slot holding a smaller key.  Stored key = code + 1 (0 = empty slot).
// Only LEFT codes are inserted; right records merely look their code up.  A slot costs 8 bytes
// (key + one word of flags and x): 16 KiB per 1024-px row and 64 VGPRs, so EIGHT workgroups = 32
// waves share a CU.
//
// The two probe loops are written in gfx950 assembly: the lanes still probing narrow EXEC with
// v_cmpx and the loop ends on s_cbranch_execnz -- one scalar instruction per round where the
// compiler's structurised form of the same divergent loop spends five or six on exit masks
// (the kernel issued 0.72 scalar instructions per vector instruction before; PMC r01_k).

// continues the ordered insert of key `cur` whose first probe at slot h returned `o`
// (o == 0: slot was empty -> done; o == cur: already present -> done; o < cur: displaced o, carry
// it on; o > cur: keep cur and move on).  keys_lds = LDS byte offset of the key table.
__device__ __forceinline__ void rj_insert_chain(uint32_t keys_lds, uint32_t cur, uint32_t o, uint32_t h, uint32_t smask) {
  uint32_t addr;
  unsigned long long sv;
  asm volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "v_cmpx_ne_u32_e32 vcc, 0, %[cur]\n\t"       // lanes without a record never probe on
      "v_cmpx_ne_u32_e32 vcc, 0, %[o]\n\t"
      "v_cmpx_ne_u32_e32 vcc, %[o], %[cur]\n\t"
      "s_cbranch_execz 2f\n"
      "1:\n\t"
      "v_min_u32_e32 %[cur], %[o], %[cur]\n\t"
      "v_add_u32_e32 %[h], 1, %[h]\n\t"
      "v_and_b32_e32 %[h], %[smask], %[h]\n\t"
      "v_lshl_add_u32 %[addr], %[h], 2, %[base]\n\t"
      "ds_max_rtn_u32 %[o], %[addr], %[cur]\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmpx_ne_u32_e32 vcc, 0, %[o]\n\t"
      "v_cmpx_ne_u32_e32 vcc, %[o], %[cur]\n\t"
      "s_cbranch_execnz 1b\n"
      "2:\n\t"
      "s_mov_b64 exec, %[sv]"
      : [cur] "+v"(cur), [o] "+v"(o), [h] "+v"(h), [addr] "=&v"(addr), [sv] "=&s"(sv)
      : [smask] "s"(smask), [base] "s"(keys_lds)
      : "vcc", "memory");
}

// slot of key k on its probe path: larger keys sit in front of it.  kk = value of the first probe
// (pass 0 for a lane without a record).  Returns the slot where the walk stopped and, in kk, what
// it holds there: kk == k -> found.
__device__ __forceinline__ uint32_t rj_find_chain(uint32_t keys_lds, uint32_t k, uint32_t& kk, uint32_t h, uint32_t smask) {
  uint32_t addr;
  unsigned long long sv;
  asm volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "v_cmpx_gt_u32_e32 vcc, %[kk], %[k]\n\t"
      "s_cbranch_execz 2f\n"
      "1:\n\t"
      "v_add_u32_e32 %[h], 1, %[h]\n\t"
      "v_and_b32_e32 %[h], %[smask], %[h]\n\t"
      "v_lshl_add_u32 %[addr], %[h], 2, %[base]\n\t"
      "ds_read_b32 %[kk], %[addr]\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmpx_gt_u32_e32 vcc, %[kk], %[k]\n\t"
      "s_cbranch_execnz 1b\n"
      "2:\n\t"
      "s_mov_b64 exec, %[sv]"
      : [kk] "+v"(kk), [h] "+v"(h), [addr] "=&v"(addr), [sv] "=&s"(sv)
      : [k] "v"(k), [smask] "s"(smask), [base] "s"(keys_lds)
      : "vcc", "memory");
  return h;
}

// Occupancy the register allocator aims for: 256- and 512-thread rows keep 8 waves per SIMD (64
// VGPRs); 1024-thread rows with 8 / 16 pixel slots per thread (W > 4096: one workgroup per CU) get
// the 128 registers their 16 waves leave them.
template <int SPT, int NT>
struct RjOcc {
  static constexpr int kWaves = (SPT >= 8) ? 4 : 8;
};

// VIRT (k_partition.h): the "rows" are partitions of the non-epipolar matcher -- dense record arrays (code, pixel
// index) of a contiguous code range per side instead of two image rows; a record's "x" is its position in the
// partition, the disparity filter looks the pixel indices up, and results go to the partition's stretch of v.staged.
struct RjVirt {
  const uint2* kv;        // [npairs][recs]: records (code, pixel index y * W + x), side s of a pair at + s * (recs / 2).  One
                          // 8-byte element per record: the scatter that writes them leaves runs of ~5 records per bin and
                          // tile, and two 4-byte arrays made that twice as many partial cache lines (k_partition.h)
  int32_t* part;          // per pair (stride ps ints): cursors, partition offsets, match counts, misc (GpLayout)
  uint32_t* staged;       // [npairs][recs / 2] uint2: (left, right) pixel index of a partition's matches at its left offset
  long recs, ps;
  int o_off, o_rowcnt, o_misc, pmax;
  GpcDivW dw;
  int vtol;
  int use_list;           // 1: workgroup b takes partition part[o_misc + 8 + b] (the plan's list of over-large partitions: the grid
                          // of the 8192-record launch is that list, not every partition of which nearly all return at once --
                          // dispatching ~8000 workgroups of 128 KiB of LDS each cost 44-48 us per 8 pairs of 1920x1080)
  int min_recs;           // this launch takes the partitions with more than min_recs records on a side (and at most NT*SPT):
                          // the few bins that are large by themselves go to the 8192-slot instantiation, the rest to the 4096 one
};

// (The persistent variant that also writes the supports -- join + output in one launch -- is a kernel of its own:
// k_rowjoin_fused.h.)

// codes:   [npairs*2][H][W]   (image 2p = left, 2p+1 = right)
// cand:    [npairs*2][H][W]   candidate bytes (grad, or the caller's scattered mask): WIDE only
// staged:  [npairs][H][W]     packed (xL | xR<<16), first rowcnt entries of each row valid
// rowcnt:  [npairs][H]
// grid: (ceil((H - 26) / rpw), npairs); NT threads, NB = NT*SPT >= W; table of S = 1 << log2s slots,
//       S >= NB, S >= 2*(W-26) where the LDS allows it (only left codes are inserted: load factor
//       <= 0.5; rows beyond 8218 px fill a 16384-slot table up to W-26 / 16384 < 1)
// dynamic LDS: 8*(S+1) bytes  (16 KiB for W = 1024: 8 workgroups per CU = 32 waves, 64 VGPRs)
// Wide rows use more threads per row before more pixel slots per thread, so that the one
// or two workgroups that fit a CU (98 KiB of table at W = 3840) still fill its SIMDs.
template <int SPT, int NT, bool WIDE, bool VIRT = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RjOcc<SPT, NT>::kWaves, 8))) void k_row_join(
    const uint32_t* __restrict__ codes, const uint8_t* __restrict__ cand, int W, int H, int disp_high, int apply_filter,
    const int32_t* __restrict__ img_stats, uint32_t* __restrict__ staged, int32_t* __restrict__ rowcnt,
    int log2s, int rpw, RjVirt v) {
#define RJ_SEQ 0
#include "k_rowjoin_body.h"
#undef RJ_SEQ
}

// The same join over a frame sequence: codes / cand [nframes][H][W], pair p = (frame p, frame p + 1); img_stats in the
// pair layout [npairs*2] as for k_row_join (k_seq_stats).  grid (H - 26, nframes - 1).  VIRT is not instantiated.
template <int SPT, int NT, bool WIDE, bool VIRT = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RjOcc<SPT, NT>::kWaves, 8))) void k_row_join_seq(
    const uint32_t* __restrict__ codes, const uint8_t* __restrict__ cand, int W, int H, int disp_high, int apply_filter,
    const int32_t* __restrict__ img_stats, uint32_t* __restrict__ staged, int32_t* __restrict__ rowcnt,
    int log2s, int rpw, RjVirt v) {
#define RJ_SEQ 1
#include "k_rowjoin_body.h"
#undef RJ_SEQ
}

}  // namespace gpc
