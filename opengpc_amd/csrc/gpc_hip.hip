// gpc_hip.hip -- host side of libgpc_hip.so: context, workspaces, launches, C ABI.
//
// gfx950 only.  No CPU fallback: every entry point needs a live HIP device.
#include "../../include/gpc_hip.h"

#include <hip/hip_runtime.h>

#if defined(__SSE2__)
#include <emmintrin.h>   // the host expansion of packed results has an SSE2 path (x86 hosts); scalar otherwise
#endif
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <map>
#include <memory>
#include <utility>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "aggregate_host.h"
#include "clean_host.h"
#include "dense_host.h"
#include "field_score_host.h"
#include "gapfill_host.h"
#include "gpc_device.h"
#include "inpaint_host.h"
#include "k_aggregate.h"
#include "k_clean.h"
#include "k_consensus.h"
#include "k_dense.h"
#include "k_extract.h"
#include "k_field_score.h"
#include "k_gapfill.h"
#include "k_global.h"
#include "k_hash.h"
#include "k_hashtable.h"
#include "k_htjoin.h"
#include "k_inpaint.h"
#include "k_partition.h"
#include "k_preprocess.h"
#include "k_propagate.h"
#include "k_pyramid.h"
#include "k_quad.h"
#include "k_refine.h"
#include "k_rowjoin.h"
#include "k_rowjoin_fused.h"
#include "k_rows.h"
#include "k_score.h"
#include "k_search.h"
#include "k_track.h"
#include "k_track_stream.h"
#include "k_train.h"
#include "k_train_forest.h"
#include "k_union.h"
#include "owners.h"
#include "propagate_host.h"
#include "pyramid_host.h"
#include "search_host.h"
#include "track_stream_host.h"

// Eight sections of the host code below are cut out at their rules into files of their own, csrc/host_*.h, and included where
// they stood: host_staging.h (what scoring, tracks and the stages after them share), host_consensus.h, host_refine.h,
// host_pyramid.h, host_dense.h, host_quads.h, host_clean.h, host_inpaint.h and host_field_score.h (host_search.h, host_aggregate.h, host_propagate.h and host_gapfill.h came between).  They are parts of THIS translation unit, not self-contained headers: each needs what
// stands above its include, and `#pragma once` is all the guard it has.  Each says its linkage once: an anonymous namespace
// with its types, helpers and templates, then one extern "C" block with its entry points.  Everything else is still here.

namespace {

enum KernelId {
  KID_PREPROCESS = 0,
  KID_HASH,
  KID_ROW_JOIN,
  KID_GATHER_ROWS,
  KID_MASK,
  KID_GLOBAL_KEYS,
  KID_GLOBAL_SORT,
  KID_GLOBAL_MATCH,
  KID_TRAIN_EVAL,
  KID_GROUP_UNION,
  KID_TRACK_FILL,
  KID_TRACK_SCATTER,
  KID_TRACK_LINK,
  KID_TRACK_SETTLE,
  KID_TRACK_SCAN,
  KID_TRACK_WALK,
  KID_CONS_CELLS,
  KID_CONS_SCAN,
  KID_CONS_SCATTER,
  KID_CONS_COUNT,
  KID_CONS_BLOCKS,
  KID_CONS_WRITE,
  KID_TRS_FILL,
  KID_TRS_SCATTER,
  KID_TRS_LINK,
  KID_TRS_SETTLE,
  KID_TRS_SCAN,
  KID_TRS_WALK,
  KID_TRS_SAVE,
  KID_TRS_NCAND,
  KID_SCORE_RECORDS,
  KID_SCORE_MATCHABLE,
  KID_SEARCH,
  KID_REFINE,
  KID_PYR_DOWN,
  KID_PYR_KEEP,
  KID_PYR_SCAN,
  KID_PYR_WRITE,
  KID_DENSE_CLAIM,
  KID_DENSE_PULL,
  KID_DENSE_TOP,
  KID_DENSE_PUSH,
  KID_TF_BEGIN,
  KID_TF_EVAL,
  KID_TF_TOT,
  KID_TF_COMMIT,
  KID_INPAINT_BEGIN,
  KID_INPAINT_PASS,
  KID_QUAD_SIDES,
  KID_QUAD_FILL,
  KID_QUAD_SCATTER,
  KID_QUAD_CLOSE,
  KID_QUAD_SETTLE,
  KID_QUAD_SCAN,
  KID_QUAD_WRITE,
  KID_CLEAN_FLIP,
  KID_CLEAN_CHECK,
  KID_CLEAN_TILE,
  KID_CLEAN_BORDER,
  KID_CLEAN_FLATTEN,
  KID_CLEAN_SIZES,
  KID_CLEAN_APPLY,
  KID_COUNT
};
const char* const kKernelNames[KID_COUNT] = {
    "k_preprocess", "k_hash", "k_row_join", "k_gather_rows",
    "k_mask", "k_global_keys", "k_global_sort", "k_global_match", "k_train_eval", "k_group_union",
    "k_track_fill", "k_track_scatter", "k_track_link", "k_track_settle", "k_track_scan", "k_track_walk",
    "k_cons_cells", "k_cons_scan", "k_cons_scatter", "k_cons_count", "k_cons_blocks", "k_cons_write",
    "k_trs_fill", "k_trs_scatter", "k_trs_link", "k_trs_settle", "k_trs_scan", "k_trs_walk", "k_trs_save", "k_trs_ncand",
    "k_score_records", "k_score_matchable", "k_search", "k_refine", "k_pyr_down", "k_pyr_keep", "k_pyr_scan", "k_pyr_write",
    "k_dense_claim", "k_dense_pull", "k_dense_top", "k_dense_push",
    "k_tf_begin", "k_tf_eval", "k_tf_tot", "k_tf_commit",
    "k_inpaint_begin", "k_inpaint_pass",
    "k_quad_sides", "k_quad_fill", "k_quad_scatter", "k_quad_close", "k_quad_settle", "k_quad_scan", "k_quad_write",
    "k_clean_flip", "k_clean_check", "k_clean_tile", "k_clean_border", "k_clean_flatten", "k_clean_sizes", "k_clean_apply"};

// The owners of owners.h over the HIP runtime.  Everything the library allocates passes through these four backends, which
// also keep the process-wide counts that gpc_hip_debug_live_resources reports.
std::atomic<uint64_t> g_live[4];  // device blocks, device bytes, page-locked blocks, streams + events
struct DevMem {
  using status = hipError_t;
  static hipError_t alloc(void** p, size_t bytes, unsigned) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) ++g_live[0], g_live[1] += bytes;
    return e;
  }
  static hipError_t release(void* p, size_t bytes) {
    --g_live[0], g_live[1] -= bytes;
    return hipFree(p);
  }
};
struct PinnedMem {
  using status = hipError_t;
  static hipError_t alloc(void** p, size_t bytes, unsigned flags) {
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e == hipSuccess) ++g_live[2];
    return e;
  }
  static hipError_t release(void* p, size_t) {
    --g_live[2];
    return hipHostFree(p);
  }
};
struct StreamApi {
  using handle = hipStream_t;
  using status = hipError_t;
  static hipError_t create(hipStream_t* s, unsigned flags) {
    const hipError_t e = hipStreamCreateWithFlags(s, flags);
    if (e == hipSuccess) ++g_live[3];
    return e;
  }
  static hipError_t destroy(hipStream_t s) {
    --g_live[3];
    return hipStreamDestroy(s);
  }
};
struct EventApi {
  using handle = hipEvent_t;
  using status = hipError_t;
  static hipError_t create(hipEvent_t* ev, unsigned flags) {
    const hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) ++g_live[3];
    return e;
  }
  static hipError_t destroy(hipEvent_t ev) {
    --g_live[3];
    return hipEventDestroy(ev);
  }
};
template <class T>
using DevBlock = gpc::Block<DevMem, T>;
using DevBuf = DevBlock<void>;
template <class T>
using Pinned = gpc::Block<PinnedMem, T>;
using Stream = gpc::Handle<StreamApi>;
using Event = gpc::Handle<EventApi>;

struct TimedSpan {
  Event a, b;
  int kid;
};

// where run_match puts PACKED results (k_gather_rows mode 2): words between the pairs' arrays
struct PackedOut {
  int32_t* rows = nullptr;
  long packed_stride = 0, rows_stride = 0;  // words between the pairs' arrays
  int32_t* totals = nullptr;                // non-null: scratch [npairs]; the pairs' records are then written back to back
};

// Host threads that expand packed results (gpc_hip_expand_packed) into the caller's gpc_support arrays while the
// next chunk is on the link.  Jobs carry the index of the staging slot they read; wait_slot() blocks until every
// job of a slot is done, so the slot can be overwritten.
struct ExpandJob {
  const uint32_t* packed;
  const int32_t* rows;
  int H, y0, y1, first, limit;  // rows [y0, y1) of a pair whose supports start at index `first`; stop at `limit`
  gpc_support* out;
  int slot;
  // a plain copy instead (pageable input images into the page-locked bounce buffer of their chunk): copy_bytes > 0
  const void* copy_src = nullptr;
  void* copy_dst = nullptr;
  size_t copy_bytes = 0;
};

class ExpandPool {
 public:
  ~ExpandPool() { stop(); }
  // bind: CPUs the workers may run on (the NUMA node of the GPU: the page-locked buffers they read and write live there,
  // and workers that land on the other socket made the same call take 7.3 instead of 5.4 ms); null = wherever
  // bind: the CPUs of the GPU's NUMA node.  groups: the same CPUs by last-level cache (one set per CCD): worker i is held on
  // group i mod n.  Left to the scheduler, workers woken by one thread are placed on idle CPUs of the WAKER's cache domain --
  // all eight on one CCD, whose link to the memory controllers then carries every record they write: the same 256-pair call
  // took 8.5 ms instead of 5.3 (profiles/r05_g_bench.json against r05_e: worker CPUs 64-71 + their SMT siblings).
  void start(int nthreads, const cpu_set_t* bind, const std::vector<cpu_set_t>* groups = nullptr) {
    if ((int)threads_.size() == nthreads) return;
    stop();
    quit_ = false;
    have_bind_ = bind != nullptr;
    if (bind) bind_ = *bind;
    groups_.clear();
    if (bind && groups) groups_ = *groups;
    cpus_.assign((size_t)nthreads, -1);
    started_ = 0;
    for (int i = 0; i < nthreads; ++i)
      threads_.emplace_back([this, i] {
        if (!groups_.empty()) (void)sched_setaffinity(0, sizeof(cpu_set_t), &groups_[(size_t)i % groups_.size()]);
        else if (have_bind_) (void)sched_setaffinity(0, sizeof bind_, &bind_);
        run(i);
      });
    // every worker has reported the CPU it starts on: worker_cpus() has an entry for a worker that is never handed a job
    // (with eight workers about one call in four of 32 pairs leaves one idle)
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [&] { return started_ == nthreads; });
  }
  void stop() {
    {
      std::lock_guard<std::mutex> g(m_);
      quit_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
    threads_.clear();
  }
  void push(const ExpandJob& j) {
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back(j);
      ++pending_[j.slot & 7];
    }
    cv_.notify_one();
  }
  void wait_slot(int slot) {
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [&] { return pending_[slot & 7] == 0; });
  }
  void wait_all() {
    for (int s = 0; s < 8; ++s) wait_slot(s);
  }
  int size() const { return (int)threads_.size(); }
  // the CPU every worker started on or last ran a job on (diagnostics: gpc_hip_host_worker_cpus)
  int worker_cpus(int* out, int cap) {
    std::lock_guard<std::mutex> g(m_);
    int n = 0;
    for (size_t i = 0; i < cpus_.size() && n < cap; ++i) out[n++] = cpus_[i];
    return (int)cpus_.size();
  }

 private:
  void run(int index);
  std::vector<std::thread> threads_;
  std::vector<int> cpus_;
  std::deque<ExpandJob> q_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  int pending_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int started_ = 0;
  bool quit_ = false;
  bool have_bind_ = false;
  cpu_set_t bind_;
  std::vector<cpu_set_t> groups_;
};

}  // namespace

// Who frees what: every block, stream and event below is an owner (owners.h) and goes when the context is deleted, in
// reverse order of declaration -- no list to extend.  The order that matters is kept by gpc_hip_destroy and by where
// own_stream stands: gpc_hip_destroy waits for `stream` and for every stream the context made before `delete` frees a
// block; it stops the expansion pool, whose workers read and write the page-locked blocks, before `delete` frees those;
// own_stream is the first owner declared, so it is destroyed last.
struct gpc_hip_ctx {
  int device = 0;
  Stream own_stream;
  hipStream_t stream = nullptr;   // own_stream or the caller's (gpc_hip_set_stream): not owned
  // gpc_hip_match_batch: upload / download streams and the events that chain a chunk's stages
  Stream s_in, s_out, s_cnt;
  Stream s_aux;                   // the non-epipolar matcher's launch for over-large partitions runs beside the main one
  Event e_fork, e_join;
  Event e_flag;                   // the device-wide matchers' plan words have arrived on the host
  Event e_in[4], e_comp[4], e_cnt[4], e_out[4];
  DevBuf packed;                  // packed results of the chunks in flight (3 slots)
  Pinned<void> h_stage;           // page-locked landing area of packed results (4 slots)
  Pinned<void> h_in;              // page-locked bounce buffer for PAGEABLE input images (2 slots x 2 sides x a chunk)
  Pinned<int32_t> h_cnt;          // page-locked landing area of counts [npairs] + candidate counts [npairs][2]: a copy to the
                                  // caller's (pageable) arrays would block the host until the chunk's kernels are done
  ExpandPool pool;
  // host clock at the stages of the last gpc_hip_match_batch / _packed call, ms since its entry (gpc_hip_batch_stages):
  // [0] last upload seen complete, [1] last chunk's kernels done (its counts have arrived), [2] last chunk of packed
  // records has landed in host memory, [3] expansion / delivery done (the call returns)
  float stage_ms[4] = {0.f, 0.f, 0.f, 0.f};
  bool grad_is_bits = false;      // c->grad holds k_preprocess's bit image (set by run_preprocess, read by run_hash)
  bool no_grad_bits = false;      // GPC_HIP_NO_GRAD_BITS: the batched pipelines keep the byte image (A/B checks)
  int upload_mode = 1;            // GPC_HIP_UPLOAD: single-pair host path -- 0: hipMemcpyAsync per side, 1: one k_upload2 launch, 2: k_preprocess reads the host's pages
  int direct_max = 2;             // GPC_HIP_DIRECT_MAX: batches up to this size with a page-locked `out` are written by the
                                  // kernels straight into the caller's array (no packed records, no host expansion); 0 = never
  bool have_node_cpus = false;    // CPUs of the NUMA node this GPU hangs off (from sysfs), within the process's affinity mask
  cpu_set_t node_cpus;
  std::vector<cpu_set_t> node_l3;  // node_cpus by last-level cache (CCD): the expansion workers are dealt over these
  int numa_node = -1;
  // Two lanes (gpc_hip_set_pipeline): consecutive device-resident batch calls alternate between two sets of workspaces on
  // two streams of the context's own, wired with events so that batch k+1's k_preprocess and k_hash run beside batch k's
  // join (which then takes one workgroup per CU less: a wave slot per SIMD stays free for them).  A lane is SWAPPED INTO
  // the members below for the duration of a call (LaneScope), so every run_* function works on it unchanged.
  struct Lane {
    Stream s;
    Event e_in, e_hash, e_join;
    DevBuf smooth, grad, codes, stats, jstate, staged, rowcnt;
    size_t jstate_granules = 0;
    uint32_t join_epoch = 0;
    bool grad_is_bits = false, used = false;
  };
  Lane lanes[2];
  int pipeline = 1, next_lane = 0;
  // experiment hooks (gpc_hip_debug_pipeline_events, tools/overlap_experiment.py; all null in the product): events the
  // device-resident batch call waits for before k_preprocess / between k_preprocess and k_hash, and records after k_hash /
  // after the join -- enough to let one batch's k_preprocess run beside the previous batch's join and nothing else
  hipEvent_t dbg_wait_pre = nullptr, dbg_wait_hash = nullptr, dbg_rec_hash = nullptr, dbg_rec_join = nullptr;
  bool no_pair_packed = false;    // GPC_HIP_NO_PAIR_PACKED: the two-step forms deliver 12-byte records over the link (A/B checks)
  bool no_feeder = false;         // GPC_HIP_NO_FEEDER: the chunk pipeline always runs on the calling thread (A/B checks)
  int fed_calls = 0;              // batch calls that ran on a feeder thread (gpc_hip_fed_calls)
  int chunk_pairs = 0;            // GPC_HIP_CHUNK: pairs per chunk of gpc_hip_match_batch (tuning)
  int expand_threads = 0;         // GPC_HIP_EXPAND_THREADS (tuning)
  char err[256] = {0};

  bool naive = false;  // gpc_hip_set_arithmetic: the reference's SSE=OFF (*Naive) arithmetic
  bool have_forest = false;
  GpcForestDev forest;        // tests in file order (SSE bit placement)
  GpcForestDev forest_naive;  // tests reversed: slot u = test T-1-u lands on bit u (MSB-first codes), raw int tau
  int forest_w = 0, forest_h = 0;
  gpc_filter_mask forest_src;  // what gpc_hip_set_forest was last given: the same forest again costs nothing
  // group mode (gpc_hip_set_forest_groups with more than one group; gpc_hip_set_forest leaves it): the hash kernel runs
  // every group's tests (k_hash_groups), the joins run over virtual pairs p * ngroups + g, k_group_union unites them
  int ngroups = 0;             // 0 outside group mode
  int gmax_tests = 0;          // the largest group (code_bits, wide_codes)
  bool gtau = false;           // one of the groups has a nonzero tau
  DevBuf gforest_dev;          // [3][GPC_MAX_GROUPS] GpcForestDev: SSE order, Naive order, SSE with the tall tile's offsets
  DevBuf vstats, vcand, vout, vcnt, vncand, uplane, ublk, gdense;  // virtual-pair statistics / candidates / results, union state
  // match-and-score, match-and-filter (all_records): every record of every pair of the call and their counts
  DevBuf all_rec, all_cnt;
  // the host forms of scoring, tracks and filtering (Stage): what a call or a chunk of it sends up and brings down; the
  // copies that read a piece of the transfer arena are done
  DevBuf stage;
  Event e_stage[2];
  // point tracks (gpc_hip_track_*): per-pixel planes of pairs 1 .. P-1, predecessor per record, head counts per chunk
  DevBuf tr_plane, tr_pred, tr_blk;
  // match filtering (gpc_hip_consensus_*): class and record index per sorted position, cursors and first positions per pair
  // and grid cell, kept records per chunk, the keep mask where the caller wants none
  DevBuf cs_key, cs_idx, cs_cur, cs_start, cs_blk, cs_keep;
  // pyramid matching (gpc_hip_pyramid_*): the raw images of levels 1 .. L-1, every record and the counts of every level, the
  // occupancy bit planes, keep bits and chunk counts of the merge
  DevBuf py_img, py_rec, py_cnt, py_plane, py_flags, py_blk;
  // densifying (gpc_hip_densify_*): the owner plane, the counts and the sums of the cell pyramid, the refinements of the
  // match-and-fill forms
  DevBuf dn_owner, dn_n, dn_s, dn_ref;
  // cleaning fields (gpc_hip_clean_*): the sizes of the components (the labels live in dn_owner or in the caller's plane); the
  // forward field where the caller of a match-fill-and-clean form wants none, and the backward field
  DevBuf cl_size, cl_fwd, cl_bwd;
  // completing fields (gpc_hip_inpaint_*): the pass plane where the caller passes none; the control words (pixels filled per
  // pass, stats where the caller passes none, holes per tile)
  DevBuf ip_pass, ip_ctl;
  // aggregating the search's costs (gpc_hip_aggregate_*): the cost volume of a group of pairs, then its path volumes
  DevBuf ag_ws;
  int64_t agg_group_bytes = AG_GROUP_BYTES;  // GPC_HIP_AGG_GROUP_BYTES: what the volumes of one group of pairs may take (tests)
  // propagating field values between neighbours (gpc_hip_propagate_*): the other field of the iterations' ping-pong
  DevBuf pg_ws;
  // closing holes along scanlines (gpc_hip_gapfill_*): the four planes of distances to the ends of a hole's runs
  DevBuf gf_ws;
  // quads over a stereo sequence (gpc_hip_quads_*): the per-pixel planes of a group of steps followed by its owner words
  // (one fill covers both), the candidate i' per support slot, the quad counts per chunk; the image-major copies of the
  // statistics words, code images and (32-bit codes) candidate bytes of each side, which the two flow joins of
  // gpc_hip_match_stereo_sequence_device read
  DevBuf qd_plane, qd_sel, qd_blk, qd_stats, qd_codes[2], qd_gcand[2];
  int quad_steps = 0;         // GPC_HIP_QUAD_STEPS: steps per group of the closing (tests; default: what QD_PLANE_BYTES holds)
  DevBuf sstats;  // frame sequences: the frames' statistics expanded into the pair layout [npairs*2] (k_seq_stats)

  // workspaces
  DevBuf raw, smooth, grad, candmap, codes, staged, rowcnt, stats, out, counts, ncand, mask;
  DevBuf gkv;  // records (code, pixel index) of the partitioned device-wide matchers, by bin
  DevBuf gkeys[2], gvals[2], ghist, gmisc, hkeys[2], hvals[2], hrec;
  DevBuf gpart;       // partition plan of the non-epipolar matcher (k_partition.h) + one overflow word for the batch
  Pinned<int32_t> h_flag;     // page-locked landing word of that overflow flag
  int no_partition = 0;       // GPC_HIP_NO_PARTITION: always take the radix-sort path (A/B checks)
  int rows_per_chunk = 16;    // GPC_HIP_ROWS_PER_CHUNK: rows one partition workgroup scatters (A/B checks)
  int gp_log2bins = 0;        // GPC_HIP_GP_LOG2BINS = 8 .. 11: force the number of code-range bins (A/B checks)
  int ht_hint_w = 0, ht_hint_h = 0, ht_hint_lbits = 0;  // what the hash-table planner ended on for the last image size: where it starts next time
  bool ht_no_half = false;    // GPC_HIP_HT_NO_HALF: never the 512-thread k_ht_join (A/B checks)
  int ht_mid = 0;             // GPC_HIP_HT_MID = 10 .. 64: force HtjArgs::mid (A/B checks; 10 = one wave per bucket beyond ten records)
  int ht_lbits = 0;           // GPC_HIP_HT_LBITS = 7 .. 10: force the buckets per bin of the hash-table matcher (A/B checks)
  int gp_target = 2000;       // GPC_HIP_GP_TARGET: records per side a partition of the non-epipolar matcher aims at. Per 32 pairs of
                              // 1024x436, join + gather: 1400 -> 208 us, 1800 -> 189, 2000 / 2200 -> 182, 2600 -> 192, 3000 -> 208
  int flat_chunks = 0;        // GPC_HIP_FLAT_CHUNKS: gpc_hip_match_batch with equal chunks only (A/B checks)
  DevBuf forest_dev;  // [0] = forest, [1] = forest_naive, [2] = forest with the tall tile's offsets: the hash kernel reads its tests from here (scalar loads)
  int hash_tall = -1;  // GPC_HIP_HASH_TALL = 0 | 1: never / always the 40-row tile where it exists (tests, A/B checks); default: by rounds

  // fused join + output (k_rowjoin.h, FUSE): ticket counters + look-back granules, launch epoch, error word
  DevBuf jstate;
  size_t jstate_granules = 0;
  uint32_t join_epoch = 0;
  Pinned<int32_t> h_err;      // page-locked, device-visible: a look-back of the fused join timed out
  int32_t* d_err = nullptr;   // the device's address of that word (a view of h_err)
  int no_fuse = 0;            // GPC_HIP_NO_FUSE: join + k_gather_rows as two launches (A/B checks)
  int fuse_always = 0;        // GPC_HIP_FUSE_ALWAYS: the fused join wherever it is possible, however small the launch (tests, A/B checks)
  int fuse_wgs = 0;           // GPC_HIP_FUSE_WGS: workgroups of the persistent join (tuning; default = what the device holds)
  int fuse_min_pairs = 1;     // GPC_HIP_FUSE_MIN_PAIRS: smaller batches take the two-launch path
  int pre_rows = 0;           // GPC_HIP_PRE_ROWS = 14 | 6 | 2: that strip height of k_preprocess whatever the launch's size (tests)
  int fuse_shards = 0;        // GPC_HIP_FUSE_SHARDS: ticket counters the pairs are dealt over (0: join_shards() chooses)
  int num_cus = 0;
  std::map<std::pair<const void*, size_t>, int> wgs_per_cu;  // occupancy of the persistent instantiations launched so far, per LDS size
  std::map<const void*, int> dyn_lds;     // largest dynamic-LDS size a kernel has been allowed so far (hipFuncSetAttribute once, not per call)

  int hash_tpw = 0;    // GPC_HIP_HASH_TPW: tiles per workgroup of the hash kernel (tuning)
  int32_t hash_plan[4] = {0, 0, 0, 0};  // {ty, tpw, grid.y, last_from} of the last run_hash (gpc_hip_hash_plan); ty = 0: none yet
  int join_nt = 0;     // GPC_HIP_JOIN_NT = 256 | 512 | 1024: force the join kernel's threads per row (tuning)

  // rocprof name of the instantiation last launched under each timing slot (bench.py reports it)
  char launch_name[KID_COUNT][96] = {{0}};

  // timing
  bool timing = false;
  unsigned timing_mask = 0xFFFFFFFFu;  // which KernelIds are bracketed by events when timing is on
  std::vector<TimedSpan> spans;
  std::vector<TimedSpan> free_spans;

  std::vector<gpc_hip_train_set*> train_sets;  // training sets created on this context
  std::vector<gpc_hip_track_stream*> track_streams;  // track streams created on this context
  uint64_t code_gen = 1;  // counts the changes of forest and arithmetic: codes hashed under another value are not comparable
  // gpc_hip_extract_triplets: raw (host entry only), smooth and grad of one chunk of frame pairs, the chunk's column groups
  // (allocated by the call, released before it returns)
  DevBuf ext_raw, ext_smooth, ext_grad, ext_groups;
  int extract_frames = 0;     // GPC_HIP_EXTRACT_FRAMES: frame pairs per chunk (tests; default: 64 MiB of smoothed frames)
  int train_group = 0;        // GPC_HIP_TRAIN_GROUP: ferns per group of gpc_hip_train_forest (tests; default: what grid and workspace allow)
  int seq_frames = 0;         // GPC_HIP_SEQ_FRAMES: frames per chunk of gpc_hip_match_sequence (tests; default 16)

  // Forest::preprocessImage -> Forest::rectifiedMatch without the round trip (the reference's PreprocessedImage travels by
  // value through host memory, inference.hpp:161-165): the last two preprocessed images stay on the device beside the
  // host copies the caller received; a match call whose host arrays are recognised as those copies (resident_slot) skips
  // the upload.  Guarded by g_res_mu: a preprocess call of ANY context that writes over a recorded host array drops the record.
  struct Resident {
    bool valid = false;
    const uint8_t *smooth = nullptr, *grad = nullptr;
    const int32_t* mask = nullptr;
    int n_mask = 0, W = 0, H = 0;
    bool naive = false;
    uint64_t fp = 0;  // fingerprint of the three host arrays as delivered
  };
  Resident res[2];
  int res_next = 0;
  DevBuf res_smooth, res_grad;  // [2][H][W] bytes each
  size_t res_n = 0;             // bytes per slot
  int resident_mode = 1;        // GPC_HIP_RESIDENT = 0: never; 1: pointers + sizes + sampled fingerprint; 2: + every byte hashed
  int resident_hits = 0;        // match calls served from the device-resident images (gpc_hip_resident_hits)
  // Page-locked transfer arena of the host-buffer entry points.  The caller's arrays (std::vector, ndb::Buffer, numpy:
  // pageable) never reach hipMemcpy: the runtime pins such memory for the copy and KEEPS the pinning cached, and when the
  // caller later frees the array the driver must suspend and restore the process's queues to drop it -- the next
  // submission then waits ~27 ms (measured: profiles/r05_a_cold_start.txt).  So pageable memory is copied by CPU threads
  // into / out of this arena, and the device reads / writes the arena over the link.
  Pinned<uint8_t> h_xfer;
  // page-locked staging of gpc_hip_preprocess_begin / _fetch: [raw | smooth | grad | mask | count]
  Pinned<uint8_t> h_pre;
  int pre_slot = -1, pre_W = 0, pre_H = 0;  // what _begin left for _fetch
  bool pre_have_mask = false;
  Event e_pre;                  // smooth and grad of that image have landed in the staging block
  // what gpc_hip_*_match_begin left for gpc_hip_match_fetch: results in the transfer arena (or, `direct`, already in the
  // caller's page-locked array), the count and the candidate counts in h_cnt[0 .. 2]
  struct PendingMatch {
    bool active = false, direct = false, have_ncand = false;
    void* dev_out = nullptr;  // group mode: the union's records are in device memory (c->gdense), cap_dev of them at most
    bool packed = false;   // the arena holds [H row counts | cap_dev words xL | xR << 16] (epipolar sort-matcher): 4 bytes
                           // per support over the link instead of 12, expanded into the caller's array by the workers
    size_t esz = 0;
    int cap_dev = 0, H = 0;
  } pend;
  bool debug = false;           // GPC_HIP_DEBUG: launch geometry on stderr
  bool debug_plan = false;      // GPC_HIP_DEBUG_PLAN: the hash-table planner's choice on stderr
};

struct gpc_hip_train_set {
  gpc_hip_ctx* owner = nullptr;
  int n = 0;
  long np = 0;                // n rounded up to a multiple of 256
  DevBlock<uint8_t> planes;   // [3][729][np]
  DevBlock<uint8_t> flags;    // [np]
  DevBlock<int32_t> counts;   // scratch: tp/fp per (candidate, tau) + tot
  DevBlock<gpc::GpcSplit> d_cand;
  std::vector<int32_t> h_counts;  // host staging of the counters
};

namespace {

// every live context (gpc_hip_create .. gpc_hip_destroy) and the lock of their Resident records
std::mutex g_res_mu;
std::vector<gpc_hip_ctx*> g_ctxs;

#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call,        \
               hipGetErrorString(e_), __FILE__, __LINE__);                             \
      return GPC_E_HIP;                                                                \
    }                                                                                  \
  } while (0)

#define CHK(expr)                  \
  do {                             \
    int s_ = (expr);               \
    if (s_ != GPC_OK) return s_;   \
  } while (0)

double host_ms() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

template <class T>
int ensure(gpc_hip_ctx* c, DevBlock<T>& b, size_t bytes) {
  if (bytes <= b.cap) return GPC_OK;
  if (b.p) HIPCHK(c, hipStreamSynchronize(c->stream));
  // slack: growth without reallocation, and the fused join reads whole pixel-slot rows (up to 16 KiB past a row's end)
  HIPCHK(c, b.alloc(bytes + bytes / 8 + 65536));
  return GPC_OK;
}

// a page-locked block of exactly `want` bytes in place of the old one.  Waits for nothing: the caller does where the device
// may still use the old block, and decides when to grow and by how much.
template <class T>
int ensure_pinned(gpc_hip_ctx* c, Pinned<T>& b, size_t want) {
  HIPCHK(c, b.alloc(want, hipHostMallocDefault));
  return GPC_OK;
}

struct Timed {
  gpc_hip_ctx* c;
  TimedSpan s;
  bool on;
  // (the mask has 32 bits: a kernel of index 32 or above is bracketed whenever timing is on)
  Timed(gpc_hip_ctx* ctx, int kid) : c(ctx), on(ctx->timing && (kid >= 32 || ((ctx->timing_mask >> kid) & 1u))) {
    if (!on) return;
    if (!c->free_spans.empty()) {
      s = std::move(c->free_spans.back());
      c->free_spans.pop_back();
    } else {
      if (s.a.create(hipEventDefault) != hipSuccess || s.b.create(hipEventDefault) != hipSuccess) {
        on = false;
        return;
      }
    }
    s.kid = kid;
    (void)hipEventRecord(s.a, c->stream);
  }
  ~Timed() {
    if (!on) return;
    (void)hipEventRecord(s.b, c->stream);
    c->spans.push_back(std::move(s));
  }
};

// hipFuncAttributeMaxDynamicSharedMemorySize, raised only when a launch needs more than the kernel has been granted
int allow_dyn_lds(gpc_hip_ctx* c, const void* fn, size_t bytes) {
  int& have = c->dyn_lds[fn];
  if ((int)bytes <= have) return GPC_OK;
  HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  have = (int)bytes;
  return GPC_OK;
}

int check_dims(int W, int H) {
  if (W <= 0 || H <= 0 || (W % 16) != 0) return GPC_E_INVALID;
  if (W < 2 * GPC_R + 16 || H < 2 * GPC_R + 4) return GPC_E_INVALID;
  // the reference takes any multiple of 16; here a row must fit one workgroup's join table (k_rowjoin.h) and a
  // pixel index 30 bits
  if (W > 16384 || (long)W * H > (1l << 30)) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// CPUs this process may really use: affinity mask and cgroup quota, at most 16
int usable_cpus() {
  int n = 1;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (FILE* fp = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32];
    long per = 0;
    if (fscanf(fp, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
      const long lim = atol(q) / per;
      if (lim >= 1 && lim < n) n = (int)lim;
    }
    fclose(fp);
  }
  if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    long quota = -1, per = 0;
    if (fscanf(fp, "%ld", &quota) == 1 && quota > 0) {
      if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
        if (fscanf(fq, "%ld", &per) == 1 && per > 0 && quota / per >= 1 && quota / per < n) n = (int)(quota / per);
        fclose(fq);
      }
    }
    fclose(fp);
  }
  return n < 1 ? 1 : (n > 16 ? 16 : n);
}

// The CPUs of the GPU's NUMA node: /sys/bus/pci/devices/<bus id>/numa_node, then that node's cpulist, intersected with
// what the process may use.  GPC_HIP_NO_NUMA_BIND leaves the workers unbound.
void find_gpu_node_cpus(gpc_hip_ctx* c) {
  c->have_node_cpus = false;
  if (getenv("GPC_HIP_NO_NUMA_BIND")) return;
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, c->device) != hipSuccess) return;
  for (char* p = bdf; *p; ++p) *p = (char)tolower((unsigned char)*p);
  char path[256];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
  int node = -1;
  if (FILE* fp = fopen(path, "r")) {
    if (fscanf(fp, "%d", &node) != 1) node = -1;
    fclose(fp);
  }
  if (node < 0) return;
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  FILE* fp = fopen(path, "r");
  if (!fp) return;
  char list[4096] = {0};
  const size_t got = fread(list, 1, sizeof list - 1, fp);
  fclose(fp);
  list[got] = 0;
  cpu_set_t node_set, mine;
  CPU_ZERO(&node_set);
  for (const char* p = list; *p;) {  // "0-15,128-143"
    while (*p && !isdigit((unsigned char)*p)) ++p;
    if (!*p) break;
    char* e = nullptr;
    long a = strtol(p, &e, 10), b = a;
    p = e;
    if (*p == '-') b = strtol(p + 1, &e, 10), p = e;
    for (long k = a; k <= b && k < CPU_SETSIZE; ++k) CPU_SET((int)k, &node_set);
  }
  if (sched_getaffinity(0, sizeof mine, &mine) != 0) return;
  CPU_AND(&c->node_cpus, &node_set, &mine);
  if (CPU_COUNT(&c->node_cpus) < 2) return;  // nothing sensible to bind to
  c->numa_node = node;
  c->have_node_cpus = true;
  // the node's CPUs by last-level cache: /sys/devices/system/cpu/cpuN/cache/index3/shared_cpu_list ("64-71,192-199")
  c->node_l3.clear();
  if (getenv("GPC_HIP_NO_CCD_SPREAD")) return;
  cpu_set_t seen;
  CPU_ZERO(&seen);
  for (int cpu = 0; cpu < CPU_SETSIZE; ++cpu) {
    if (!CPU_ISSET(cpu, &c->node_cpus) || CPU_ISSET(cpu, &seen)) continue;
    snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE* f3 = fopen(path, "r");
    if (!f3) { c->node_l3.clear(); return; }
    char l3[1024] = {0};
    const size_t g3 = fread(l3, 1, sizeof l3 - 1, f3);
    fclose(f3);
    l3[g3] = 0;
    cpu_set_t grp;
    CPU_ZERO(&grp);
    for (const char* p = l3; *p;) {
      while (*p && !isdigit((unsigned char)*p)) ++p;
      if (!*p) break;
      char* e = nullptr;
      long a = strtol(p, &e, 10), b = a;
      p = e;
      if (*p == '-') b = strtol(p + 1, &e, 10), p = e;
      for (long k = a; k <= b && k < CPU_SETSIZE; ++k)
        if (CPU_ISSET((int)k, &c->node_cpus)) CPU_SET((int)k, &grp);
    }
    if (CPU_COUNT(&grp) == 0) CPU_SET(cpu, &grp);
    CPU_OR(&seen, &seen, &grp);
    c->node_l3.push_back(grp);
  }
  if (c->node_l3.size() < 2) c->node_l3.clear();  // one cache domain: nothing to spread over
}

// Worker threads gpc_hip_match_batch may start for the host expansion when nobody said how many: the process's CPUs
// shared among the ranks of this node (one process per GPU sets LOCAL_WORLD_SIZE, torch.distributed.run does), less one
// for the thread that feeds the GPU; at least 2, at most 8 (3 .. 10 workers all keep up with the link).
int default_expand_threads() {
  int share = 0;
  int local_world = 1;
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 64) local_world = v;
  }
  cpu_set_t set;
  int visible = 1;
  if (sched_getaffinity(0, sizeof set, &set) == 0) visible = CPU_COUNT(&set);
  // a one-GPU box gives the process a quota of its own (usable_cpus sees it); on a node shared by the ranks of one
  // job every rank sees all CPUs and must share them
  share = local_world > 1 ? visible / local_world - 1 : usable_cpus() - 2;
  return share < 2 ? 2 : (share > 8 ? 8 : share);
}

// Packed supports (xL | xR << 16, rows in ascending order, rows[y] of them in row y) -> ndb::Support records
// {x, y, float(xL - xR)} (inference.hpp:384-391, buffer.hpp:91-97) for the rows [y0, y1) of one pair whose first
// support has index `first`; stops at index `limit`.  Four records are 48 bytes = three 16-byte streaming
// stores (no read-for-ownership of the 625 MB a 256-pair batch expands to).
void expand_rows(const uint32_t* packed, const int32_t* rows, int y0, int y1, long first, long limit, gpc_support* out) {
  long pos = first;
  const uint32_t* src = packed + first;
#if defined(__SSE2__)
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const __m128i m16 = _mm_set1_epi32(0xFFFF);
#endif
  for (int y = y0; y < y1 && pos < limit; ++y) {
    const long cnt = rows[y];
    long n = cnt;
    if (pos + n > limit) n = limit - pos;
    long i = 0;
    auto one = [&](uint32_t v) {
      const int xl = (int)(v & 0xFFFFu), xr = (int)(v >> 16);
      out[pos].x = xl;
      out[pos].y = y;
      out[pos].d = (float)(xl - xr);
      ++pos;
    };
#if defined(__SSE2__)
    if (aligned) {
      for (; i < n && (pos & 3); ++i) one(src[i]);
      const __m128 Y = _mm_castsi128_ps(_mm_set1_epi32(y));
      for (; i + 4 <= n; i += 4, pos += 4) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i));
        const __m128i xl = _mm_and_si128(v, m16);
        const __m128 X = _mm_castsi128_ps(xl);
        const __m128 D = _mm_cvtepi32_ps(_mm_sub_epi32(xl, _mm_srli_epi32(v, 16)));
        const __m128 t0 = _mm_castsi128_ps(_mm_unpacklo_epi32(xl, _mm_castps_si128(Y)));  // x0 y x1 y
        const __m128 t1 = _mm_castsi128_ps(_mm_unpackhi_epi32(xl, _mm_castps_si128(Y)));  // x2 y x3 y
        const __m128 a = _mm_shuffle_ps(t0, _mm_shuffle_ps(D, X, _MM_SHUFFLE(1, 1, 0, 0)), _MM_SHUFFLE(2, 0, 1, 0));  // x0 y d0 x1
        const __m128 b = _mm_shuffle_ps(_mm_shuffle_ps(Y, D, _MM_SHUFFLE(1, 1, 0, 0)), t1, _MM_SHUFFLE(1, 0, 2, 0));  // y d1 x2 y
        const __m128 c = _mm_shuffle_ps(_mm_shuffle_ps(D, X, _MM_SHUFFLE(3, 3, 2, 2)),
                                        _mm_shuffle_ps(Y, D, _MM_SHUFFLE(3, 3, 0, 0)), _MM_SHUFFLE(2, 0, 2, 0));      // d2 x3 y d3
        __m128i* o = reinterpret_cast<__m128i*>(out + pos);
        _mm_stream_si128(o, _mm_castps_si128(a));
        _mm_stream_si128(o + 1, _mm_castps_si128(b));
        _mm_stream_si128(o + 2, _mm_castps_si128(c));
      }
    }
#endif
    for (; i < n; ++i) one(src[i]);
    src += cnt;
  }
#if defined(__SSE2__)
  _mm_sfence();
#endif
}

void ExpandPool::run(int index) {
  {
    std::lock_guard<std::mutex> g(m_);
    cpus_[(size_t)index] = sched_getcpu();
    ++started_;
  }
  done_.notify_all();
  for (;;) {
    ExpandJob j;
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [&] { return quit_ || !q_.empty(); });
      if (q_.empty()) return;
      j = q_.front();
      q_.pop_front();
      cpus_[(size_t)index] = sched_getcpu();
    }
    if (j.copy_bytes) memcpy(j.copy_dst, j.copy_src, j.copy_bytes);
    else expand_rows(j.packed, j.rows, j.y0, j.y1, j.first, j.limit, j.out);
    {
      std::lock_guard<std::mutex> g(m_);
      if (--pending_[j.slot & 7] == 0) done_.notify_all();
    }
  }
}

int pow2_at_least(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}

// ---------------------------------------------------------------- forest parsing

bool next_tok(const char*& p, std::string& tok) {
  while (*p && isspace((unsigned char)*p)) ++p;
  if (!*p) return false;
  const char* s = p;
  while (*p && !isspace((unsigned char)*p)) ++p;
  tok.assign(s, p - s);
  return true;
}

bool next_int(const char*& p, int& v) {
  std::string tok;
  if (!next_tok(p, tok)) return false;
  char* end = nullptr;
  long l = strtol(tok.c_str(), &end, 10);
  if (end == tok.c_str()) return false;
  v = (int)l;
  return true;
}

// ---------------------------------------------------------------- pipeline stages

// The two device-wide matchers run_match hands over to stand below it and use this section's helpers.  They are declared
// here, not moved in front of run_match: the order in which the translation unit first names the kernel templates is the
// order of their instantiations in the device code, and run_match names the row joins first.
// seq: the code images (and candidate bytes) are a frame sequence [npairs + 1][H][W], pair p = frames (p, p + 1); the
// statistics are in the pair layout all the same (k_seq_stats)
int run_global_match(gpc_hip_ctx* c, int W, int H, int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand,
                     void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool seq = false);
int run_hashtable_match(gpc_hip_ctx* c, int W, int H, int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand,
                        void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool seq = false);

// raw0/raw1 device pointers; fills smooth, grad for npairs*sides images
// gradbits: the caller's only reader of the gradient image is run_hash (a batched pipeline): it may leave as one bit per pixel
// d_smooth_out / d_grad_out: where the images go instead of the context's workspaces (byte gradient image only)
int run_preprocess(gpc_hip_ctx* c, const uint8_t* d_raw0, const uint8_t* d_raw1, int W, int H,
                   int npairs, int sides, int thr, bool gradbits = false, uint8_t* d_smooth_out = nullptr,
                   uint8_t* d_grad_out = nullptr, int32_t* d_stats = nullptr) {
  const int nimg = npairs * sides;
  const size_t n = (size_t)W * H;
  if (!d_smooth_out) {
    CHK(ensure(c, c->smooth, n * nimg));
    CHK(ensure(c, c->grad, n * nimg));
    d_smooth_out = (uint8_t*)c->smooth.p;
    d_grad_out = (uint8_t*)c->grad.p;
  } else {
    gradbits = false;
  }
  // d_stats: where the images' statistics words go instead of the head of c->stats (a track stream keeps slot 0 for the
  // carried frame)
  if (!d_stats) {
    CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE * nimg));
    d_stats = (int32_t*)c->stats.p;
  }
  // threshold^2 passes through _mm_set1_epi16 in the SSE build (filter.hpp:418); sobelNaive keeps the int (:159)
  const int thr_sq = c->naive ? (thr & 0xFF) * (thr & 0xFF) : (int)(int16_t)(uint16_t)((thr & 0xFF) * (thr & 0xFF));
  // Rows per thread (the strip a thread marches down): 14 read every raw row 1.14 times and are what a launch that fills the
  // device many times over wants; a smaller launch is a matter of ROUNDS -- the device holds 8 workgroups per CU, and a launch
  // of 1.2 rounds takes two -- so the strip height is the one whose rounds x (rows + 2 read + ~2 of set-up) comes out lowest:
  // 64 images of 1024x436 are 1024 workgroups of 14-row strips (half a round of long chains: 23 us), 2432 of 6-row ones
  // (1.2 rounds: 21 us) and exactly 2048 of 7-row ones (one round).
  const int gx = (W / PP_PX + PP_TX - 1) / PP_TX;
  auto blocks_with = [&](int r) { return (long)gx * ((H + PP_TY * r - 1) / (PP_TY * r)) * nimg; };
  int rows = c->pre_rows;
  if (!rows) {
    static const int heights[] = {PP_ROWS, 10, 7, PP_ROWS_MID, 4, PP_ROWS_SMALL};
    const long places = 8l * (c->num_cus > 0 ? c->num_cus : 256);
    long best = -1;
    for (int r : heights) {
      const long cost = (blocks_with(r) + places - 1) / places * (r + 4);
      if (best < 0 || cost < best) { best = cost; rows = r; }   // (ties go to the taller strip: fewer re-read rows)
    }
  }
  dim3 grid(gx, (H + PP_TY * rows - 1) / (PP_TY * rows), nimg);
  Timed t(c, KID_PREPROCESS);
  // (the SSE=OFF arithmetic keeps the byte image: its 32-test codes need the candidate BYTES in the matchers, wide_codes())
  c->grad_is_bits = gradbits && !c->naive && !c->no_grad_bits;
  snprintf(c->launch_name[KID_PREPROCESS], sizeof c->launch_name[0], "gpc::k_preprocess<%s, %d%s>", c->naive ? "true" : "false", rows,
           c->grad_is_bits ? ", true" : "");
#define LAUNCH_PRE(NAIVE, ROWS, BITS)                                                                        \
  hipLaunchKernelGGL((gpc::k_preprocess<NAIVE, ROWS, BITS>), grid, dim3(PP_TX * PP_TY), 0, c->stream, d_raw0, d_raw1, \
                     d_smooth_out, d_grad_out, W, H, sides, thr_sq, d_stats)
#define LAUNCH_PRE_ROWS(NAIVE, BITS)                                  \
  do {                                                                \
    if (rows == PP_ROWS) LAUNCH_PRE(NAIVE, PP_ROWS, BITS);            \
    else if (rows == 10) LAUNCH_PRE(NAIVE, 10, BITS);                 \
    else if (rows == 7) LAUNCH_PRE(NAIVE, 7, BITS);                   \
    else if (rows == PP_ROWS_MID) LAUNCH_PRE(NAIVE, PP_ROWS_MID, BITS); \
    else if (rows == 4) LAUNCH_PRE(NAIVE, 4, BITS);                   \
    else LAUNCH_PRE(NAIVE, PP_ROWS_SMALL, BITS);                      \
  } while (0)
  if (c->naive) LAUNCH_PRE_ROWS(true, false);
  else if (c->grad_is_bits) LAUNCH_PRE_ROWS(false, true);
  else LAUNCH_PRE_ROWS(false, false);
#undef LAUNCH_PRE_ROWS
#undef LAUNCH_PRE
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// smooth/grad/(candmap) device pointers for nimg images -> code image
// groups > 0: k_hash_groups over the context's groups (gpc_hip_set_forest_groups), image 2p + s writing group g as image
// (p * groups + g) * 2 + s (gstep 2) or, one image, g (gstep 1); the statistics of those virtual images in c->stats
int run_hash(gpc_hip_ctx* c, const uint8_t* d_smooth, const uint8_t* d_grad, const uint8_t* d_cand,
             int W, int H, int nimg, bool dense, uint32_t* d_codes, int groups = 0, int gstep = 2, int32_t* d_stats = nullptr) {
  if (!c->have_forest) return GPC_E_NO_FOREST;
  // tiles per workgroup: each CU holds 2 workgroups (67 KiB of LDS each); walking several
  // vertically adjacent tiles hides the next window's load latency, but the grid must still fill
  // the 512 slots and split the tile rows evenly.  cost ~ rounds * tiles per workgroup.
  // tiles cover the candidate rows 13 .. H-14 only (k_hash.h)
  // the gradient image is k_preprocess's bit image: the batched SSE pipelines (run_preprocess(..., gradbits))
  const bool gbits = c->grad_is_bits && d_grad == (const uint8_t*)c->grad.p && !dense && !c->naive && d_cand == nullptr;
  const int slots = 2 * (c->num_cus > 0 ? c->num_cus : 256);  // workgroups of k_hash the device holds at once (2 per CU: 67-76 KiB of LDS each)
  const int gx = (W + HT_X - 1) / HT_X;
  int ty = HT_Y;
  {
    // Launches too small for several tiles per workgroup run in ROUNDS of `slots` one-tile workgroups: a single 1920x1080
    // pair is 8 x 33 x 2 = 528 tiles of 32 rows -- a second round for 16 of them, 39 us of a 74 us step -- and 432 tiles
    // of 40 rows.  The taller tile (batched SSE pipelines only) is taken where rounds x window rows comes out lower.
    const long n32 = (long)gx * ((H - 2 * GPC_R + HT_Y - 1) / HT_Y) * nimg, n40 = (long)gx * ((H - 2 * GPC_R + HT_Y_TALL - 1) / HT_Y_TALL) * nimg;
    const long c32 = (n32 + slots - 1) / slots * (HT_Y + 2 * GPC_R), c40 = (n40 + slots - 1) / slots * (HT_Y_TALL + 2 * GPC_R);
    if (gbits && n32 < 2l * slots && c40 < c32) ty = HT_Y_TALL;
    if (gbits && c->hash_tall == 1) ty = HT_Y_TALL;
    if (c->hash_tall == 0) ty = HT_Y;
  }
  const int tiles_y = (H - 2 * GPC_R + ty - 1) / ty;
  int tpw = 1;
  if ((long)gx * tiles_y * nimg >= 2l * slots) {  // small launches keep one tile per workgroup (parallelism first)
    // What a split costs is the longest chain of tiles one of the `slots` resident workgroup places works through.  A column
    // of tiles_y tiles becomes ceil(tiles_y / t) workgroups of t tiles and one of the remainder; the hardware starts the
    // next workgroup wherever one ends, so the places fill like bins: as many whole workgroups as fit the rounds, the
    // short ones last.  (Scored as "idle tail of the last round + 4 % for a ragged split" before: at 32 pairs of 1024x436
    // -- 13 tile rows, 256 columns -- that took 4 + 4 + 4 + 1 tiles in two rounds (8 tiles on the longest chain) over
    // 7 + 6 in one (7): k_hash 58 -> 52 us.)  A workgroup's start (tap tables, first window not overlapped) is ~0.4 tile.
    double best = 1e30;
    for (int t = 2; t <= 16 && t <= tiles_y; ++t) {
      const long per_col = (tiles_y + t - 1) / t, ncol = (long)gx * nimg;
      const long nwg = per_col * ncol;
      // (a split that leaves a few places empty still counts: one 3840x2160 pair is 15 x 67 x 2 tiles = 510 workgroups of 4 for
      //  512 places -- 57 us where 1020 workgroups of 2 take 60, and 68 with k_hash's wave priorities)
      if (nwg * 8 < (long)slots * 7) break;
      const int rem = tiles_y - (int)(per_col - 1) * t;             // tiles of a column's last workgroup (1 .. t)
      const long n_full = (per_col - 1) * ncol, n_rem = ncol;         // workgroups of t tiles / of rem tiles
      // full-size workgroups dealt over the places first, the short ones onto the least loaded places
      const long full_rounds = n_full / slots, full_left = n_full % slots;
      double chain = (double)full_rounds * (t + 0.4);
      long short_left = n_rem;
      if (full_left) {  // `full_left` places carry one more full workgroup; the others take short ones meanwhile
        const long free_places = slots - full_left;
        const long fit = free_places * (long)((t + 0.4) / (rem + 0.4));  // short workgroups that fit beside that round
        short_left = n_rem > fit ? n_rem - fit : 0;
        chain += t + 0.4;
      }
      chain += (double)((short_left + slots - 1) / slots) * (rem + 0.4);
      if (chain < best - 1e-9) { best = chain; tpw = t; }
    }
  }
  if (c->hash_tpw > 0) tpw = c->hash_tpw < tiles_y ? c->hash_tpw : tiles_y;  // GPC_HIP_HASH_TPW (tuning)
  dim3 grid(gx, (tiles_y + tpw - 1) / tpw, nimg);
  // the last `slots` workgroups in dispatch order: the launch's last round (k_hash.h: wave priority by the tiles left)
  const long nwg_all = (long)grid.x * grid.y * grid.z;
  const int last_from = nwg_all > slots ? (int)(nwg_all - slots) : 0;
  c->hash_plan[0] = ty, c->hash_plan[1] = tpw, c->hash_plan[2] = (int32_t)grid.y, c->hash_plan[3] = last_from;
  Timed t(c, KID_HASH);
  const bool tau = groups > 0 ? c->gtau : c->forest.type != 0;
  int32_t* st = d_stats ? d_stats : (int32_t*)c->stats.p;  // (d_stats: as for run_preprocess)
  if (groups > 0) {
    const GpcForestDev* gf = (const GpcForestDev*)c->gforest_dev.p;
    snprintf(c->launch_name[KID_HASH], sizeof c->launch_name[0], "gpc::k_hash_groups<%s, %s, %s, %s, %d>", tau ? "true" : "false",
             dense ? "true" : "false", c->naive ? "true" : "false", gbits ? "true" : "false", ty);
#define LAUNCH_HASH_G(TAU, DENSE, NAIVE, GB, TY, FD)                                                                       \
  hipLaunchKernelGGL((gpc::k_hash_groups<TAU, DENSE, NAIVE, GB, TY>), grid, dim3(HT_THREADS), 0, c->stream, d_smooth, d_grad, \
                     d_cand, d_codes, W, H, gf + (FD) * GPC_MAX_GROUPS, st, tpw, last_from, groups, gstep)
    if (gbits) {
      if (ty == HT_Y_TALL) {
        if (tau) LAUNCH_HASH_G(true, false, false, true, HT_Y_TALL, 2); else LAUNCH_HASH_G(false, false, false, true, HT_Y_TALL, 2);
      } else {
        if (tau) LAUNCH_HASH_G(true, false, false, true, HT_Y, 0); else LAUNCH_HASH_G(false, false, false, true, HT_Y, 0);
      }
    } else if (c->naive) {
      if (tau && dense) LAUNCH_HASH_G(true, true, true, false, HT_Y, 1);
      else if (tau) LAUNCH_HASH_G(true, false, true, false, HT_Y, 1);
      else if (dense) LAUNCH_HASH_G(false, true, true, false, HT_Y, 1);
      else LAUNCH_HASH_G(false, false, true, false, HT_Y, 1);
    } else {
      if (tau && dense) LAUNCH_HASH_G(true, true, false, false, HT_Y, 0);
      else if (tau) LAUNCH_HASH_G(true, false, false, false, HT_Y, 0);
      else if (dense) LAUNCH_HASH_G(false, true, false, false, HT_Y, 0);
      else LAUNCH_HASH_G(false, false, false, false, HT_Y, 0);
    }
#undef LAUNCH_HASH_G
    HIPCHK(c, hipGetLastError());
    return GPC_OK;
  }
  snprintf(c->launch_name[KID_HASH], sizeof c->launch_name[0], "gpc::k_hash<%s, %s, %s, %s, %d>", tau ? "true" : "false",
           dense ? "true" : "false", c->naive ? "true" : "false", gbits ? "true" : "false", ty);
#define LAUNCH_HASH(TAU, DENSE, NAIVE)                                                                    \
  hipLaunchKernelGGL((gpc::k_hash<TAU, DENSE, NAIVE>), grid, dim3(HT_THREADS), 0, c->stream, d_smooth, d_grad, \
                     d_cand, d_codes, W, H, (const GpcForestDev*)c->forest_dev.p + (NAIVE ? 1 : 0), st, tpw, last_from)
  if (gbits) {
#define LAUNCH_HASH_BITS(TAU, TY, FD)                                                                                      \
  hipLaunchKernelGGL((gpc::k_hash<TAU, false, false, true, TY>), grid, dim3(HT_THREADS), 0, c->stream, d_smooth, d_grad, \
                     d_cand, d_codes, W, H, (const GpcForestDev*)c->forest_dev.p + FD, st, tpw, last_from)
    if (ty == HT_Y_TALL) {
      if (tau) LAUNCH_HASH_BITS(true, HT_Y_TALL, 2); else LAUNCH_HASH_BITS(false, HT_Y_TALL, 2);
    } else {
      if (tau) LAUNCH_HASH_BITS(true, HT_Y, 0); else LAUNCH_HASH_BITS(false, HT_Y, 0);
    }
#undef LAUNCH_HASH_BITS
  } else if (c->naive) {
    if (tau && dense) LAUNCH_HASH(true, true, true);
    else if (tau) LAUNCH_HASH(true, false, true);
    else if (dense) LAUNCH_HASH(false, true, true);
    else LAUNCH_HASH(false, false, true);
  } else {
    if (tau && dense) LAUNCH_HASH(true, true, false);
    else if (tau) LAUNCH_HASH(true, false, false);
    else if (dense) LAUNCH_HASH(false, true, false);
    else LAUNCH_HASH(false, false, false);
  }
#undef LAUNCH_HASH
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// Significant bits of the codes the current forest can produce (the partitioned matcher bins on the top ones of
// these, k_partition.h).  SSE placement (filter.hpp:574-595): test t -> bit t for
// t <= 7, test 8 is OR-ed into bit 0, test t -> bit t-1 for t >= 9; Naive (filter.hpp:245-249): T bits.
// (group mode: the largest group's -- one planner width for every group; a smaller group's codes then fill the low bins)
int code_bits(const gpc_hip_ctx* c) {
  const int T = c->ngroups > 1 ? c->gmax_tests : c->forest.num_tests;
  if (c->naive) return T;
  return T <= 8 ? T : T - 1;
}

// SSE=OFF arithmetic with 32 tests: codes use bit 31 and 0xFFFFFFFF is a code (k_rowjoin.h, WIDE)
bool wide_codes(const gpc_hip_ctx* c) { return c->naive && (c->ngroups > 1 ? c->gmax_tests : c->forest.num_tests) == 32; }

// How the join kernel covers a row of W pixels: NT threads x SPT pixel slots, table of 1 << log2s slots.
struct JoinPlan {
  int nt, spt, log2s;
  size_t lds;
};

JoinPlan plan_join(const gpc_hip_ctx* c, int W) {
  JoinPlan p;
  p.spt = 1;
  p.nt = 256;
  while (p.spt * p.nt < W && p.spt < 4) p.spt <<= 1;    // <= 1024 px: 256 threads, 8 workgroups per CU
  while (p.spt * p.nt < W && p.nt < 1024) p.nt <<= 1;   // <= 4096 px: more threads per row
  if (c->join_nt && 4 * c->join_nt >= W) {  // tuning override (GPC_HIP_JOIN_NT): threads per row, slots per thread follow
    p.nt = c->join_nt;
    p.spt = 1;
    while (p.spt * p.nt < W) p.spt <<= 1;
  }
  while (p.spt * p.nt < W && p.spt < 16) p.spt <<= 1;   // <= 16384 px: 1024 threads with 8 / 16 slots each
  // only left codes are inserted: S >= 2*(W-26) keeps the load factor <= 0.5 (up to the 16384 slots = 128 KiB
  // one workgroup can have: beyond 8218 px the table fills further, W-26 < 16384 keys always fit);
  // S >= NT*SPT because the rank phase reuses the key table as bucket counters
  p.log2s = 1;
  while ((1 << p.log2s) < p.nt * p.spt || ((1 << p.log2s) < 2 * (W - 2 * GPC_R) && p.log2s < 14)) ++p.log2s;
  p.lds = ((size_t)8 * ((1u << p.log2s) + 1) + 15) / 16 * 16;  // keys + flag/x words
  return p;
}

// A look-back of the fused join gave up (k_rowjoin_fused.h, RJ_SPIN_LIMIT): the results of that launch are not to be
// used.  The kernel stores the launch's epoch (never 0) into a page-locked word with a plain system-scope store; the word
// is looked at wherever an entry point has just synchronised the stream, at the top of the NEXT fused launch (callers that
// wait on their own stream -- set_stream + their own synchronisation -- learn of it there at the latest) and in
// gpc_hip_destroy, and says WHICH launch failed.
int check_join_err(gpc_hip_ctx* c) {
#ifdef RJ_DBG_COUNT
  if (c->h_err.p && c->h_err.p[1]) {
    fprintf(stderr, "[RJ_DBG_COUNT] look-backs %d, windows with a row that had not published %d, displaced keys that met their copy %d\n", c->h_err.p[1], c->h_err.p[2], c->h_err.p[3]);
    c->h_err.p[1] = c->h_err.p[2] = c->h_err.p[3] = 0;
  }
#endif
  if (c->h_err.p) {
    // (one exchange: a launch still in flight may store its epoch between a load and a clearing store, and would be lost)
    const int32_t ep = __atomic_exchange_n(c->h_err.p, 0, __ATOMIC_ACQ_REL);
    if (ep) {
      snprintf(c->err, sizeof(c->err), "k_row_join_fused: a row waited too long for the rows before it in fused launch %d of this "
               "context (%u launched so far): THAT launch's supports are not to be used; a call that reports this at its start "
               "has queued nothing itself", ep, c->join_epoch);
      return GPC_E_HIP;
    }
  }
  return GPC_OK;
}

// Ticket counters (shards of pairs) of a fused launch.  Workgroup b serves shard b % shards and lands on XCD b % 8, so
//   * 8 | shards pins every shard -- its pairs -- to one XCD, and the XCDs finish apart: 256 pairs with 8 / 16 / 32 / 64
//     shards 567-570 us, with 3 .. 13 shards 550-554 us (15 / 17 / 21 / 31: 561 / 562 / 565 / 573; 2 shards 653 and one
//     shard 1246: same-address atomics on the counter);
//   * a shard's workgroups take only its rows, so shards of unequal size finish apart as well: 8 pairs of 1920x1080 over
//     7 shards (one of them two pairs) 155 us against 123 over 8.
// So: 3 .. 13 shards, not a multiple of 8, the least time the fullest shard runs alone; ties go to the count nearest 7.
int join_shards(const gpc_hip_ctx* c, int npairs) {
  if (c->fuse_shards > 0) return npairs < c->fuse_shards ? npairs : c->fuse_shards;
  return join_shards_auto(npairs);  // (gpc_device.h: reachable by a host-only compile)
}

// State of the fused join: ticket counters + one granule per (pair, row); zeroed when (re)allocated, then kept
// consistent by the kernel itself (the last draw resets a counter; granules carry the launch's epoch).
int ensure_join_state(gpc_hip_ctx* c, size_t granules) {
  const size_t tk_bytes = sizeof(uint32_t) * RJ_SHARDS * RJ_TICKET_STRIDE;
  if (!c->h_err.p) {
    HIPCHK(c, c->h_err.alloc(64, hipHostMallocMapped));
    memset(c->h_err.p, 0, 64);
    HIPCHK(c, hipHostGetDevicePointer((void**)&c->d_err, c->h_err.p, 0));
  }
  if (granules > c->jstate_granules || c->join_epoch >= (1u << 30) - 2u) {
    CHK(ensure(c, c->jstate, tk_bytes + sizeof(unsigned long long) * granules));
    HIPCHK(c, hipMemsetAsync(c->jstate.p, 0, c->jstate.cap, c->stream));
    c->jstate_granules = (c->jstate.cap - tk_bytes) / sizeof(unsigned long long);
    c->join_epoch = 0;
  }
  return GPC_OK;
}

int ensure_flag_event(gpc_hip_ctx* c) {
  if (!c->e_flag) HIPCHK(c, c->e_flag.create(hipEventDisableTiming));
  return GPC_OK;
}

// The second stream of the device-wide matchers: a launch for the few over-large partitions / bins runs beside the main one.
int ensure_aux_stream(gpc_hip_ctx* c) {
  if (c->s_aux) return GPC_OK;
  HIPCHK(c, c->s_aux.create(hipStreamNonBlocking));
  HIPCHK(c, c->e_fork.create(hipEventDisableTiming));
  HIPCHK(c, c->e_join.create(hipEventDisableTiming));
  return GPC_OK;
}

// code images of npairs pairs -> supports / correspondences in d_out.
// d_cand: the candidate bytes the hash kernel used ([2*npairs][H][W]: grad, or the scattered mask list)
// mode 0: gpc_support, 1: gpc_correspondence, 2: packed supports (epipolar sort-match only; `po` says where)
// seq: a frame sequence (codes / d_cand [npairs + 1][H][W], pair p = frames p and p + 1; statistics in the pair layout):
// the epipolar matcher takes k_row_join_seq + k_gather_rows, the device-wide matchers read the images at a stride of one
int run_match(gpc_hip_ctx* c, int W, int H, int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand,
              void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, const PackedOut* po = nullptr, bool seq = false) {
  const int apply_filter = (mode != 1);
  if (mode == 2 && (s->use_hashtable || !s->epipolar_mode || !po)) return GPC_E_UNSUPPORTED;
  if (seq && (mode == 2 || po)) return GPC_E_UNSUPPORTED;
  if (s->use_hashtable) return run_hashtable_match(c, W, H, npairs, s, mode, d_cand, d_out, cap, d_counts, d_ncand, seq);
  if (s->epipolar_mode) {
    CHK(ensure(c, c->staged, sizeof(uint32_t) * (size_t)W * H * npairs));
    CHK(ensure(c, c->rowcnt, sizeof(int32_t) * (size_t)H * npairs * 2));
    // |dy| is 0 for every epipolar match; a negative tolerance rejects everything
    int disp_high = s->disp_high;
    if (apply_filter && s->vertical_tolerance < 0) disp_high = -1;
    const JoinPlan jp = plan_join(c, W);
    if (jp.nt * jp.spt < W) return GPC_E_UNSUPPORTED;  // unreachable below check_dims' 16384 px
    // One launch for join + output (k_rowjoin_fused.h) for rows up to 4096 px (12 bits of x beside the flags) when the
    // records' place follows from the rows before them alone (not the gap-free packing of `totals`)
    const size_t flds = RJF_LDS_BYTES(jp.nt * jp.spt);
    bool fuse = !seq && !c->no_fuse && npairs >= c->fuse_min_pairs && jp.spt <= 4 && jp.nt * jp.spt <= 4096 &&
                !(po && po->totals) && (long)npairs * (H - 2 * GPC_R) < (1l << 31) - 65536;
    if (fuse && !c->fuse_always) {
      // The persistent launch pays off once every workgroup takes several rows (its output lags one row behind, and the
      // last row of a workgroup is placed with a blocking look-back): measured against join + k_gather_rows (round 5, with
      // the wave priorities of k_rowjoin_fused.h), 1024x436 steps: 4 .. 16 pairs 4-14 % slower, 20 / 24 pairs 3 % faster,
      // 28 pairs 8 %, 32 .. 256 pairs 8-11 %; 1920x1080: one pair 6 % slower, 8 pairs 8 % faster; one 3840x2160 pair 9 %
      // faster.  Rows per resident workgroup >= 4, or >= 3 for rows of 2048 px and more, is where it wins.
      const long lds_wgs = (long)(160 * 1024 / (flds + 64)), wave_wgs = 32 / (jp.nt / 64);
      const long resident = (long)c->num_cus * (lds_wgs < wave_wgs ? lds_wgs : wave_wgs);
      const long rows_total = (long)npairs * (H - 2 * GPC_R);
      fuse = rows_total >= 4 * resident || (W >= 2048 && rows_total >= 3 * resident);
    }
    if (fuse) {
      // k_row_join_fused (k_rowjoin_fused.h): one by-value parameter the kernel reads from its argument segment
      const int nrows = H - 2 * GPC_R;
      CHK(check_join_err(c));  // a look-back of an EARLIER launch that timed out is reported before anything new is queued
      CHK(ensure_join_state(c, (size_t)npairs * nrows));
      const size_t lds = flds;
      gpc::RjfArgs a;
      memset(&a, 0, sizeof a);
      a.codes = (const uint32_t*)c->codes.p;
      a.cand = d_cand;
      a.img_stats = (const int32_t*)c->stats.p;
      a.tickets = (uint32_t*)c->jstate.p;
      a.status = (unsigned long long*)((uint32_t*)c->jstate.p + RJ_SHARDS * RJ_TICKET_STRIDE);
      a.err = c->d_err;
      a.out = d_out;
      a.counts = d_counts;
      a.ncand = d_ncand;
      a.rows_out = po ? po->rows : nullptr;
      a.packed_stride = po ? po->packed_stride : 0l;
      a.rows_stride = po ? po->rows_stride : 0l;
      a.W = W;
      a.H = H;
      a.disp_high = disp_high;
      a.apply_filter = apply_filter;
      a.epoch = ++c->join_epoch;
      a.npairs = npairs;
      a.mode = mode;
      a.cap = cap;
      Timed t(c, KID_ROW_JOIN);
      const bool wide = wide_codes(c);
      snprintf(c->launch_name[KID_ROW_JOIN], sizeof c->launch_name[0], "gpc::k_row_join_fused<%d, %d, %s>", jp.spt, jp.nt,
               wide ? "true" : "false");
      c->launch_name[KID_GATHER_ROWS][0] = 0;
#define LAUNCH_RJF(SPT, NT, WIDE)                                                                               \
  do {                                                                                                          \
    const void* fn_ = reinterpret_cast<const void*>(gpc::k_row_join_fused<SPT, NT, WIDE>);                      \
    int& per_cu = c->wgs_per_cu[std::make_pair(fn_, lds)];                                                      \
    if (per_cu == 0) {                                                                                          \
      if (lds > 48 * 1024) CHK(allow_dyn_lds(c, fn_, lds));                                                     \
      HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn_, NT, lds));                           \
      if (per_cu < 1) per_cu = 1;                                                                               \
    }                                                                                                           \
    /* (two lanes: one workgroup per CU less, the other lane's k_preprocess / k_hash need a wave slot per SIMD) */ \
    long nwg = c->fuse_wgs > 0 ? c->fuse_wgs : (long)((c->pipeline > 1 && per_cu > 1) ? per_cu - 1 : per_cu) * c->num_cus; \
    if (nwg > (long)npairs * nrows) nwg = (long)npairs * nrows;                                                 \
    /* every shard needs a workgroup that draws its tickets (workgroup b serves shard b % nshards) */           \
    int nsh = join_shards(c, npairs);                                                                           \
    if (nsh > nwg) nsh = (int)nwg;                                                                              \
    a.nshards = nsh;                                                                                            \
    if (c->debug) fprintf(stderr, "[gpc_hip] k_row_join_fused<%d, %d>: %d workgroups per CU by the occupancy API, %ld workgroups, %d shards, %zu B of LDS\n", SPT, NT, per_cu, nwg, nsh, lds); \
    const GpcJoinSplit sp_ = make_join_split(npairs, nsh);                                                      \
    a.n_hi = sp_.n_hi;                                                                                          \
    for (int k_ = 0; k_ < 2; ++k_) {                                                                            \
      a.ps[k_] = sp_.ps[k_];                                                                                    \
      a.ps_magic[k_] = sp_.ps_magic[k_];                                                                        \
      a.ps_sh[k_] = sp_.ps_sh[k_];                                                                              \
    }                                                                                                           \
    hipLaunchKernelGGL((gpc::k_row_join_fused<SPT, NT, WIDE>), dim3((unsigned)nwg), dim3(NT), lds, c->stream, a); \
  } while (0)
#define LAUNCH_RJF_W(SPT, NT) do { if (wide) LAUNCH_RJF(SPT, NT, true); else LAUNCH_RJF(SPT, NT, false); } while (0)
#define LAUNCH_RJF_S(NT)                      \
  switch (jp.spt) {                           \
    case 1: LAUNCH_RJF_W(1, NT); break;       \
    case 2: LAUNCH_RJF_W(2, NT); break;       \
    default: LAUNCH_RJF_W(4, NT); break;      \
  }
      if (jp.nt == 1024) { LAUNCH_RJF_S(1024) }
      else if (jp.nt == 512) { LAUNCH_RJF_S(512) }
      else { LAUNCH_RJF_S(256) }
#undef LAUNCH_RJF_S
#undef LAUNCH_RJF_W
#undef LAUNCH_RJF
      HIPCHK(c, hipGetLastError());
      return GPC_OK;
    }
    {
      Timed t(c, KID_ROW_JOIN);
      const int rpw = 1;  // (the kernel takes one row per workgroup)
      const dim3 jgrid((H - 2 * GPC_R + rpw - 1) / rpw, npairs);
      const bool wide = wide_codes(c);
      snprintf(c->launch_name[KID_ROW_JOIN], sizeof c->launch_name[0], "gpc::k_row_join%s<%d, %d, %s>", seq ? "_seq" : "",
               jp.spt, jp.nt, wide ? "true" : "false");
#define LAUNCH_JOIN_K(K, SPT, NT, WIDE)                                                                       \
  do {                                                                                                        \
    const void* fn_ = reinterpret_cast<const void*>(gpc::K<SPT, NT, WIDE>);                                   \
    if (jp.lds > 48 * 1024) CHK(allow_dyn_lds(c, fn_, jp.lds));                                               \
    hipLaunchKernelGGL((gpc::K<SPT, NT, WIDE>), jgrid, dim3(NT), jp.lds, c->stream,                           \
                       (const uint32_t*)c->codes.p, d_cand, W, H, disp_high, apply_filter,                    \
                       (const int32_t*)c->stats.p, (uint32_t*)c->staged.p, (int32_t*)c->rowcnt.p, jp.log2s,   \
                       rpw, gpc::RjVirt());                                                    \
  } while (0)
#define LAUNCH_JOIN(SPT, NT, WIDE) \
  do { if (seq) LAUNCH_JOIN_K(k_row_join_seq, SPT, NT, WIDE); else LAUNCH_JOIN_K(k_row_join, SPT, NT, WIDE); } while (0)
#define LAUNCH_JOIN_W(SPT, NT) do { if (wide) LAUNCH_JOIN(SPT, NT, true); else LAUNCH_JOIN(SPT, NT, false); } while (0)
#define LAUNCH_JOIN_S(NT)                      \
  switch (jp.spt) {                            \
    case 1: LAUNCH_JOIN_W(1, NT); break;       \
    case 2: LAUNCH_JOIN_W(2, NT); break;       \
    default: LAUNCH_JOIN_W(4, NT); break;      \
  }
      if (jp.nt == 1024) {
        if (jp.spt == 16) LAUNCH_JOIN_W(16, 1024);
        else if (jp.spt == 8) LAUNCH_JOIN_W(8, 1024);
        else LAUNCH_JOIN_S(1024)
      } else if (jp.nt == 512) { LAUNCH_JOIN_S(512) }
      else { LAUNCH_JOIN_S(256) }
#undef LAUNCH_JOIN_S
#undef LAUNCH_JOIN_W
#undef LAUNCH_JOIN
#undef LAUNCH_JOIN_K
      HIPCHK(c, hipGetLastError());
    }
    {
      Timed t(c, KID_GATHER_ROWS);
      snprintf(c->launch_name[KID_GATHER_ROWS], sizeof c->launch_name[0], "gpc::k_gather_rows");
      if (po && po->totals)
        hipLaunchKernelGGL(gpc::k_pair_totals, dim3(npairs), dim3(RM_THREADS), 0, c->stream, (const int32_t*)c->rowcnt.p, H,
                           po->totals);
      const int gr = ((long)((H - 2 * GPC_R + GR_ROWS - 1) / GR_ROWS) * npairs >= 2048) ? GR_ROWS : 1;
      hipLaunchKernelGGL(gpc::k_gather_rows, dim3((H - 2 * GPC_R + gr - 1) / gr, npairs), dim3(RM_THREADS), 0, c->stream,
                         (const uint32_t*)c->staged.p, (const int32_t*)c->rowcnt.p, W, H, mode, d_out,
                         cap, d_counts, (const int32_t*)c->stats.p, d_ncand, gr, po ? po->rows : nullptr,
                         po ? po->packed_stride : 0l, po ? po->rows_stride : 0l,
                         po ? (const int32_t*)po->totals : (const int32_t*)nullptr);
      HIPCHK(c, hipGetLastError());
    }
    return GPC_OK;
  }
  return run_global_match(c, W, H, npairs, s, mode, d_cand, d_out, cap, d_counts, d_ncand, seq);
}

// Shared set-up of the two device-wide-sort matchers (k_global.h, k_hashtable.h); every launch
// covers the whole batch (pair = blockIdx.y / .z).
struct GlobalPlan {
  int nmax, nblk, nmblk;
  gpc::GpcBatchStrides bs;
  int32_t *hist, *blkcnt, *gmisc, *rowcnt;
  size_t esz;
};

int plan_global(gpc_hip_ctx* c, int W, int H, int npairs, int mode, int cap, bool hashtable, GlobalPlan& g, bool seq) {
  const size_t n = (size_t)W * H;
  g.nmax = 2 * (W - 2 * GPC_R) * (H - 2 * GPC_R);
  g.nblk = (g.nmax + GS_TILE - 1) / GS_TILE;
  g.nmblk = (g.nmax + RM_THREADS - 1) / RM_THREADS;
  g.esz = mode == 0 ? sizeof(gpc_support) : sizeof(gpc_correspondence);
  const size_t recs = (size_t)g.nmax * npairs;
  for (int i = 0; i < 2; ++i) {
    CHK(ensure(c, c->gkeys[i], sizeof(uint32_t) * recs));
    CHK(ensure(c, c->gvals[i], sizeof(uint32_t) * recs));
    if (hashtable) {
      CHK(ensure(c, c->hkeys[i], sizeof(uint32_t) * recs));
      CHK(ensure(c, c->hvals[i], sizeof(uint32_t) * recs));
    }
  }
  if (hashtable) CHK(ensure(c, c->hrec, 2 * sizeof(uint32_t) * recs));
  CHK(ensure(c, c->ghist, sizeof(int32_t) * ((size_t)256 * g.nblk + g.nmblk) * npairs));
  CHK(ensure(c, c->gmisc, sizeof(int32_t) * GM_STRIDE * npairs));
  CHK(ensure(c, c->rowcnt, sizeof(int32_t) * (size_t)H * 2 * npairs));
  g.hist = (int32_t*)c->ghist.p;
  g.blkcnt = g.hist + (size_t)256 * g.nblk * npairs;
  g.gmisc = (int32_t*)c->gmisc.p;
  g.rowcnt = (int32_t*)c->rowcnt.p;
  g.bs.codes = (long)((seq ? 1 : 2) * n);  // (a sequence: pair p's images are frames p and p + 1)
  g.bs.recs = g.nmax;
  g.bs.hist = (long)256 * g.nblk;
  g.bs.blk = g.nmblk;
  g.bs.out = (long)cap * (long)g.esz;
  g.bs.rows = 2 * H;
  return GPC_OK;
}

// stable LSD radix sort of (keys, vals) by `passes` 8-bit digits; result in buffer index passes & 1
int radix_passes(gpc_hip_ctx* c, const GlobalPlan& g, int npairs, uint32_t* keys[2], uint32_t* vals[2], int passes) {
  for (int pass = 0; pass < passes; ++pass) {
    const int src = pass & 1, dst = src ^ 1;
    hipLaunchKernelGGL(gpc::k_g_hist, dim3(g.nblk, npairs), dim3(GS_THREADS), 0, c->stream,
                       (const uint32_t*)keys[src], (const int32_t*)g.gmisc, 8 * pass, g.hist, g.nblk, g.bs);
    hipLaunchKernelGGL(gpc::k_g_scan, dim3(1, npairs), dim3(1024), 0, c->stream, g.hist, 256 * g.nblk, g.bs.hist);
    hipLaunchKernelGGL(gpc::k_g_scatter, dim3(g.nblk, npairs), dim3(GS_THREADS), 0, c->stream,
                       (const uint32_t*)keys[src], (const uint32_t*)vals[src], keys[dst], vals[dst],
                       (const int32_t*)g.gmisc, 8 * pass, (const int32_t*)g.hist, g.nblk, g.bs);
  }
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// Both radix fallbacks open alike: records per row (k_g_rowcount), then every record's (code, pixel index) into keys / vals.
void launch_radix_records(gpc_hip_ctx* c, const GlobalPlan& g, int W, int H, int npairs, const uint8_t* d_cand, uint32_t* keys,
                          uint32_t* vals) {
  const uint32_t* codes = (const uint32_t*)c->codes.p;
  const uint8_t* wcand = wide_codes(c) ? d_cand : nullptr;  // 32-bit codes: 0xFFFFFFFF is told from the sentinel by the candidate byte
  const int32_t* stats = (const int32_t*)c->stats.p;
  const dim3 rgrid(H - 2 * GPC_R, 2, npairs);
  hipLaunchKernelGGL(gpc::k_g_rowcount, rgrid, dim3(RM_THREADS), 0, c->stream, codes, wcand, W, H, g.rowcnt, stats, g.gmisc, g.bs);
  hipLaunchKernelGGL(gpc::k_g_build, rgrid, dim3(RM_THREADS), 0, c->stream, codes, wcand, W, H, (const int32_t*)g.rowcnt, stats,
                     keys, vals, g.gmisc, g.bs);
}

// launch_name[KID_GLOBAL_MATCH] names the join launches of a device-wide match in launch order (include/gpc_hip.h):
// " + " between two launches, "[list]" behind one whose grid was the planner's work list.
void name_join_launch(gpc_hip_ctx* c, const char* kernel, bool list) {
  char* n = c->launch_name[KID_GLOBAL_MATCH];
  const size_t at = strlen(n);
  snprintf(n + at, sizeof c->launch_name[0] - at, "%s%s%s", at ? " + " : "", kernel, list ? "[list]" : "");
}

// ---------------------------------------------------------------- the two partitioned matchers' shared host side
// Both partition the records into bins (k_gp_hist -> k_g_scan -> planner -> k_gp_scatter, k_partition.h) and join every
// bin or run of bins in one workgroup.  The planner leaves four words for the host behind its plan: maxima over the
// batch, copied to the page-locked c->h_flag.  What they mean is the planner's:
struct CodeRangePlan {   // k_gp_plan (k_partition.h)
  int32_t overflow;      // [0] a single bin beyond GpLayout::cap_hard records on a side: the caller sorts instead
  int32_t max_parts;     // [1] largest number of partitions of a pair: the join's grid
  int32_t max_bin_side;  // [2] largest bin, records of one side: beyond GP_NB some partitions need the 8192-record join
  int32_t max_list;      // [3] longest list of over-large partitions of a pair: up to GP_BIGCAP it is that join's grid
};
struct BucketCheck {  // k_ht_check (k_htjoin.h)
  int32_t overflow;   // [0] a bin beyond 4096 records (left + right)
  int32_t max_bin;    // [1] largest bin, left + right records: the next attempt is sized by it
  int32_t max_pair;   // [2] largest pair, left + right records: records per bucket
  int32_t max_list;   // [3] longest list of bins beyond 2048 records of a pair: up to HTJ_BIGCAP the 1024-thread launch's grid
};
template <class Words>
Words plan_words(const gpc_hip_ctx* c) {
  static_assert(sizeof(Words) == 4 * sizeof(int32_t), "a planner leaves four words");
  Words w;
  memcpy(&w, c->h_flag.p, sizeof w);
  return w;
}

// What both lay out alike: chunks of rows (L), the records, the staged matches, the landing place of the plan's words.
struct PartIo {
  const uint32_t* codes;
  const uint8_t* wcand;
  uint2* kv;
};
int partition_io(gpc_hip_ctx* c, const GlobalPlan& g, int H, int npairs, const uint8_t* d_cand, gpc::GpLayout& L, PartIo& io) {
  const int rows = H - 2 * GPC_R;
  L.rows_per_chunk = rows >= 64 ? c->rows_per_chunk : (rows + 3) / 4;  // >= 4 chunks per image
  L.nchunk = (rows + L.rows_per_chunk - 1) / L.rows_per_chunk;
  CHK(ensure(c, c->staged, sizeof(uint2) * (size_t)(g.nmax / 2) * npairs));  // (left, right) position per match
  CHK(ensure(c, c->gkv, sizeof(uint2) * (size_t)g.bs.recs * npairs));
  if (!c->h_flag.p) CHK(ensure_pinned(c, c->h_flag, 64));
  CHK(ensure_flag_event(c));
  io.codes = (const uint32_t*)c->codes.p;
  io.wcand = wide_codes(c) ? d_cand : nullptr;
  io.kv = (uint2*)c->gkv.p;
  return GPC_OK;
}

// k_gp_hist / k_gp_scatter come for 256, 1024 and 2048 bins
template <bool HT>
struct BinKernels {
  decltype(&gpc::k_gp_hist<HT, 256>) hist;
  decltype(&gpc::k_gp_scatter<HT, 256>) scatter;
};
template <bool HT>
BinKernels<HT> bin_kernels(int nbins) {
  const decltype(BinKernels<HT>::hist) hist[3] = {gpc::k_gp_hist<HT, 2048>, gpc::k_gp_hist<HT, 1024>, gpc::k_gp_hist<HT, 256>};
  const decltype(BinKernels<HT>::scatter) scatter[3] = {gpc::k_gp_scatter<HT, 2048>, gpc::k_gp_scatter<HT, 1024>,
                                                       gpc::k_gp_scatter<HT, 256>};
  const int k = nbins > 1024 ? 0 : nbins > 256 ? 1 : 2;
  return {hist[k], scatter[k]};
}

// One planning round: clear the plan's words (`clear`), histogram, scan, the caller's planner; the four words at d_flag
// start for the host; scatter; wait for the words.  The scatter goes out BEFORE the host looks at them (an event marks
// them): it does not depend on them -- only whether its result is used does -- and the device then works through the
// host's round trip instead of idling (~15 us per call; a batch that has to be planned again, or sorted instead, has
// scattered once for nothing).  The wait synchronises the stream once per round.
template <bool HT, class Planner>
int partition_round(gpc_hip_ctx* c, const GlobalPlan& g, int W, int H, int npairs, const PartIo& io, const gpc::GpLayout& L,
                    int32_t* tabs, int32_t* d_flag, void* clear, size_t clear_bytes, Planner launch_planner) {
  const BinKernels<HT> k = bin_kernels<HT>(L.nbins);
  const dim3 cgrid(L.nchunk, 2, npairs);
  {
    Timed t(c, KID_GLOBAL_KEYS);
    HIPCHK(c, hipMemsetAsync(clear, 0, clear_bytes, c->stream));
    hipLaunchKernelGGL(k.hist, cgrid, dim3(GPS_THREADS), 0, c->stream, io.codes, io.wcand, W, H, g.bs.codes, tabs, L, make_divw(W));
    hipLaunchKernelGGL(gpc::k_g_scan, dim3(1, 2 * npairs), dim3(1024), 0, c->stream, tabs, L.nbins * L.nchunk,
                       (long)L.nbins * L.nchunk);
    CHK(launch_planner());
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(c->h_flag.p, d_flag, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->e_flag, c->stream));
  {
    Timed t(c, KID_GLOBAL_SORT);
    hipLaunchKernelGGL(k.scatter, cgrid, dim3(GPS_THREADS), 0, c->stream, io.codes, io.wcand, W, H, g.bs.codes,
                       (const int32_t*)tabs, L, make_divw(W), io.kv, g.bs.recs);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventSynchronize(c->e_flag));
  return GPC_OK;
}

// A launch for the few over-large partitions / bins on the second stream, beside the main stream's launch instead of
// after it: the constructor forks (s_aux waits for what the main stream holds), side_done() goes behind the side launch,
// join() behind the main one.  Not `on`: all three do nothing.
struct SideLaunch {
  gpc_hip_ctx* c;
  bool on;
  int status;  // of the fork: CHK it before the side launch
  SideLaunch(gpc_hip_ctx* ctx, bool on_) : c(ctx), on(on_), status(on_ ? fork() : GPC_OK) {}
  int fork() {
    CHK(ensure_aux_stream(c));
    HIPCHK(c, hipEventRecord(c->e_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_aux, c->e_fork, 0));
    return GPC_OK;
  }
  int side_done() {
    if (on) HIPCHK(c, hipEventRecord(c->e_join, c->s_aux));
    return GPC_OK;
  }
  int join() {
    if (on) HIPCHK(c, hipStreamWaitEvent(c->stream, c->e_join, 0));
    return GPC_OK;
  }
};

// the longest work list of the batch as a launch's x dimension
inline dim3 list_grid(int max_list, int npairs) { return dim3(max_list > 0 ? max_list : 1, npairs); }

// k_row_join<SPT, 1024, WIDE, true>, one workgroup per partition.  SPT = 4: 8192 table slots for up to 4096 left records
// (64 KiB, two workgroups = 32 waves per CU); SPT = 8: 16384 slots for up to 8192 (one workgroup per CU).
template <int SPT>
int launch_vjoin(gpc_hip_ctx* c, hipStream_t stream, dim3 grid, bool wide, int W, int H, const gpc_settings* s, int mode,
                 const gpc::RjVirt& v) {
  constexpr int log2s = SPT == 8 ? 14 : 13;
  constexpr size_t lds = ((size_t)8 * ((1u << log2s) + 1) + 15) / 16 * 16;
  auto launch = [&](auto kernel) -> int {
    CHK(allow_dyn_lds(c, reinterpret_cast<const void*>(kernel), lds));
    hipLaunchKernelGGL(kernel, grid, dim3(1024), lds, stream, (const uint32_t*)nullptr, (const uint8_t*)nullptr, W, H,
                       s->disp_high, mode == 0 ? 1 : 0, (const int32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, log2s, 1, v);
    return GPC_OK;
  };
  CHK(wide ? launch(gpc::k_row_join<SPT, 1024, true, true>) : launch(gpc::k_row_join<SPT, 1024, false, true>));
  char name[48];
  snprintf(name, sizeof name, "gpc::k_row_join<%d, 1024, %s, true>", SPT, wide ? "true" : "false");
  name_join_launch(c, name, v.use_list != 0);
  return GPC_OK;
}

// k_ht_join<RPT, NT>, one workgroup per bin of at most NT * RPT records (8 bytes of LDS each)
template <int RPT, int NT>
int launch_htjoin(gpc_hip_ctx* c, hipStream_t stream, dim3 grid, const gpc::HtjArgs& a) {
  constexpr size_t lds = (size_t)8 * NT * RPT;
  CHK(allow_dyn_lds(c, reinterpret_cast<const void*>(gpc::k_ht_join<RPT, NT>), lds));
  hipLaunchKernelGGL((gpc::k_ht_join<RPT, NT>), grid, dim3(NT), lds, stream, a);
  char name[32];
  snprintf(name, sizeof name, "gpc::k_ht_join<%d, %d>", RPT, NT);
  name_join_launch(c, name, a.use_list != 0);
  return GPC_OK;
}

// Non-epipolar matcher by partition + LDS join (k_partition.h).  *done = false when some partition is too large for one
// workgroup (heavily duplicated codes): nothing has been written then and the caller takes the radix-sort path.
int run_partition_match(gpc_hip_ctx* c, const GlobalPlan& g, int W, int H, int npairs, const gpc_settings* s, int mode,
                        const uint8_t* d_cand, void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool* done) {
  *done = false;
  const bool wide = wide_codes(c);
  const int bits = wide ? 32 : code_bits(c);
  gpc::GpLayout L = {};
  // 256 bins (8 top code bits) up to ~1 M record slots per pair; 512 / 1024 for larger images, so that a bin of a textured
  // image still holds about a partition's worth of records (the scatter's runs get shorter: k_partition.h)
  // ... and 2048 beyond 1920x1080
  int lb = 8;
  while (lb < 11 && (double)g.nmax * 0.7 / (double)(1 << lb) > 2800.0) ++lb;
  if (c->gp_log2bins > 0) lb = c->gp_log2bins;
  if (lb > bits) lb = bits;
  L.nbins = 1 << lb;
  L.bshift = bits - lb;
  L.target = c->gp_target;  // records per side a partition aims at: half of what k_row_join<4, 1024> holds (skewed bins, zero-code rows)
  L.cap = GP_NB;
  L.cap_hard = 2 * GP_NB;  // a bin that is large by itself (skewed top code bits) goes to the 8192-record join
  // cuts happen where a running count <= nmax passes a multiple of the target, and around bins of more than
  // GP_NB - target records (k_gp_plan); the join's grid is what the plan really made (read back with the overflow word)
  L.pmax = g.nmax / L.target + 2 * (g.nmax / (GP_NB - L.target)) + 2;
  // ... and a partition is a run of whole bins, so there are never more partitions than bins: without this bound the
  // plan kernel's LDS (8 bytes per possible partition) outgrew a workgroup's 160 KiB from ~6.5 M pixels on and the
  // launch failed where the radix path would have served (3840x2160: 189 KB)
  if (L.pmax > L.nbins) L.pmax = L.nbins;
  L.o_off = 0;
  L.o_rowcnt = L.o_off + 2 * (L.pmax + 1);
  L.o_misc = L.o_rowcnt + L.pmax;
  L.ps = L.o_misc + 8 + GP_BIGCAP;
  PartIo io;
  CHK(partition_io(c, g, H, npairs, d_cand, L, io));
  // gpart: [(bin, chunk) tables][plan block per pair][the four words]
  const size_t tab_ints = (size_t)2 * npairs * L.nbins * L.nchunk;
  const size_t plan_bytes = sizeof(int32_t) * ((size_t)L.ps * npairs + 4);
  CHK(ensure(c, c->gpart, sizeof(int32_t) * tab_ints + plan_bytes));
  int32_t* tabs = (int32_t*)c->gpart.p;
  int32_t* part = tabs + tab_ints;
  int32_t* d_flag = part + (size_t)L.ps * npairs;
  const size_t plan_lds = sizeof(int32_t) * 2 * ((size_t)L.pmax + 1);
  CHK(partition_round<false>(c, g, W, H, npairs, io, L, tabs, d_flag, part, plan_bytes, [&]() -> int {
    CHK(allow_dyn_lds(c, reinterpret_cast<const void*>(gpc::k_gp_plan), plan_lds));
    hipLaunchKernelGGL(gpc::k_gp_plan, dim3(npairs), dim3(GP_THREADS), plan_lds, c->stream, (const int32_t*)tabs,
                       (const int32_t*)c->stats.p, part, L, d_flag);
    return GPC_OK;
  }));
  const CodeRangePlan plan = plan_words<CodeRangePlan>(c);
  if (plan.overflow) return GPC_OK;
  const int maxparts = plan.max_parts > 0 ? plan.max_parts : 1;
  {
    Timed t(c, KID_GLOBAL_MATCH);
    c->launch_name[KID_GLOBAL_MATCH][0] = 0;
    gpc::RjVirt v;
    v.kv = io.kv;
    v.part = part;
    v.staged = (uint32_t*)c->staged.p;
    v.recs = g.bs.recs;
    v.ps = L.ps;
    v.o_off = L.o_off;
    v.o_rowcnt = L.o_rowcnt;
    v.o_misc = L.o_misc;
    v.pmax = L.pmax;
    v.dw = make_divw(W);
    v.vtol = s->vertical_tolerance;
    v.min_recs = -1;
    v.use_list = 0;
    // Every partition goes to the 4096-record launch except the bins that are larger by themselves: those few (19 of
    // 1024 code ranges of a 1920x1080 image with the Tau forest) get a launch of the 8192-record instantiation first, on
    // the second stream: its workgroups (one per CU, 44-48 us per 8 pairs of 1920x1080 as a launch by itself) run beside
    // the 4096-record launch instead of after it.  (Planning the whole batch for the larger kernel, as before, ran every
    // partition at one workgroup per CU.)
    const dim3 jgrid(maxparts, npairs);
    SideLaunch side(c, plan.max_bin_side > GP_NB);
    CHK(side.status);
    if (side.on) {
      gpc::RjVirt big = v;
      big.min_recs = GP_NB;
      big.use_list = plan.max_list <= GP_BIGCAP;  // the plan's work list is the grid; else every partition, nearly all returning at once
      CHK(launch_vjoin<8>(c, c->s_aux, big.use_list ? list_grid(plan.max_list, npairs) : jgrid, wide, W, H, s, mode, big));
      CHK(side.side_done());
    }
    CHK(launch_vjoin<4>(c, c->stream, jgrid, wide, W, H, s, mode, v));
    CHK(side.join());
    hipLaunchKernelGGL(gpc::k_gp_gather, dim3((maxparts + GPG_PARTS - 1) / GPG_PARTS, npairs), dim3(RM_THREADS), 0, c->stream,
                       (const uint32_t*)c->staged.p, (const int32_t*)part, L, g.bs.recs, make_divw(W),
                       mode, d_out, g.bs.out, cap, d_counts, (const int32_t*)c->stats.p, d_ncand);
    HIPCHK(c, hipGetLastError());
  }
  *done = true;
  return GPC_OK;
}

// Non-epipolar mode: the partitioned matcher, or one device-wide stable radix sort per pair (k_global.h).
int run_global_match(gpc_hip_ctx* c, int W, int H, int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand,
                     void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool seq) {
  GlobalPlan g;
  CHK(plan_global(c, W, H, npairs, mode, cap, false, g, seq));
  if (!c->no_partition) {
    bool done = false;
    CHK(run_partition_match(c, g, W, H, npairs, s, mode, d_cand, d_out, cap, d_counts, d_ncand, &done));
    if (done) return GPC_OK;
  }
  const int apply_filter = (mode == 0);
  const int32_t* stats = (const int32_t*)c->stats.p;
  uint32_t* keys[2] = {(uint32_t*)c->gkeys[0].p, (uint32_t*)c->gkeys[1].p};
  uint32_t* vals[2] = {(uint32_t*)c->gvals[0].p, (uint32_t*)c->gvals[1].p};
  {
    Timed t(c, KID_GLOBAL_KEYS);
    launch_radix_records(c, g, W, H, npairs, d_cand, keys[0], vals[0]);
    HIPCHK(c, hipGetLastError());
  }
  {
    Timed t(c, KID_GLOBAL_SORT);
    CHK(radix_passes(c, g, npairs, keys, vals, 4));  // all 32 code bits
  }
  {
    Timed t(c, KID_GLOBAL_MATCH);
    c->launch_name[KID_GLOBAL_MATCH][0] = 0;
    name_join_launch(c, "gpc::k_g_match", false);
    const int ngm = (g.nmax + GMT_TILE - 1) / GMT_TILE;  // <= nmblk, so the match-block counters are large enough
    hipLaunchKernelGGL((gpc::k_g_match<false>), dim3(ngm, npairs), dim3(RM_THREADS), 0, c->stream,
                       (const uint32_t*)keys[0], (const uint32_t*)vals[0], (const int32_t*)g.gmisc, make_divw(W),
                       s->disp_high, s->vertical_tolerance, apply_filter, g.blkcnt, mode, (void*)nullptr, 0,
                       (int32_t*)nullptr, stats, (int32_t*)nullptr, g.bs);
    hipLaunchKernelGGL(gpc::k_g_scan, dim3(1, npairs), dim3(1024), 0, c->stream, g.blkcnt, ngm, (long)g.bs.blk);
    hipLaunchKernelGGL((gpc::k_g_match<true>), dim3(ngm, npairs), dim3(RM_THREADS), 0, c->stream,
                       (const uint32_t*)keys[0], (const uint32_t*)vals[0], (const int32_t*)g.gmisc, make_divw(W),
                       s->disp_high, s->vertical_tolerance, apply_filter, g.blkcnt, mode, d_out, cap, d_counts, stats,
                       d_ncand, g.bs);
    HIPCHK(c, hipGetLastError());
  }
  return GPC_OK;
}

// useHashtable mode by partition into bins of 1024 buckets + one workgroup per bin (k_htjoin.h).  *done = false when a bin
// holds more records than one workgroup takes; nothing has been written then and the caller takes the radix path.
int run_hashtable_partition(gpc_hip_ctx* c, const GlobalPlan& g, int W, int H, int npairs, const gpc_settings* s, int mode,
                            const uint8_t* d_cand, void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool* done) {
  *done = false;
  if (H >= HTJ_MAXH) return GPC_OK;  // positions are packed y << 14 | x
  gpc::GpLayout L = {};
  // Bins of 1024 buckets (210 of them) up to ~1 M record slots per pair, 512 / 256 / 128 buckets per bin for larger
  // images: Hashmatch's buckets are `state % 214673`, so bins fill evenly and the estimate (70 % of the pixels are
  // candidates) may aim at 3500 of the 4096 records a workgroup takes.  The histogram then tells the truth: k_ht_check
  // reports the batch's largest bin, and a bin that does not fit sends the planning round again with as many fewer
  // buckets per bin as that takes (one more histogram, ~0.1 ms per 8 pairs of 1920x1080) instead of the whole batch to the
  // radix path; only a bin that stays too large at 128 buckets -- one state repeated thousands of times (striped images)
  // or more than ~6 M candidates -- goes on to the 8192-record kernel (one workgroup per CU) or, beyond that, the radix path.
  int lbits = HTJ_LBITS;
  while (lbits > 7 && (double)g.nmax * 0.7 / (double)((HM_BUCKETS >> lbits) + 1) > 3500.0) --lbits;
  if (c->ht_hint_w == W && c->ht_hint_h == H && c->ht_hint_lbits > 0 && c->ht_hint_lbits < lbits) lbits = c->ht_hint_lbits;
  if (c->ht_lbits > 0) lbits = c->ht_lbits;
  int rpt = 4;
  L.epi = s->epipolar_mode ? 1 : 0;
  PartIo io;
  CHK(partition_io(c, g, H, npairs, d_cand, L, io));
  int32_t *tabs = nullptr, *bincnt = nullptr, *biglist = nullptr;
  BucketCheck chk;
  for (int attempt = 0;; ++attempt) {
    L.bshift = lbits;
    L.nbins = (int)((HM_BUCKETS + (1u << lbits) - 1) >> lbits);  // 210 / 420 / 839 / 1678
    // gpart: [(bin, chunk) tables][pairs per bin][the four words][work list per pair]
    const size_t tab_ints = (size_t)2 * npairs * L.nbins * L.nchunk;
    const size_t cnt_ints = (size_t)npairs * L.nbins;
    const size_t big_ints = (size_t)npairs * (HTJ_BIGCAP + 1);
    CHK(ensure(c, c->gpart, sizeof(int32_t) * (tab_ints + cnt_ints + 4 + big_ints)));
    tabs = (int32_t*)c->gpart.p;
    bincnt = tabs + tab_ints;
    int32_t* d_flag = bincnt + cnt_ints;
    biglist = d_flag + 4;
    CHK(partition_round<true>(c, g, W, H, npairs, io, L, tabs, d_flag, d_flag, sizeof(int32_t) * (4 + big_ints), [&]() -> int {
      hipLaunchKernelGGL(gpc::k_ht_check, dim3(npairs), dim3(256), 0, c->stream, (const int32_t*)tabs,
                         (const int32_t*)c->stats.p, L.nbins, L.nchunk, HTJ_THREADS * 4, d_flag, 512 * 4, biglist);
      return GPC_OK;
    }));
    chk = plan_words<BucketCheck>(c);
    if (!chk.overflow) {  // every bin fits the 4096-record kernel
      c->ht_hint_w = W;
      c->ht_hint_h = H;
      c->ht_hint_lbits = lbits;
      break;
    }
    // halving the buckets per bin halves an evenly filled bin: how many halvings bring the largest one under 3900?
    int want = lbits;
    while (want > 7 && (chk.max_bin >> (lbits - want)) > 3900) --want;
    if (want < lbits && c->ht_lbits == 0 && attempt < 3) {
      lbits = want;
      continue;
    }
    if (chk.max_bin <= HTJ_THREADS * 8) {  // the 8192-record kernel takes what is left (one workgroup per CU)
      rpt = 8;
      break;
    }
    return GPC_OK;  // the caller sorts instead
  }
  {
    Timed t(c, KID_GLOBAL_MATCH);
    c->launch_name[KID_GLOBAL_MATCH][0] = 0;
    gpc::HtjArgs a;
    a.kv = io.kv;
    a.tabs = tabs;
    a.stats = (const int32_t*)c->stats.p;
    a.staged = (uint2*)c->staged.p;
    a.bincnt = bincnt;
    a.recs = g.bs.recs;
    a.nbins = L.nbins;
    a.nchunk = L.nchunk;
    a.lbits = lbits;
    // Ten-record lists that fill up (k_htjoin.h): measured per-record handling against one wave per bucket --
    // 1920x1080 x8 (13 records per bucket): k_ht_join 787 -> 527 us; 1024x436 x32 (2.7 per bucket): 239 -> 278 us.  The
    // batch's largest record count decides: from 8 records per bucket on.
    a.mid = c->ht_mid > 0 ? c->ht_mid : ((double)chk.max_pair / (double)HM_BUCKETS >= 8.0 ? 32 : HM_CAP);
    a.epi = L.epi;
    a.disp_high = s->disp_high;
    a.vtol = s->vertical_tolerance;
    a.apply_filter = (mode == 0);
    a.dw = make_divw(W);
    a.min_recs = -1;
    a.use_list = 0;
    a.biglist = biglist;
    // 512 threads where the bins are small (k_htjoin.h): at most 512 buckets, and bins of at most 2048 records; the few
    // larger ones (a bucket of repeated states can double a bin) go to a 1024-thread launch on a stream of its own beside it
    const bool half = rpt == 4 && lbits <= 9 && !c->ht_no_half &&
                      (double)chk.max_pair / (double)L.nbins <= 0.9 * 512 * 4;  // the average bin fits comfortably
    if (c->debug_plan)
      fprintf(stderr, "[ht plan] lbits %d bins %d largest bin %d largest pair %d rpt %d half %d mid %d\n", lbits, L.nbins, chk.max_bin,
              chk.max_pair, rpt, (int)half, a.mid);
    const dim3 hgrid(L.nbins, npairs);
    // (every bin is taken by exactly one launch: k_ht_check has seen that none exceeds the largest kernel's capacity)
    if (rpt == 8) {
      CHK((launch_htjoin<8, HTJ_THREADS>(c, c->stream, hgrid, a)));
    } else if (half) {
      SideLaunch side(c, chk.max_bin > 512 * 4);
      CHK(side.status);
      if (side.on) {
        gpc::HtjArgs big = a;
        big.min_recs = 512 * 4;
        big.use_list = chk.max_list <= HTJ_BIGCAP;  // the larger bins' list is the grid; else every bin, nearly all returning at once
        CHK((launch_htjoin<4, HTJ_THREADS>(c, c->s_aux, big.use_list ? list_grid(chk.max_list, npairs) : hgrid, big)));
        CHK(side.side_done());
      }
      CHK((launch_htjoin<4, 512>(c, c->stream, hgrid, a)));
      CHK(side.join());
    } else {
      CHK((launch_htjoin<4, HTJ_THREADS>(c, c->stream, hgrid, a)));
    }
    hipLaunchKernelGGL(gpc::k_ht_gather, dim3((L.nbins + HTG_BINS - 1) / HTG_BINS, npairs), dim3(RM_THREADS), 0, c->stream, a,
                       mode, d_out, g.bs.out, cap, d_counts, d_ncand);
    HIPCHK(c, hipGetLastError());
  }
  *done = true;
  return GPC_OK;
}

// useHashtable mode (hashmatch.hpp): the partitioned matcher, or a stable radix sort by bucket id + one thread per bucket
// (k_hashtable.h)
int run_hashtable_match(gpc_hip_ctx* c, int W, int H, int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand,
                        void* d_out, int cap, int32_t* d_counts, int32_t* d_ncand, bool seq) {
  GlobalPlan g;
  CHK(plan_global(c, W, H, npairs, mode, cap, true, g, seq));
  if (!c->no_partition) {
    bool done = false;
    CHK(run_hashtable_partition(c, g, W, H, npairs, s, mode, d_cand, d_out, cap, d_counts, d_ncand, &done));
    if (done) return GPC_OK;
  }
  const int apply_filter = (mode == 0);
  const int epi = s->epipolar_mode ? 1 : 0;
  const int32_t* stats = (const int32_t*)c->stats.p;
  uint32_t* codes0 = (uint32_t*)c->gkeys[0].p;
  uint32_t* kv0 = (uint32_t*)c->gvals[0].p;
  uint32_t* keys[2] = {(uint32_t*)c->hkeys[0].p, (uint32_t*)c->hkeys[1].p};
  uint32_t* vals[2] = {(uint32_t*)c->hvals[0].p, (uint32_t*)c->hvals[1].p};
  {
    Timed t(c, KID_GLOBAL_KEYS);
    launch_radix_records(c, g, W, H, npairs, d_cand, codes0, kv0);
    hipLaunchKernelGGL(gpc::k_ht_bucket_ids, dim3(g.nmblk, npairs), dim3(256), 0, c->stream,
                       (const uint32_t*)codes0, (const uint32_t*)kv0, (const int32_t*)g.gmisc, make_divw(W), epi, keys[0],
                       vals[0], (uint2*)c->hrec.p, g.bs);
    HIPCHK(c, hipGetLastError());
  }
  {
    Timed t(c, KID_GLOBAL_SORT);
    CHK(radix_passes(c, g, npairs, keys, vals, 3));  // 214673 < 2^18: three 8-bit digits -> result in [1]
  }
  {
    Timed t(c, KID_GLOBAL_MATCH);
    c->launch_name[KID_GLOBAL_MATCH][0] = 0;
    name_join_launch(c, "gpc::k_ht_pairs", false);
    const int nhp = (g.nmax + HP_TILE - 1) / HP_TILE;  // <= nmblk, so the match-block counters are large enough
    hipLaunchKernelGGL((gpc::k_ht_pairs<false>), dim3(nhp, npairs), dim3(HP_THREADS), 0, c->stream,
                       (const uint32_t*)keys[1], (const uint32_t*)vals[1], (const uint2*)c->hrec.p, keys[0],
                       vals[0], (const int32_t*)g.gmisc, make_divw(W), epi, s->disp_high, s->vertical_tolerance,
                       apply_filter, g.blkcnt, mode, (void*)nullptr, 0, (int32_t*)nullptr, stats, (int32_t*)nullptr,
                       g.bs);
    hipLaunchKernelGGL(gpc::k_g_scan, dim3(1, npairs), dim3(1024), 0, c->stream, g.blkcnt, nhp, (long)g.bs.blk);
    hipLaunchKernelGGL((gpc::k_ht_pairs<true>), dim3(nhp, npairs), dim3(HP_THREADS), 0, c->stream,
                       (const uint32_t*)keys[1], (const uint32_t*)vals[1], (const uint2*)c->hrec.p, keys[0],
                       vals[0], (const int32_t*)g.gmisc, make_divw(W), epi, s->disp_high, s->vertical_tolerance,
                       apply_filter, g.blkcnt, mode, d_out, cap, d_counts, stats, d_ncand, g.bs);
    HIPCHK(c, hipGetLastError());
  }
  return GPC_OK;
}

int check_settings(const gpc_settings* s) {
  if (!s) return GPC_E_INVALID;
  if (s->gradient_threshold < 0 || s->gradient_threshold > 255) return GPC_E_INVALID;
  return GPC_OK;
}

int forest_matches(gpc_hip_ctx* c, int W, int H) {
  if (!c->have_forest) return GPC_E_NO_FOREST;
  // the reference asserts FilterMask dims == image dims (inference.hpp:350-353)
  if (c->forest_w != W || c->forest_h != H) return GPC_E_INVALID;
  return GPC_OK;
}

// settings, dimensions and forest are usable for a match of pairs (seq: of consecutive frames).  Group mode has no
// hash-table matcher and no sequences.
int match_usable(gpc_hip_ctx* c, const gpc_settings* s, int W, int H, bool seq) {
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  if (c->ngroups > 1 && (seq || s->use_hashtable)) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// the records of a pair that are there to be read or copied: its count may be negative, or larger than its capacity
inline int valid_records(int count, int cap) { return count < 0 ? 0 : (count > cap ? cap : count); }

// The device's address of page-locked host memory the GPU can write (hipHostMalloc / gpc_hip_host_alloc), or null.
void* device_view_of_host(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not an error of this library
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
  return a.devicePointer;
}

// ---------------------------------------------------------------- device-resident preprocessed images

uint64_t fp_mix(uint64_t h, uint64_t v) {
  h ^= v;
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

// words of `bytes` bytes at p: all of them (full), or 66 spread evenly, first and last included
uint64_t fp_array(uint64_t h, const void* p, size_t bytes, bool full) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  h = fp_mix(h, (uint64_t)bytes);
  if (bytes < 8) {
    for (size_t i = 0; i < bytes; ++i) h = fp_mix(h, b[i]);
    return h;
  }
  const size_t words = bytes / 8;
  auto word = [&](size_t byte_off) {
    uint64_t v;
    memcpy(&v, b + byte_off, 8);
    return v;
  };
  if (full) {
    uint64_t a0 = h, a1 = ~h, a2 = h * 3, a3 = h * 5;  // four chains: the multiply's latency is hidden
    size_t i = 0;
    for (; i + 4 <= words; i += 4) {
      a0 = fp_mix(a0, word(8 * i));
      a1 = fp_mix(a1, word(8 * i + 8));
      a2 = fp_mix(a2, word(8 * i + 16));
      a3 = fp_mix(a3, word(8 * i + 24));
    }
    for (; i < words; ++i) a0 = fp_mix(a0, word(8 * i));
    h = fp_mix(fp_mix(fp_mix(a0, a1), a2), a3);
  } else {
    const size_t samples = words < 65 ? words : 65;
    for (size_t k = 0; k < samples; ++k) h = fp_mix(h, word(8 * (samples > 1 ? k * (words - 1) / (samples - 1) : 0)));
  }
  return fp_mix(h, word(bytes - 8));  // the tail (bytes need not be a multiple of 8)
}

uint64_t fingerprint(const uint8_t* smooth, const uint8_t* grad, size_t n, const int32_t* mask, int n_mask, bool full) {
  uint64_t h = 0x6A09E667F3BCC908ull;
  h = fp_array(h, smooth, n, full);
  h = fp_array(h, grad, n, full);
  return fp_array(h, mask, sizeof(int32_t) * (size_t)n_mask, full);
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na && nb && x < y + nb && y < x + na;
}

// Host memory [p, p + bytes) is about to be (or has been) written by this library: records of ANY context that describe it
// are void.  Call with g_res_mu held.
void drop_overlapping(const void* p, size_t bytes) {
  for (gpc_hip_ctx* o : g_ctxs)
    for (auto& r : o->res) {
      if (!r.valid) continue;
      const size_t n = (size_t)r.W * r.H;
      if (ranges_overlap(p, bytes, r.smooth, n) || ranges_overlap(p, bytes, r.grad, n) ||
          ranges_overlap(p, bytes, r.mask, sizeof(int32_t) * (size_t)r.n_mask))
        r.valid = false;
    }
}

// The slot whose host copies these arrays are, or -1: same addresses, sizes and arithmetic, and the arrays still hold
// what was delivered (fingerprint).
int resident_slot(gpc_hip_ctx* c, const uint8_t* smooth, const uint8_t* grad, const int32_t* mask, int n_mask, int W, int H) {
  if (!c->resident_mode) return -1;
  std::lock_guard<std::mutex> g(g_res_mu);
  for (int k = 0; k < 2; ++k) {
    const gpc_hip_ctx::Resident& r = c->res[k];
    if (!r.valid || r.smooth != smooth || r.grad != grad || r.mask != mask || r.n_mask != n_mask || r.W != W || r.H != H ||
        r.naive != c->naive)
      continue;
    if (fingerprint(smooth, grad, (size_t)W * H, mask, n_mask, c->resident_mode == 2) == r.fp) return k;
  }
  return -1;
}

// Copies between page-locked staging and the caller's pageable arrays, shared among the expansion workers once they
// are worth waking (>= 512 KiB in all); host_copy_wait ends the group.
void host_copy(gpc_hip_ctx* c, void* dst, const void* src, size_t bytes, bool parallel) {
  if (!bytes) return;
  if (!parallel || c->pool.size() < 2) {
    memcpy(dst, src, bytes);
    return;
  }
  const size_t step = 192 * 1024;
  for (size_t at = 0; at < bytes; at += step) {
    ExpandJob j = {};
    j.slot = 6;  // a wait slot of its own (0 .. 3: landing slots of packed results, 7: the bounce buffer)
    j.copy_src = static_cast<const uint8_t*>(src) + at;
    j.copy_dst = static_cast<uint8_t*>(dst) + at;
    j.copy_bytes = at + step <= bytes ? step : bytes - at;
    c->pool.push(j);
  }
}
void host_copy_wait(gpc_hip_ctx* c) {
  if (c->pool.size() >= 1) c->pool.wait_slot(6);  // (whoever pushed: returns at once when nothing is pending)
}

// at least `bytes` of transfer arena; *dev receives the device's view of it
int xfer_reserve(gpc_hip_ctx* c, size_t bytes, uint8_t** dev) {
  if (bytes > c->h_xfer.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(ensure_pinned(c, c->h_xfer, bytes + bytes / 4 + 4096));
  }
  HIPCHK(c, hipHostGetDevicePointer((void**)dev, c->h_xfer.p, 0));
  return GPC_OK;
}

// at least `bytes` of the page-locked landing area of small per-pair words
int pinned_area(gpc_hip_ctx* c, size_t bytes) {
  if (bytes <= c->h_cnt.cap) return GPC_OK;
  return ensure_pinned(c, c->h_cnt, bytes);
}
// ... for npairs counts + 2 * npairs candidate counts
int pinned_counts(gpc_hip_ctx* c, int npairs) { return pinned_area(c, sizeof(int32_t) * 3 * (size_t)npairs); }

// dst[0 .. bytes) = src[0 .. bytes) by a kernel (device memory or device views of page-locked host memory; both 16-byte
// aligned, bytes a multiple of 16): no copy-engine submission, no runtime staging
int dev_copy16(gpc_hip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!bytes) return GPC_OK;
  if ((bytes & 15u) || (((uintptr_t)dst | (uintptr_t)src) & 15u) || bytes / 16 >= (1ull << 32)) return GPC_E_INVALID;
  const unsigned n16 = (unsigned)(bytes / 16);
  hipLaunchKernelGGL(gpc::k_upload2, dim3((n16 + 255) / 256, 1), dim3(256), 0, c->stream, (const uint4*)src, (const uint4*)src,
                     (uint4*)dst, (uint4*)dst, n16);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

inline size_t pad16(size_t v) { return (v + 15) & ~(size_t)15; }

// The chunk pipeline is a few hundred HIP calls and event waits per batch: driven from a CPU of the OTHER socket every
// one of them crosses the inter-socket link on its way to the GPU, and the same 256-pair call takes 7.9 ms instead of
// 5.3 (profiles/r05_c_h2h_numa.txt; which socket a process's main thread lands on is the scheduler's choice, which is
// why one leg of the round-3 and round-4 bench records was slow and the other not).  So when the calling thread runs
// off the GPU's NUMA node -- and the process may use that node's CPUs -- the pipeline runs on a thread of its own, bound
// there like the expansion workers, and the caller waits for it.  The caller's own affinity is never touched.
template <class F>
int on_gpu_node(gpc_hip_ctx* c, int npairs, F&& body) {
  bool hop = c && !c->no_feeder && c->have_node_cpus && npairs >= 4;
  if (hop) {
    // ... or is held on one or two CPUs (a pinned worker of the caller's own pool): the runtime's helper threads are
    // created by whoever makes the first call, inherit that mask and then share the CPU with the pipeline -- the same
    // call took 9.8 ms from a thread pinned to one CPU of the GPU's own node
    const int cpu = sched_getcpu();
    cpu_set_t cur;
    const bool narrow = sched_getaffinity(0, sizeof cur, &cur) == 0 && CPU_COUNT(&cur) < 3 && CPU_COUNT(&c->node_cpus) >= 4;
    hop = narrow || (cpu >= 0 && cpu < CPU_SETSIZE && !CPU_ISSET(cpu, &c->node_cpus));
  }
  if (!hop) return body();
  int st = GPC_E_HIP;
  std::thread t([&] {
    (void)sched_setaffinity(0, sizeof c->node_cpus, &c->node_cpus);
    st = body();
  });
  t.join();
  ++c->fed_calls;
  return st;
}


// Swaps a lane's workspaces, join state and stream into the context's members (and back): the pipeline stages then run on
// the lane exactly as they run on the context.
struct LaneScope {
  gpc_hip_ctx* c;
  gpc_hip_ctx::Lane& l;
  hipStream_t user;
  LaneScope(gpc_hip_ctx* ctx, gpc_hip_ctx::Lane& lane) : c(ctx), l(lane), user(ctx->stream) { swap(); c->stream = l.s; }
  ~LaneScope() { swap(); c->stream = user; }
  void swap() {
    std::swap(c->smooth, l.smooth);
    std::swap(c->grad, l.grad);
    std::swap(c->codes, l.codes);
    std::swap(c->stats, l.stats);
    std::swap(c->jstate, l.jstate);
    std::swap(c->staged, l.staged);
    std::swap(c->rowcnt, l.rowcnt);
    std::swap(c->jstate_granules, l.jstate_granules);
    std::swap(c->join_epoch, l.join_epoch);
    std::swap(c->grad_is_bits, l.grad_is_bits);
  }
};

int ensure_lanes(gpc_hip_ctx* c) {
  for (auto& l : c->lanes) {
    if (l.s) continue;
    HIPCHK(c, l.s.create(hipStreamNonBlocking));
    HIPCHK(c, l.e_in.create(hipEventDisableTiming));
    HIPCHK(c, l.e_hash.create(hipEventDisableTiming));
    HIPCHK(c, l.e_join.create(hipEventDisableTiming));
  }
  return GPC_OK;
}

// every lane's queued work is done (host wait)
int drain_lanes(gpc_hip_ctx* c) {
  for (auto& l : c->lanes)
    if (l.s && l.used) HIPCHK(c, hipStreamSynchronize(l.s));
  return GPC_OK;
}

// A host entry point that fills the transfer arena begins: what a _begin queued may still be writing its results there, so
// it is waited for, and ended as every later call on the context ends it; then the lanes are drained.
int host_call_begin(gpc_hip_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pend.active || c->pre_slot >= 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pend.active = false;
    c->pre_slot = -1;
  }
  if (c->pipeline > 1) CHK(drain_lanes(c));
  return GPC_OK;
}

int ensure_pool(gpc_hip_ctx* c) {
  if (c->pool.size() == 0) {
    int nt = c->expand_threads > 0 ? c->expand_threads : default_expand_threads();
    nt = nt < 1 ? 1 : (nt > 32 ? 32 : nt);
    c->pool.start(nt, c->have_node_cpus ? &c->node_cpus : nullptr, &c->node_l3);
  }
  return GPC_OK;
}

}  // namespace

namespace gpc {
// per-image statistics as k_preprocess leaves them (candidates 0, last candidate row -1, OR of the codes 0): the
// match-from-resident-images path runs k_hash without a k_preprocess before it.  One thread per image.
__global__ void k_stats_init(int32_t* __restrict__ stats, int nimg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nimg) return;
  stats[i * GPC_STAT_STRIDE + GPC_STAT_NCAND] = 0;
  stats[i * GPC_STAT_STRIDE + GPC_STAT_LASTROW] = -1;
  stats[i * GPC_STAT_STRIDE + GPC_STAT_CODEOR] = 0;
  stats[i * GPC_STAT_STRIDE + 3] = 0;
}

// Frame sequences: the statistics of nframes frames -> the pair layout the joins read (image 2p + s of pair p = frame
// p + s), and the candidate count of every frame into ncand[nframes] (optional).  One thread per word.
__global__ void k_seq_stats(const int32_t* __restrict__ fstats, int32_t* __restrict__ pstats, int32_t* __restrict__ ncand,
                            int nframes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nwords = 2 * (nframes - 1) * GPC_STAT_STRIDE;
  if (i < nwords) {
    const int img = i / GPC_STAT_STRIDE, k = i - img * GPC_STAT_STRIDE;
    pstats[i] = fstats[((img >> 1) + (img & 1)) * GPC_STAT_STRIDE + k];
  }
  if (ncand && i < nframes) ncand[i] = fstats[i * GPC_STAT_STRIDE + GPC_STAT_NCAND];
}
}  // namespace gpc

namespace {

// Group mode: hash + match + union of npairs pairs whose smoothed images (and gradient / candidate images) are on the device.
// d_cand_hash: the candidate map k_hash reads (null: the gradient image's); d_cand: the candidate bytes of the matchers.
// The groups' codes go to c->codes as virtual pairs [pair][group][side][H][W] with statistics of their own (vstats); the
// joins run unchanged over the npairs * G virtual pairs into vout (a group has at most one record per left pixel: the
// image's candidate count bounds it), and k_group_union writes each pair's union to d_out[p][cap] (true totals into
// d_counts, candidate counts into d_ncand).
int run_group_match(gpc_hip_ctx* c, const uint8_t* d_sm, const uint8_t* d_gr, const uint8_t* d_cand_hash, int W, int H,
                    int npairs, const gpc_settings* s, int mode, const uint8_t* d_cand, void* d_out, long cap,
                    int32_t* d_counts, int32_t* d_ncand) {
  if (s->use_hashtable) return GPC_E_UNSUPPORTED;  // (its pair / triplet rules may emit a left pixel twice)
  const int G = c->ngroups;
  const size_t n = (size_t)W * H;
  const int npv = npairs * G;
  const size_t esz = mode == 0 ? sizeof(gpc_support) : sizeof(gpc_correspondence);
  const long vcap = (long)(W - 2 * GPC_R) * (H - 2 * GPC_R) + 1;
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * npv));
  CHK(ensure(c, c->vstats, sizeof(int32_t) * GPC_STAT_STRIDE * 2 * npv));
  CHK(ensure(c, c->vout, esz * (size_t)vcap * npv));
  CHK(ensure(c, c->vcnt, sizeof(int32_t) * npv));
  CHK(ensure(c, c->vncand, sizeof(int32_t) * 2 * npv));
  hipLaunchKernelGGL(gpc::k_stats_init, dim3((2 * npv + 63) / 64), dim3(64), 0, c->stream, (int32_t*)c->vstats.p, 2 * npv);
  // (the virtual images' statistics stand in for the real ones while the groups are hashed and joined)
  std::swap(c->stats, c->vstats);
  int st = run_hash(c, d_sm, d_gr, d_cand_hash, W, H, 2 * npairs, false, (uint32_t*)c->codes.p, G, 2);
  const uint8_t* vc = d_cand;
  if (st == GPC_OK && wide_codes(c) && d_cand) {
    // the WIDE joins read the candidate bytes of their (virtual) image: one copy per group
    st = ensure(c, c->vcand, 2 * n * npv);
    for (int p = 0; p < npairs && st == GPC_OK; ++p)
      for (int g = 0; g < G && st == GPC_OK; ++g)
        if (hipMemcpyAsync((uint8_t*)c->vcand.p + (size_t)(p * G + g) * 2 * n, d_cand + (size_t)p * 2 * n, 2 * n,
                           hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
          st = GPC_E_HIP;
    vc = (const uint8_t*)c->vcand.p;
  }
  if (st == GPC_OK)
    st = run_match(c, W, H, npv, s, mode, vc, c->vout.p, (int)vcap, (int32_t*)c->vcnt.p, (int32_t*)c->vncand.p);
  std::swap(c->stats, c->vstats);
  CHK(st);
  const int nchunk = (int)((vcap + UN_CHUNK - 1) / UN_CHUNK);
  CHK(ensure(c, c->uplane, sizeof(uint32_t) * n * npv));
  CHK(ensure(c, c->ublk, sizeof(int32_t) * (size_t)nchunk * npv));
  Timed t(c, KID_GROUP_UNION);
  snprintf(c->launch_name[KID_GROUP_UNION], sizeof c->launch_name[0], "gpc::k_group_union<%s>", mode == 0 ? "false" : "true");
  HIPCHK(c, hipMemsetAsync(c->uplane.p, 0xFF, sizeof(uint32_t) * n * npv, c->stream));
  const dim3 sgrid(nchunk < 512 ? nchunk : 512, npv), cgrid(nchunk, npv);
#define UNION_LAUNCH(CORR)                                                                                                  \
  do {                                                                                                                     \
    typedef gpc::UnRec<CORR> R_;                                                                                           \
    const R_* vo_ = (const R_*)c->vout.p;                                                                                  \
    hipLaunchKernelGGL((gpc::k_group_union_scatter<CORR>), sgrid, dim3(UN_THREADS), 0, c->stream, vo_,                     \
                       (const int32_t*)c->vcnt.p, vcap, W, H, (uint32_t*)c->uplane.p, G);                                  \
    hipLaunchKernelGGL((gpc::k_group_union_count<CORR>), cgrid, dim3(UN_THREADS), 0, c->stream, vo_,                       \
                       (const int32_t*)c->vcnt.p, vcap, W, H, (const uint32_t*)c->uplane.p, G, (int32_t*)c->ublk.p, nchunk); \
    hipLaunchKernelGGL(gpc::k_group_union_scan, dim3(npairs), dim3(1024), 0, c->stream, (int32_t*)c->ublk.p, nchunk, G,    \
                       d_counts, d_ncand, (const int32_t*)c->vstats.p);                                                    \
    hipLaunchKernelGGL((gpc::k_group_union<CORR>), cgrid, dim3(UN_THREADS), 0, c->stream, vo_, (const int32_t*)c->vcnt.p,  \
                       vcap, W, H, (const uint32_t*)c->uplane.p, G, (const int32_t*)c->ublk.p, nchunk, (R_*)d_out, cap);   \
  } while (0)
  if (mode == 0) UNION_LAUNCH(false);
  else UNION_LAUNCH(true);
#undef UNION_LAUNCH
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

}  // namespace

// =================================================================== C ABI

extern "C" {

int gpc_hip_abi_version(void) { return GPC_HIP_ABI_VERSION; }

const char* gpc_hip_status_string(int status) {
  switch (status) {
    case GPC_OK: return "ok";
    case GPC_E_INVALID: return "invalid argument";
    case GPC_E_NO_DEVICE: return "no usable HIP device (gfx950 required)";
    case GPC_E_HIP: return "HIP runtime error";
    case GPC_E_CAPACITY: return "output capacity too small";
    case GPC_E_NO_FOREST: return "no forest set";
    case GPC_E_FOREST_RANGE: return "forest test offset outside the 27x27 patch";
    case GPC_E_IO: return "forest file could not be read";
    case GPC_E_UNSUPPORTED: return "unsupported setting on the HIP path";
    default: return "unknown status";
  }
}

int gpc_hip_device_count(int* count) {
  if (!count) return GPC_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    *count = 0;
    return GPC_E_NO_DEVICE;
  }
  *count = n;
  return GPC_OK;
}

int gpc_hip_create(int device, gpc_hip_ctx** out) {
  if (!out) return GPC_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return GPC_E_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return GPC_E_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GPC_E_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GPC_E_NO_DEVICE;
  gpc_hip_ctx* c = new gpc_hip_ctx();
  c->device = device;
  if (c->own_stream.create(hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return GPC_E_NO_DEVICE;
  }
  c->stream = c->own_stream;
  const char* ht = getenv("GPC_HIP_HASH_TPW");
  if (ht && atoi(ht) > 0 && atoi(ht) <= 64) c->hash_tpw = atoi(ht);
  c->no_partition = getenv("GPC_HIP_NO_PARTITION") != nullptr;
  c->flat_chunks = getenv("GPC_HIP_FLAT_CHUNKS") != nullptr;
  if (const char* e = getenv("GPC_HIP_GP_TARGET")) {
    const int v = atoi(e);
    if (v >= 256 && v <= 3500) c->gp_target = v;
  }
  if (const char* e = getenv("GPC_HIP_GP_LOG2BINS")) {
    const int v = atoi(e);
    if (v >= 8 && v <= 11) c->gp_log2bins = v;
  }
  c->ht_no_half = getenv("GPC_HIP_HT_NO_HALF") != nullptr;
  if (const char* e = getenv("GPC_HIP_HT_MID")) {
    const int v = atoi(e);
    if (v >= HM_CAP && v <= 64) c->ht_mid = v;
  }
  if (const char* e = getenv("GPC_HIP_HT_LBITS")) {
    const int v = atoi(e);
    if (v >= 7 && v <= 10) c->ht_lbits = v;
  }
  if (const char* e = getenv("GPC_HIP_ROWS_PER_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 64) c->rows_per_chunk = v;
  }
  if (const char* e = getenv("GPC_HIP_DIRECT_MAX")) {
    const int v = atoi(e);
    if (v >= 0 && v <= 4096) c->direct_max = v;
  }
  const char* ck = getenv("GPC_HIP_CHUNK");
  if (ck && atoi(ck) > 0 && atoi(ck) <= 1024) c->chunk_pairs = atoi(ck);
  if (const char* e = getenv("GPC_HIP_SEQ_FRAMES")) {
    const int v = atoi(e);
    if (v >= 2 && v <= 1024) c->seq_frames = v;
  }
  if (const char* e = getenv("GPC_HIP_QUAD_STEPS")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 1024) c->quad_steps = v;
  }
  if (const char* e = getenv("GPC_HIP_AGG_GROUP_BYTES")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= AG_GROUP_BYTES) c->agg_group_bytes = v;
  }
  const char* et = getenv("GPC_HIP_EXPAND_THREADS");
  if (et && atoi(et) > 0 && atoi(et) <= 64) c->expand_threads = atoi(et);
  if (const char* e = getenv("GPC_HIP_UPLOAD")) c->upload_mode = atoi(e);
  c->no_grad_bits = getenv("GPC_HIP_NO_GRAD_BITS") != nullptr;
  c->no_feeder = getenv("GPC_HIP_NO_FEEDER") != nullptr;
  c->no_pair_packed = getenv("GPC_HIP_NO_PAIR_PACKED") != nullptr;
  c->no_fuse = getenv("GPC_HIP_NO_FUSE") != nullptr;
  if (const char* e = getenv("GPC_HIP_HASH_TALL")) c->hash_tall = atoi(e) ? 1 : 0;
  if (const char* e = getenv("GPC_HIP_PRE_ROWS")) {
    const int v = atoi(e);
    if (v == PP_ROWS || v == 10 || v == 7 || v == PP_ROWS_MID || v == 4 || v == PP_ROWS_SMALL) c->pre_rows = v;
  }
  c->fuse_always = getenv("GPC_HIP_FUSE_ALWAYS") != nullptr;
  if (const char* e = getenv("GPC_HIP_FUSE_WGS")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 65536) c->fuse_wgs = v;
  }
  if (const char* e = getenv("GPC_HIP_FUSE_SHARDS")) {
    const int v = atoi(e);
    if (v >= 1 && v <= RJ_SHARDS) c->fuse_shards = v;
  }
  if (const char* e = getenv("GPC_HIP_FUSE_MIN_PAIRS")) {
    const int v = atoi(e);
    if (v >= 1) c->fuse_min_pairs = v;
  }
  if (const char* e = getenv("GPC_HIP_RESIDENT")) {
    const int v = atoi(e);
    if (v >= 0 && v <= 2) c->resident_mode = v;
  }
  if (const char* e = getenv("GPC_HIP_EXTRACT_FRAMES")) {
    const int v = atoi(e);
    if (v >= 1) c->extract_frames = v;
  }
  if (const char* e = getenv("GPC_HIP_TRAIN_GROUP")) {
    const int v = atoi(e);
    if (v >= 1) c->train_group = v;
  }
  c->debug = getenv("GPC_HIP_DEBUG") != nullptr;
  c->debug_plan = getenv("GPC_HIP_DEBUG_PLAN") != nullptr;
  c->num_cus = prop.multiProcessorCount;
  find_gpu_node_cpus(c);
  const char* jn = getenv("GPC_HIP_JOIN_NT");
  if (jn && (atoi(jn) == 256 || atoi(jn) == 512 || atoi(jn) == 1024)) c->join_nt = atoi(jn);
  {
    std::lock_guard<std::mutex> g(g_res_mu);
    g_ctxs.push_back(c);
  }
  *out = c;
  return GPC_OK;
}

int gpc_hip_destroy(gpc_hip_ctx* c) {
  if (!c) return GPC_E_INVALID;
  {
    std::lock_guard<std::mutex> g(g_res_mu);
    for (size_t k = 0; k < g_ctxs.size(); ++k)
      if (g_ctxs[k] == c) { g_ctxs.erase(g_ctxs.begin() + k); break; }
  }
  (void)hipSetDevice(c->device);
  (void)drain_lanes(c);
  (void)hipStreamSynchronize(c->stream);
  for (hipStream_t s : {c->own_stream.h, c->s_in.h, c->s_out.h, c->s_cnt.h, c->s_aux.h})
    if (s) (void)hipStreamSynchronize(s);
  // a fused-join time-out nobody has asked about (callers that only ever waited on their own stream): say so, once
  const int pending_err = check_join_err(c);
  if (pending_err != GPC_OK) fprintf(stderr, "gpc_hip_destroy: %s\n", c->err);
  while (!c->train_sets.empty()) (void)gpc_hip_train_set_destroy(c, c->train_sets.back());
  while (!c->track_streams.empty()) (void)gpc_hip_track_stream_destroy(c, c->track_streams.back());
  c->pool.stop();
  delete c;
  return pending_err;
}

const char* gpc_hip_last_error(const gpc_hip_ctx* c) { return c ? c->err : "null context"; }

int gpc_hip_set_stream(gpc_hip_ctx* c, void* hip_stream) {
  if (!c) return GPC_E_INVALID;
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return GPC_OK;
}

int gpc_hip_synchronize(gpc_hip_ctx* c) {
  if (!c) return GPC_E_INVALID;
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return check_join_err(c);
}

int gpc_hip_reserve(gpc_hip_ctx* c, int W, int H, int max_pairs) {
  if (!c || max_pairs <= 0) return GPC_E_INVALID;
  CHK(check_dims(W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  const int nimg = 2 * max_pairs;
  const int G = c->ngroups > 1 ? c->ngroups : 1;  // group mode: codes and statistics per group (virtual pairs)
  CHK(ensure(c, c->raw, n * nimg));
  CHK(ensure(c, c->smooth, n * nimg));
  CHK(ensure(c, c->grad, n * nimg));
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * nimg * G));
  if (G > 1) {
    CHK(ensure(c, c->vstats, sizeof(int32_t) * GPC_STAT_STRIDE * nimg * G));
    CHK(ensure(c, c->vcnt, sizeof(int32_t) * max_pairs * G));
    CHK(ensure(c, c->vncand, sizeof(int32_t) * nimg * G));
    CHK(ensure(c, c->uplane, sizeof(uint32_t) * n * max_pairs * G));
  }
  CHK(ensure(c, c->staged, sizeof(uint32_t) * n * max_pairs));
  CHK(ensure(c, c->rowcnt, sizeof(int32_t) * (size_t)H * nimg));
  CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE * nimg));
  CHK(ensure(c, c->counts, sizeof(int32_t) * nimg));
  CHK(ensure(c, c->ncand, sizeof(int32_t) * nimg));
  return GPC_OK;
}

int gpc_hip_set_arithmetic(gpc_hip_ctx* c, int mode) {
  if (!c || (mode != GPC_ARITH_SSE && mode != GPC_ARITH_NAIVE)) return GPC_E_INVALID;
  if (c->naive != (mode == GPC_ARITH_NAIVE)) ++c->code_gen;
  c->naive = (mode == GPC_ARITH_NAIVE);
  return GPC_OK;
}

int gpc_hip_host_alloc(gpc_hip_ctx* c, uint64_t bytes, void** ptr) {
  if (!c || !ptr || bytes == 0) return GPC_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault));
  return GPC_OK;
}

int gpc_hip_host_free(gpc_hip_ctx* c, void* ptr) {
  if (!c || !ptr) return GPC_E_INVALID;
  HIPCHK(c, hipHostFree(ptr));
  return GPC_OK;
}

// ------------------------------------------------------------------ forest

int gpc_hip_parse_forest(const char* text, int W, int H, gpc_filter_mask* fm) {
  if (!text || !fm) return GPC_E_INVALID;
  memset(fm, 0, sizeof(*fm));
  fm->width = W;
  fm->height = H;
  const char* p = text;
  int num_ferns = 0, nonzero = 0;
  if (!next_int(p, num_ferns)) return GPC_E_IO;
  for (int i = 0; i < num_ferns; ++i) {
    int fern_id, num_tests;
    std::string scale;
    if (!next_int(p, fern_id) || !next_tok(p, scale) || !next_int(p, num_tests)) return GPC_E_IO;
    for (int j = 0; j < num_tests; ++j) {
      int level, ix, iy, jx, jy, tau;
      if (!next_int(p, level) || !next_int(p, ix) || !next_int(p, iy) || !next_int(p, jx) ||
          !next_int(p, jy) || !next_int(p, tau))
        return GPC_E_IO;
      if (fm->num_tests < GPC_MAX_TESTS) {  // inference.hpp:426
        const int t = fm->num_tests++;
        // (two's-complement wrap where the reference's int arithmetic overflows -- undefined there; found by UBSan on a
        // forged file: offsets that large are refused by gpc_hip_set_forest's window check anyway)
        fm->mask[2 * t] = (int32_t)((uint32_t)ix + (uint32_t)iy * (uint32_t)W);
        fm->mask[2 * t + 1] = (int32_t)((uint32_t)jx + (uint32_t)jy * (uint32_t)W);
        fm->tau[t] = tau;
      } else {
        fm->discarded++;
      }
      if (tau != 0) nonzero++;  // discarded tests count too (inference.hpp:433)
    }
  }
  fm->type = nonzero ? 1 : 0;
  return GPC_OK;
}

int gpc_hip_read_forest(const char* path, int W, int H, gpc_filter_mask* fm) {
  if (!path || !fm) return GPC_E_INVALID;
  memset(fm, 0, sizeof(*fm));
  fm->width = W;
  fm->height = H;
  FILE* fp = fopen(path, "rb");
  if (!fp) return GPC_E_IO;
  std::string text;
  char buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
  fclose(fp);
  return gpc_hip_parse_forest(text.c_str(), W, H, fm);
}

}  // extern "C"

namespace {
// The hash kernel's form of a forest: f in SSE order; fn reversed for the Naive arithmetic; ft SSE order with the tall
// tile's LDS offsets
int forest_dev_of(const gpc_filter_mask* fm, GpcForestDev& f, GpcForestDev& fn, GpcForestDev& ft) {
  const int W = fm->width;
  memset(&f, 0, sizeof f);
  memset(&fn, 0, sizeof fn);
  memset(&ft, 0, sizeof ft);
  for (int t = 0; t < fm->num_tests; ++t) {
    int d[4];
    for (int q = 0; q < 2; ++q) {
      // off = dx + dy*W with |dx| <= 13 < W/2: recover (dx, dy)
      const int off = fm->mask[2 * t + q];
      int dy = (off >= 0) ? (off + W / 2) / W : -((-off + W / 2) / W);
      int dx = off - dy * W;
      if (dx < -GPC_R || dx > GPC_R || dy < -GPC_R || dy > GPC_R) return GPC_E_FOREST_RANGE;
      d[2 * q] = dx;
      d[2 * q + 1] = dy;
    }
    // the hash kernel keeps 4 byte-shifted copies of the window: tap (dx,dy) is an aligned dword of copy dx&3
    int offs[2], offt[2];
    for (int q = 0; q < 2; ++q) {
      const int dx = d[2 * q], dy = d[2 * q + 1], sft = dx & 3;
      offs[q] = (sft * HT_COPY + dy * HT_STRIDE + (dx - sft)) / 4;
      offt[q] = (sft * ((HT_Y_TALL + 2 * GPC_R) * HT_STRIDE) + dy * HT_STRIDE + (dx - sft)) / 4;
    }
    f.off[t] = (offs[0] & 0xFFFF) | (offs[1] << 16);
    f.boff[2 * t] = offs[0] * 4;
    f.boff[2 * t + 1] = offs[1] * 4;
    ft.off[t] = (offt[0] & 0xFFFF) | (offt[1] << 16);   // (the byte offsets are what the kernels read)
    ft.boff[2 * t] = offt[0] * 4;
    ft.boff[2 * t + 1] = offt[1] * 4;
    f.tau[t] = (int)(int8_t)fm->tau[t];  // _mm_set1_epi8(tau) truncates (filter.hpp:651)
    if ((fm->tau[t] & 0xFF) == 0x80) f.tau_m128 = 1;
    // gpcFilterNaive shifts the code left per test: test t ends on bit T-1-t (filter.hpp:245-249)
    const int u = fm->num_tests - 1 - t;
    fn.off[u] = f.off[t];
    fn.boff[2 * u] = f.boff[2 * t];
    fn.boff[2 * u + 1] = f.boff[2 * t + 1];
    fn.tau[u] = fm->tau[t];              // gpcFilterTauNaive uses the int as is (:276)
  }
  memcpy(ft.tau, f.tau, sizeof f.tau);
  ft.tau_m128 = f.tau_m128;
  for (int t = 0; t < fm->num_tests; ++t) {
    const uint32_t tb = (uint32_t)fm->tau[t] & 0xFFu;
    f.tauk[t] = ft.tauk[t] = (int32_t)(tb == 0 ? 0u : f.tau_m128 ? tb * 0x01000100u : (((tb - 1u) & 0xFFu) * 0x01000100u) | 0x00FF00FFu);
  }
  f.num_tests = fn.num_tests = ft.num_tests = fm->num_tests;
  f.type = fn.type = ft.type = fm->type ? 1 : 0;
  return GPC_OK;
}
}  // namespace

extern "C" {

int gpc_hip_set_forest(gpc_hip_ctx* c, const gpc_filter_mask* fm) {
  if (!c || !fm) return GPC_E_INVALID;
  if (fm->num_tests < 0 || fm->num_tests > GPC_MAX_TESTS) return GPC_E_INVALID;
  CHK(check_dims(fm->width, fm->height));
  // The header-only C++ API is stateless like the reference's Forest and hands the forest over with every match call:
  // the same tests again must not cost a stream synchronisation and a blocking copy (~30 us of a 0.2 ms call)
  // (group mode leaves forest_src invalid: the same forest as before group mode is set again)
  if (c->have_forest && fm->num_tests == c->forest_src.num_tests && fm->type == c->forest_src.type &&
      fm->width == c->forest_src.width && fm->height == c->forest_src.height &&
      memcmp(fm->mask, c->forest_src.mask, sizeof(int32_t) * 2 * (size_t)fm->num_tests) == 0 &&
      memcmp(fm->tau, c->forest_src.tau, sizeof(int32_t) * (size_t)fm->num_tests) == 0)
    return GPC_OK;
  GpcForestDev f, fn, ft;
  CHK(forest_dev_of(fm, f, fn, ft));
  ++c->code_gen;
  c->forest = f;
  c->forest_naive = fn;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure(c, c->forest_dev, 3 * sizeof(GpcForestDev)));
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // a launch in flight may still read the previous tests
  const GpcForestDev both[3] = {f, fn, ft};
  HIPCHK(c, hipMemcpy(c->forest_dev.p, both, sizeof both, hipMemcpyHostToDevice));
  c->forest_w = fm->width;
  c->forest_h = fm->height;
  c->forest_src = *fm;
  c->have_forest = true;
  c->ngroups = 0;
  return GPC_OK;
}

int gpc_hip_parse_forest_groups(const char* text, int W, int H, gpc_filter_mask* groups, int cap, int* n_groups) {
  if (!text || !n_groups || cap < 0 || (cap > 0 && !groups)) return GPC_E_INVALID;
  *n_groups = 0;
  // the whole text first (a truncated file yields GPC_E_IO and no groups, as gpc_hip_parse_forest)
  struct Test { int ix, iy, jx, jy, tau; };
  std::vector<std::vector<Test>> ferns;
  const char* p = text;
  int num_ferns = 0;
  if (!next_int(p, num_ferns)) return GPC_E_IO;
  for (int i = 0; i < num_ferns; ++i) {
    int fern_id, num_tests;
    std::string scale;
    if (!next_int(p, fern_id) || !next_tok(p, scale) || !next_int(p, num_tests)) return GPC_E_IO;
    ferns.emplace_back();
    for (int j = 0; j < num_tests; ++j) {
      int level;
      Test t;
      if (!next_int(p, level) || !next_int(p, t.ix) || !next_int(p, t.iy) || !next_int(p, t.jx) || !next_int(p, t.jy) ||
          !next_int(p, t.tau))
        return GPC_E_IO;
      ferns.back().push_back(t);
    }
  }
  // greedy packing: a group takes the next fern while it stays <= 32 tests; a longer fern is cut into chunks of 32 (the
  // remainder last), each a group of its own
  std::vector<std::vector<Test>> packed;
  bool open = false;  // the last group may take more ferns
  for (const auto& f : ferns) {
    if ((int)f.size() > GPC_MAX_TESTS) {
      for (size_t k = 0; k < f.size(); k += GPC_MAX_TESTS)
        packed.emplace_back(f.begin() + k, f.begin() + std::min(f.size(), k + GPC_MAX_TESTS));
      open = false;
    } else if (open && packed.back().size() + f.size() <= GPC_MAX_TESTS) {
      packed.back().insert(packed.back().end(), f.begin(), f.end());
    } else if (!f.empty() || !open) {
      packed.push_back(f);
      open = true;
    }
  }
  if (packed.empty()) packed.emplace_back();  // (no tests at all: the empty forest gpc_hip_parse_forest gives)
  const int ng = (int)packed.size();
  *n_groups = ng;
  if (ng > GPC_MAX_GROUPS) return GPC_E_UNSUPPORTED;
  for (int g = 0; g < ng && g < cap; ++g) {
    gpc_filter_mask* fm = &groups[g];
    memset(fm, 0, sizeof(*fm));
    fm->width = W;
    fm->height = H;
    int nonzero = 0;
    for (const Test& t : packed[(size_t)g]) {
      const int k = fm->num_tests++;
      fm->mask[2 * k] = (int32_t)((uint32_t)t.ix + (uint32_t)t.iy * (uint32_t)W);   // (as gpc_hip_parse_forest)
      fm->mask[2 * k + 1] = (int32_t)((uint32_t)t.jx + (uint32_t)t.jy * (uint32_t)W);
      fm->tau[k] = t.tau;
      if (t.tau != 0) nonzero++;
    }
    fm->type = nonzero ? 1 : 0;
  }
  return ng > cap ? GPC_E_CAPACITY : GPC_OK;
}

int gpc_hip_read_forest_groups(const char* path, int W, int H, gpc_filter_mask* groups, int cap, int* n_groups) {
  if (!path || !n_groups || cap < 0 || (cap > 0 && !groups)) return GPC_E_INVALID;
  *n_groups = 0;
  FILE* fp = fopen(path, "rb");
  if (!fp) return GPC_E_IO;
  std::string text;
  char buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
  fclose(fp);
  return gpc_hip_parse_forest_groups(text.c_str(), W, H, groups, cap, n_groups);
}

int gpc_hip_set_forest_groups(gpc_hip_ctx* c, const gpc_filter_mask* groups, int n_groups) {
  if (!c || !groups || n_groups < 1 || n_groups > GPC_MAX_GROUPS) return GPC_E_INVALID;
  if (n_groups == 1) return gpc_hip_set_forest(c, groups);
  if (c->pipeline > 1) return GPC_E_UNSUPPORTED;
  std::vector<GpcForestDev> dev((size_t)3 * GPC_MAX_GROUPS);
  int maxt = 0;
  bool tau = false;
  for (int g = 0; g < n_groups; ++g) {
    const gpc_filter_mask* fm = &groups[g];
    if (fm->num_tests < 0 || fm->num_tests > GPC_MAX_TESTS) return GPC_E_INVALID;
    if (fm->width != groups[0].width || fm->height != groups[0].height) return GPC_E_INVALID;
    CHK(check_dims(fm->width, fm->height));
    CHK(forest_dev_of(fm, dev[(size_t)g], dev[(size_t)GPC_MAX_GROUPS + g], dev[(size_t)2 * GPC_MAX_GROUPS + g]));
    maxt = std::max(maxt, fm->num_tests);
    tau = tau || fm->type != 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  ++c->code_gen;
  CHK(ensure(c, c->gforest_dev, sizeof(GpcForestDev) * dev.size()));
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // a launch in flight may still read the previous tests
  HIPCHK(c, hipMemcpy(c->gforest_dev.p, dev.data(), sizeof(GpcForestDev) * dev.size(), hipMemcpyHostToDevice));
  c->forest = dev[0];
  c->forest_naive = dev[(size_t)GPC_MAX_GROUPS];
  c->forest_w = groups[0].width;
  c->forest_h = groups[0].height;
  c->forest_src.num_tests = -1;  // (no forest of gpc_hip_set_forest is current)
  c->gmax_tests = maxt;
  c->gtau = tau;
  c->ngroups = n_groups;
  c->have_forest = true;
  return GPC_OK;
}

// ------------------------------------------------------------------ host-buffer entry points

// Forest::preprocessImage in two steps (the one-call form below is both): _begin runs the kernels and leaves smooth,
// grad and the candidate list in page-locked staging memory of the context -- the device writes them there over the link
// itself -- and says how many candidates there are; _fetch copies them into the caller's arrays (which can be sized by
// then) and remembers those arrays as the host copies of an image that is still on the device (resident_slot).
static int preprocess_begin(gpc_hip_ctx* c, const uint8_t* raw, int W, int H, int thr, bool want_mask) {
  if (!c || !raw) return GPC_E_INVALID;
  if (thr < 0 || thr > 255) return GPC_E_INVALID;
  CHK(check_dims(W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  const size_t maxcand = (size_t)(W - 2 * GPC_R) * (H - 2 * GPC_R);
  c->pre_slot = -1;
  c->pend.active = false;
  if (n != c->res_n || !c->res_smooth.p) {  // another image size: both resident images go
    {
      std::lock_guard<std::mutex> g(g_res_mu);
      c->res[0].valid = c->res[1].valid = false;
    }
    CHK(ensure(c, c->res_smooth, 2 * n));
    CHK(ensure(c, c->res_grad, 2 * n));
    c->res_n = n;
  }
  if (!c->e_pre) HIPCHK(c, c->e_pre.create(hipEventDisableTiming));
  // staging: raw | smooth | grad | mask (every candidate a pixel can be) | count   (all offsets multiples of 16)
  const size_t mask_bytes = pad16(sizeof(int32_t) * maxcand);
  const size_t need = 3 * n + mask_bytes + 64;
  if (need > c->h_pre.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(ensure_pinned(c, c->h_pre, need + need / 8));
  }
  uint8_t* d_stage = nullptr;  // the device's view of the staging block
  HIPCHK(c, hipHostGetDevicePointer((void**)&d_stage, c->h_pre.p, 0));
  const int slot = c->res_next;
  {
    std::lock_guard<std::mutex> g(g_res_mu);
    c->res[slot].valid = false;
  }
  uint8_t* d_sm = (uint8_t*)c->res_smooth.p + (size_t)slot * n;
  uint8_t* d_gr = (uint8_t*)c->res_grad.p + (size_t)slot * n;
  CHK(ensure(c, c->raw, n));
  CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE * 2));
  // the image: a page-locked one is read where it lies, a pageable one (ndb::Buffer, std::vector) passes through staging
  const uint8_t* v_raw = static_cast<const uint8_t*>(device_view_of_host(raw));
  if (!v_raw || ((uintptr_t)v_raw & 15u)) {
    memcpy(c->h_pre.p, raw, n);
    v_raw = d_stage;
  }
  CHK(dev_copy16(c, c->raw.p, v_raw, n));
  CHK(run_preprocess(c, (const uint8_t*)c->raw.p, nullptr, W, H, 1, 1, thr, false, d_sm, d_gr));
  // smooth and grad leave over the link while the candidate list is made
  const unsigned n16 = (unsigned)(n / 16);
  hipLaunchKernelGGL(gpc::k_upload2, dim3((n16 + 255) / 256, 2), dim3(256), 0, c->stream, (const uint4*)d_sm, (const uint4*)d_gr,
                     (uint4*)(d_stage + n), (uint4*)(d_stage + 2 * n), n16);
  HIPCHK(c, hipEventRecord(c->e_pre, c->stream));
  if (want_mask) {
    CHK(ensure(c, c->rowcnt, sizeof(int32_t) * (size_t)H * 2));
    dim3 grid(H - 2 * GPC_R, 1);
    Timed t(c, KID_MASK);
    hipLaunchKernelGGL(gpc::k_mask_count, grid, dim3(RM_THREADS), 0, c->stream, (const uint8_t*)d_gr, W, H, (int32_t*)c->rowcnt.p);
    hipLaunchKernelGGL(gpc::k_mask_write, grid, dim3(RM_THREADS), 0, c->stream, (const uint8_t*)d_gr, W, H,
                       (const int32_t*)c->rowcnt.p, reinterpret_cast<int32_t*>(d_stage + 3 * n), (int)maxcand,
                       reinterpret_cast<int32_t*>(d_stage + 3 * n + mask_bytes));
  }
  HIPCHK(c, hipGetLastError());
  c->pre_slot = slot;
  c->pre_W = W;
  c->pre_H = H;
  c->pre_have_mask = want_mask;
  return GPC_OK;
}

static int preprocess_fetch(gpc_hip_ctx* c, uint8_t* smooth, uint8_t* grad, int32_t* mask, int mask_cap, int* n_mask) {
  if (!c || c->pre_slot < 0 || mask_cap < 0) return GPC_E_INVALID;
  const int slot = c->pre_slot, W = c->pre_W, H = c->pre_H;
  c->pre_slot = -1;
  const size_t n = (size_t)W * H;
  const size_t maxcand = (size_t)(W - 2 * GPC_R) * (H - 2 * GPC_R);
  const size_t mask_bytes = pad16(sizeof(int32_t) * maxcand);
  const uint8_t* h_smooth = c->h_pre.p + n;
  const uint8_t* h_grad = h_smooth + n;
  const int32_t* h_mask = reinterpret_cast<const int32_t*>(h_grad + n);
  const int32_t* h_count = reinterpret_cast<const int32_t*>(h_grad + n + mask_bytes);
  {
    std::lock_guard<std::mutex> g(g_res_mu);  // whatever these arrays were the host copies of, they are no longer
    drop_overlapping(smooth, smooth ? n : 0);
    drop_overlapping(grad, grad ? n : 0);
    drop_overlapping(mask, sizeof(int32_t) * (size_t)(mask ? mask_cap : 0));
  }
  const bool par = n >= 128 * 1024;
  if (par) CHK(ensure_pool(c));
  // the two images first (they have landed when e_pre has passed), the candidate list when the stream is done
  HIPCHK(c, hipEventSynchronize(c->e_pre));
  if (smooth) host_copy(c, smooth, h_smooth, n, par);
  if (grad) host_copy(c, grad, h_grad, n, par);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int cnt = c->pre_have_mask ? h_count[0] : 0;
  if (n_mask) *n_mask = cnt;
  const int ncopy = (mask && c->pre_have_mask) ? (cnt < mask_cap ? cnt : mask_cap) : 0;
  if (ncopy) host_copy(c, mask, h_mask, sizeof(int32_t) * (size_t)ncopy, par);
  uint64_t fp = 0;
  const bool record = c->resident_mode && smooth && grad && c->pre_have_mask && (mask || cnt == 0) && cnt <= mask_cap;
  if (record) fp = fingerprint(h_smooth, h_grad, n, h_mask, cnt, c->resident_mode == 2);  // (the staging copy: the same bytes)
  if (par) host_copy_wait(c);
  if (record) {
    std::lock_guard<std::mutex> g(g_res_mu);
    gpc_hip_ctx::Resident& r = c->res[slot];
    r.smooth = smooth;
    r.grad = grad;
    r.mask = mask;
    r.n_mask = cnt;
    r.W = W;
    r.H = H;
    r.naive = c->naive;
    r.fp = fp;
    r.valid = true;
    c->res_next = slot ^ 1;
  }
  return (mask && c->pre_have_mask && cnt > mask_cap) ? GPC_E_CAPACITY : GPC_OK;
}

int gpc_hip_preprocess_begin(gpc_hip_ctx* c, const uint8_t* raw, int W, int H, int thr) {
  return preprocess_begin(c, raw, W, H, thr, true);
}

int gpc_hip_preprocess_fetch(gpc_hip_ctx* c, uint8_t* smooth, uint8_t* grad, int32_t* mask, int mask_cap, int* n_mask) {
  return preprocess_fetch(c, smooth, grad, mask, mask_cap, n_mask);
}

int gpc_hip_preprocess(gpc_hip_ctx* c, const uint8_t* raw, int W, int H, int thr, uint8_t* smooth,
                       uint8_t* grad, int32_t* mask, int mask_cap, int* n_mask) {
  CHK(preprocess_begin(c, raw, W, H, thr, n_mask || mask));
  return preprocess_fetch(c, smooth, grad, mask, mask ? mask_cap : 0, n_mask);
}

int gpc_hip_resident_hits(const gpc_hip_ctx* c) { return c ? c->resident_hits : 0; }

int gpc_hip_hash_codes(gpc_hip_ctx* c, const uint8_t* smooth, const uint8_t* grad, int W, int H,
                       uint32_t* codes) {
  if (!c || !smooth || !grad || !codes) return GPC_E_INVALID;
  if (c->ngroups > 1) return GPC_E_UNSUPPORTED;  // (gpc_hip_hash_codes_groups)
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  CHK(ensure(c, c->smooth, n));
  CHK(ensure(c, c->grad, n));
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n));
  CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE));
  // (the caller's arrays pass through the page-locked arena: gpc_hip_ctx::h_xfer)
  uint8_t* d_arena = nullptr;
  CHK(xfer_reserve(c, 4 * n, &d_arena));
  CHK(ensure_pool(c));
  host_copy(c, c->h_xfer.p, smooth, n, true);
  host_copy(c, c->h_xfer.p + n, grad, n, true);
  host_copy_wait(c);
  CHK(dev_copy16(c, c->smooth.p, d_arena, n));
  c->grad_is_bits = false;  // the caller's byte image
  CHK(dev_copy16(c, c->grad.p, d_arena + n, n));
  // the reference's zero-filled gpcstates buffer (inference.hpp:274): the kernel writes the candidate rows only
  HIPCHK(c, hipMemsetAsync(c->codes.p, 0, sizeof(uint32_t) * n, c->stream));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 1, true,
               (uint32_t*)c->codes.p));
  CHK(dev_copy16(c, d_arena, c->codes.p, sizeof(uint32_t) * n));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  host_copy(c, codes, c->h_xfer.p, sizeof(uint32_t) * n, true);
  host_copy_wait(c);
  return GPC_OK;
}

int gpc_hip_hash_codes_groups(gpc_hip_ctx* c, const uint8_t* smooth, const uint8_t* grad, int W, int H, uint32_t* codes) {
  if (!c || !smooth || !grad || !codes) return GPC_E_INVALID;
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const int G = c->ngroups > 1 ? c->ngroups : 1;
  const size_t n = (size_t)W * H;
  CHK(ensure(c, c->smooth, n));
  CHK(ensure(c, c->grad, n));
  CHK(ensure(c, c->gdense, sizeof(uint32_t) * n * G));
  uint8_t* d_arena = nullptr;
  CHK(xfer_reserve(c, sizeof(uint32_t) * n * G, &d_arena));
  CHK(ensure_pool(c));
  host_copy(c, c->h_xfer.p, smooth, n, true);
  host_copy(c, c->h_xfer.p + n, grad, n, true);
  host_copy_wait(c);
  CHK(dev_copy16(c, c->smooth.p, d_arena, n));
  c->grad_is_bits = false;
  CHK(dev_copy16(c, c->grad.p, d_arena + n, n));
  HIPCHK(c, hipMemsetAsync(c->gdense.p, 0, sizeof(uint32_t) * n * G, c->stream));  // (the reference's zero-filled buffer)
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 1, true, (uint32_t*)c->gdense.p,
               G > 1 ? G : 0, 1));
  CHK(dev_copy16(c, d_arena, c->gdense.p, sizeof(uint32_t) * n * G));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  host_copy(c, codes, c->h_xfer.p, sizeof(uint32_t) * n * G, true);
  host_copy_wait(c);
  return GPC_OK;
}

// Queues hash + match of two preprocessed images; the results go to the transfer arena (cap_dev records at most; the
// caller's page-locked array instead when direct_out is its device view) and are collected by match_fetch.
static int match_preprocessed_begin(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL,
                                    const int32_t* maskL, int nL, const uint8_t* smoothR, const uint8_t* gradR,
                                    const int32_t* maskR, int nR, int W, int H, const gpc_settings* s, int mode,
                                    int cap_dev, void* direct_out) {
  if (!c || !smoothL || !gradL || !smoothR || !gradR || cap_dev < 0) return GPC_E_INVALID;
  if ((nL > 0 && !maskL) || (nR > 0 && !maskR) || nL < 0 || nR < 0) return GPC_E_INVALID;
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  c->pend.active = false;
  c->pre_slot = -1;
  const size_t n = (size_t)W * H;
  const size_t esz = mode == 0 ? sizeof(gpc_support) : sizeof(gpc_correspondence);
  if ((uint64_t)cap_dev * esz >= (1ull << 32)) return GPC_E_UNSUPPORTED;  // (beyond 2^30 pixels anyway)
  CHK(ensure(c, c->codes, sizeof(uint32_t) * 2 * n));
  CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE * 2));
  CHK(pinned_counts(c, 1));
  int32_t* d_cnt = nullptr;
  HIPCHK(c, hipHostGetDevicePointer((void**)&d_cnt, c->h_cnt.p, 0));
  // Supports of the epipolar sort-matcher cross the link PACKED (x | xR << 16 + the row counts: 4 bytes instead of 12 -- a
  // 1024x436 pair's 3.2 MB of records were 60 us of the link, a third of the call) and are expanded into the caller's
  // array by the worker threads, who read 1.1 MB where they copied 3.2
  // (group mode: the union stays on the device until match_fetch knows its size)
  const bool groups = c->ngroups > 1;
  if (groups) {
    if (s->use_hashtable) return GPC_E_UNSUPPORTED;
    direct_out = nullptr;
  }
  const bool packed = mode == 0 && !direct_out && s->epipolar_mode && !s->use_hashtable && !c->no_pair_packed && !groups;
  const size_t rows_bytes = pad16(sizeof(int32_t) * (size_t)H);
  const size_t out_bytes = groups ? 0
                           : packed ? rows_bytes + pad16(sizeof(uint32_t) * (size_t)(cap_dev > 0 ? cap_dev : 1))
                                    : pad16(esz * (size_t)(cap_dev > 0 ? cap_dev : 1));
  const int sl = resident_slot(c, smoothL, gradL, maskL, nL, W, H);
  const int sr = sl >= 0 ? resident_slot(c, smoothR, gradR, maskR, nR, W, H) : -1;
  const bool resident = sl >= 0 && sr >= 0;
  // arena: [results | smooth L R | grad L R | mask L | mask R]; the inputs only on the upload path
  const size_t mL = pad16(sizeof(int32_t) * (size_t)nL), mR = pad16(sizeof(int32_t) * (size_t)nR);
  uint8_t* d_arena = nullptr;
  const size_t in_bytes = resident ? 0 : 4 * n + mL + mR;
  // (group mode from resident images: nothing crosses the link before match_fetch)
  if ((!direct_out && out_bytes) || in_bytes) CHK(xfer_reserve(c, (direct_out ? 0 : out_bytes) + in_bytes, &d_arena));
  const size_t in_off = direct_out ? 0 : out_bytes;
  void* d_out = direct_out ? direct_out : d_arena;
  const uint8_t* d_sm = nullptr;
  const uint8_t* d_gr = nullptr;
  const uint8_t* d_cand = nullptr;
  if (resident) {
    // Both images are the host copies of images gpc_hip_preprocess left on the device: hash and match from there.  Their
    // candidates are the gradient image's (the mask list IS that image's non-zero pixels inside the margin), so the
    // pipeline is the batched one without its first kernel.
    d_sm = (const uint8_t*)c->res_smooth.p;
    d_gr = (const uint8_t*)c->res_grad.p;
    if (!(sl == 0 && sr == 1)) {  // right before left, or one image on both sides: put them in pair order
      CHK(ensure(c, c->smooth, 2 * n));
      CHK(ensure(c, c->grad, 2 * n));
      const int src[2] = {sl, sr};
      for (int k = 0; k < 2; ++k) {
        CHK(dev_copy16(c, (uint8_t*)c->smooth.p + k * n, d_sm + src[k] * n, n));
        CHK(dev_copy16(c, (uint8_t*)c->grad.p + k * n, d_gr + src[k] * n, n));
      }
      d_sm = (const uint8_t*)c->smooth.p;
      d_gr = (const uint8_t*)c->grad.p;
    }
    d_cand = d_gr;
    ++c->resident_hits;
  } else {
    CHK(ensure(c, c->smooth, 2 * n));
    CHK(ensure(c, c->grad, 2 * n));
    CHK(ensure(c, c->candmap, 2 * n));
    uint8_t* h_in = c->h_xfer.p + in_off;
    const bool par = in_bytes >= 512 * 1024;
    if (par) CHK(ensure_pool(c));
    host_copy(c, h_in, smoothL, n, par);
    host_copy(c, h_in + n, smoothR, n, par);
    host_copy(c, h_in + 2 * n, gradL, n, par);
    host_copy(c, h_in + 3 * n, gradR, n, par);
    host_copy(c, h_in + 4 * n, maskL, sizeof(int32_t) * (size_t)nL, par);
    host_copy(c, h_in + 4 * n + mL, maskR, sizeof(int32_t) * (size_t)nR, par);
    if (par) host_copy_wait(c);
    const uint8_t* d_in = d_arena + in_off;
    CHK(dev_copy16(c, c->smooth.p, d_in, 2 * n));
    CHK(dev_copy16(c, c->grad.p, d_in + 2 * n, 2 * n));
    uint8_t* d_cm = (uint8_t*)c->candmap.p;
    HIPCHK(c, hipMemsetAsync(d_cm, 0, 2 * n, c->stream));
    // the mask lists are read where they lie (over the link, once)
    if (nL > 0)
      hipLaunchKernelGGL(gpc::k_scatter_mask, dim3((nL + 255) / 256), dim3(256), 0, c->stream,
                         reinterpret_cast<const int32_t*>(d_in + 4 * n), nL, d_cm, W, H);
    if (nR > 0)
      hipLaunchKernelGGL(gpc::k_scatter_mask, dim3((nR + 255) / 256), dim3(256), 0, c->stream,
                         reinterpret_cast<const int32_t*>(d_in + 4 * n + mL), nR, d_cm + n, W, H);
    HIPCHK(c, hipGetLastError());
    d_sm = (const uint8_t*)c->smooth.p;
    d_gr = (const uint8_t*)c->grad.p;
    d_cand = d_cm;
  }
  c->grad_is_bits = false;  // byte images
  c->pend.dev_out = nullptr;
  if (groups) {
    const long cap_u = (long)c->ngroups * ((long)(W - 2 * GPC_R) * (H - 2 * GPC_R)) + 1;
    CHK(ensure(c, c->gdense, esz * (size_t)cap_u));
    CHK(run_group_match(c, d_sm, d_gr, resident ? nullptr : d_cand, W, H, 1, s, mode, d_cand, c->gdense.p, cap_u, d_cnt,
                        nullptr));
    cap_dev = (int)std::min(cap_u, (long)INT32_MAX);
    c->pend.dev_out = c->gdense.p;
  } else {
  hipLaunchKernelGGL(gpc::k_stats_init, dim3(1), dim3(64), 0, c->stream, (int32_t*)c->stats.p, 2);
  CHK(run_hash(c, d_sm, d_gr, resident ? nullptr : d_cand, W, H, 2, false, (uint32_t*)c->codes.p));
  if (packed) {
    const PackedOut po = {reinterpret_cast<int32_t*>(d_arena), (long)cap_dev, (long)H};
    CHK(run_match(c, W, H, 1, s, 2, d_cand, d_arena + rows_bytes, cap_dev, d_cnt, nullptr, &po));
  } else {
    CHK(run_match(c, W, H, 1, s, mode, d_cand, d_out, cap_dev, d_cnt, nullptr));
  }
  }
  c->pend.active = true;
  c->pend.direct = direct_out != nullptr;
  c->pend.have_ncand = false;
  c->pend.packed = packed;
  c->pend.esz = esz;
  c->pend.cap_dev = cap_dev;
  c->pend.H = H;
  return GPC_OK;
}

// Waits for what a *_begin queued and delivers min(count, cap) records; the true count always.  May be called again
// (a larger array after GPC_E_CAPACITY) until the next call on the context.
static int match_fetch(gpc_hip_ctx* c, void* out, int cap, int* n_out, int* ncl, int* ncr) {
  if (!c || !c->pend.active || !n_out || cap < 0 || (cap > 0 && !out)) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHK(check_join_err(c));
  const int32_t cnt = c->h_cnt.p[0];
  *n_out = cnt;
  if (c->pend.have_ncand) {
    if (ncl) *ncl = c->h_cnt.p[1];
    if (ncr) *ncr = c->h_cnt.p[2];
  }
  int ncopy = cnt < cap ? cnt : cap;
  if (ncopy > c->pend.cap_dev) ncopy = c->pend.cap_dev;
  if (c->pend.dev_out && ncopy > 0) {
    // group mode: the first ncopy records of the union into the arena, then into the caller's array
    const size_t bytes = c->pend.esz * (size_t)ncopy;
    uint8_t* d_arena = nullptr;
    CHK(xfer_reserve(c, bytes, &d_arena));
    HIPCHK(c, hipMemcpyAsync(c->h_xfer.p, c->pend.dev_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool par = bytes >= 256 * 1024;
    if (par) CHK(ensure_pool(c));
    host_copy(c, out, c->h_xfer.p, bytes, par);
    if (par) host_copy_wait(c);
  } else if (c->pend.packed && ncopy > 0) {
    const int H = c->pend.H;
    const int32_t* rows = reinterpret_cast<const int32_t*>(c->h_xfer.p);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(c->h_xfer.p + pad16(sizeof(int32_t) * (size_t)H));
    const bool par = ncopy >= 32 * 1024;
    if (par) CHK(ensure_pool(c));
    const int parts = par ? (c->pool.size() > 1 ? c->pool.size() : 1) : 1;
    long first = 0;
    for (int q = 0; q < parts; ++q) {
      const int y0 = GPC_R + (int)((long)(H - 2 * GPC_R) * q / parts), y1 = GPC_R + (int)((long)(H - 2 * GPC_R) * (q + 1) / parts);
      if (first < ncopy && y1 > y0) {
        if (par) c->pool.push(ExpandJob{words, rows, H, y0, y1, (int)first, ncopy, static_cast<gpc_support*>(out), 6});
        else expand_rows(words, rows, y0, y1, first, ncopy, static_cast<gpc_support*>(out));
      }
      for (int y = y0; y < y1; ++y) first += rows[y];
    }
    if (par) host_copy_wait(c);
  } else if (!c->pend.direct && ncopy > 0) {
    const size_t bytes = c->pend.esz * (size_t)ncopy;
    const bool par = bytes >= 256 * 1024;
    if (par) CHK(ensure_pool(c));
    host_copy(c, out, c->h_xfer.p, bytes, par);
    if (par) host_copy_wait(c);
  }
  return (cnt > cap || cnt > c->pend.cap_dev) ? GPC_E_CAPACITY : GPC_OK;
}

static int match_preprocessed(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL,
                              const int32_t* maskL, int nL, const uint8_t* smoothR, const uint8_t* gradR,
                              const int32_t* maskR, int nR, int W, int H, const gpc_settings* s, int mode,
                              void* out, int cap, int* n_out) {
  if (!n_out || cap < 0 || (cap > 0 && !out)) return GPC_E_INVALID;
  // a page-locked `out` is written by the matcher itself over the link
  const size_t esz = mode == 0 ? sizeof(gpc_support) : sizeof(gpc_correspondence);
  void* dv = (c && cap > 0 && (uint64_t)cap * esz < (1ull << 32)) ? device_view_of_host(out) : nullptr;
  CHK(match_preprocessed_begin(c, smoothL, gradL, maskL, nL, smoothR, gradR, maskR, nR, W, H, s, mode, cap, dv));
  const int st = match_fetch(c, out, cap, n_out, nullptr, nullptr);
  c->pend.active = false;
  return st;
}

int gpc_hip_rectified_match(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL,
                            const int32_t* maskL, int nL, const uint8_t* smoothR, const uint8_t* gradR,
                            const int32_t* maskR, int nR, int W, int H, const gpc_settings* s,
                            gpc_support* out, int cap, int* n_out) {
  return match_preprocessed(c, smoothL, gradL, maskL, nL, smoothR, gradR, maskR, nR, W, H, s, 0, out, cap, n_out);
}

int gpc_hip_stereo_match(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL,
                         const int32_t* maskL, int nL, const uint8_t* smoothR, const uint8_t* gradR,
                         const int32_t* maskR, int nR, int W, int H, const gpc_settings* s,
                         gpc_correspondence* out, int cap, int* n_out) {
  return match_preprocessed(c, smoothL, gradL, maskL, nL, smoothR, gradR, maskR, nR, W, H, s, 1, out, cap, n_out);
}

// the asynchronous forms: every match of two candidate lists has at most min(nL, nR) results
int gpc_hip_rectified_match_begin(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL, const int32_t* maskL, int nL,
                                  const uint8_t* smoothR, const uint8_t* gradR, const int32_t* maskR, int nR, int W, int H,
                                  const gpc_settings* s) {
  return match_preprocessed_begin(c, smoothL, gradL, maskL, nL, smoothR, gradR, maskR, nR, W, H, s, 0, (nL < nR ? nL : nR) + 1, nullptr);
}

int gpc_hip_stereo_match_begin(gpc_hip_ctx* c, const uint8_t* smoothL, const uint8_t* gradL, const int32_t* maskL, int nL,
                               const uint8_t* smoothR, const uint8_t* gradR, const int32_t* maskR, int nR, int W, int H,
                               const gpc_settings* s) {
  return match_preprocessed_begin(c, smoothL, gradL, maskL, nL, smoothR, gradR, maskR, nR, W, H, s, 1, (nL < nR ? nL : nR) + 1, nullptr);
}

int gpc_hip_match_fetch(gpc_hip_ctx* c, void* out, int cap, int* n_out, int* n_cand_l, int* n_cand_r) {
  return match_fetch(c, out, cap, n_out, n_cand_l, n_cand_r);
}

// ------------------------------------------------------------------ batch entry points

int gpc_hip_match_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H,
                               int npairs, const gpc_settings* s, gpc_support* d_out, int cap_per_pair,
                               int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_out || !d_counts || npairs <= 0 || cap_per_pair <= 0) return GPC_E_INVALID;
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  if (c->ngroups > 1) {
    if (c->pipeline > 1 || s->use_hashtable) return GPC_E_UNSUPPORTED;
    CHK(run_preprocess(c, d_rawL, d_rawR, W, H, npairs, 2, s->gradient_threshold, true));
    return run_group_match(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, npairs, s, 0,
                           (const uint8_t*)c->grad.p, d_out, cap_per_pair, d_counts, d_ncand);
  }
  if (c->pipeline > 1 && s->epipolar_mode && !s->use_hashtable) {
    // Two lanes: this call goes to the lane the previous one did not take.  Its inputs are what the context's stream has
    // produced so far (e_in); its k_preprocess starts when the other lane's k_hash is done -- beside that lane's join --
    // and its join is queued behind its own k_hash only: the other lane's join is draining by then and this one's
    // workgroups move in as places fall free.  Nothing is queued on the context's stream: gpc_hip_synchronize (or
    // gpc_hip_pipeline_join for a caller with a stream of its own) orders the results.
    CHK(ensure_lanes(c));
    gpc_hip_ctx::Lane& lane = c->lanes[c->next_lane];
    gpc_hip_ctx::Lane& other = c->lanes[c->next_lane ^ 1];
    c->next_lane ^= 1;
    HIPCHK(c, hipEventRecord(lane.e_in, c->stream));
    HIPCHK(c, hipStreamWaitEvent(lane.s, lane.e_in, 0));
    if (other.used) HIPCHK(c, hipStreamWaitEvent(lane.s, other.e_hash, 0));
    LaneScope in(c, lane);
    lane.used = true;
    CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * npairs));
    CHK(run_preprocess(c, d_rawL, d_rawR, W, H, npairs, 2, s->gradient_threshold, true));
    CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * npairs, false, (uint32_t*)c->codes.p));
    HIPCHK(c, hipEventRecord(lane.e_hash, c->stream));
    CHK(run_match(c, W, H, npairs, s, 0, (const uint8_t*)c->grad.p, d_out, cap_per_pair, d_counts, d_ncand));
    HIPCHK(c, hipEventRecord(lane.e_join, c->stream));
    return GPC_OK;
  }
  if (c->pipeline > 1) CHK(drain_lanes(c));  // (the device-wide matchers run on the context itself)
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * npairs));
  if (c->dbg_wait_pre) HIPCHK(c, hipStreamWaitEvent(c->stream, c->dbg_wait_pre, 0));
  CHK(run_preprocess(c, d_rawL, d_rawR, W, H, npairs, 2, s->gradient_threshold, true));
  if (c->dbg_wait_hash) HIPCHK(c, hipStreamWaitEvent(c->stream, c->dbg_wait_hash, 0));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * npairs, false,
               (uint32_t*)c->codes.p));
  if (c->dbg_rec_hash) HIPCHK(c, hipEventRecord(c->dbg_rec_hash, c->stream));
  CHK(run_match(c, W, H, npairs, s, 0, (const uint8_t*)c->grad.p, d_out, cap_per_pair, d_counts, d_ncand));
  if (c->dbg_rec_join) HIPCHK(c, hipEventRecord(c->dbg_rec_join, c->stream));
  return GPC_OK;
}

// Experiment hook, not part of the C ABI (include/gpc_hip.h does not declare it): see gpc_hip_ctx::dbg_wait_pre.
int gpc_hip_set_pipeline(gpc_hip_ctx* c, int lanes) {
  if (!c || (lanes != 1 && lanes != 2)) return GPC_E_INVALID;
  if (lanes == 2 && c->ngroups > 1) return GPC_E_UNSUPPORTED;
  HIPCHK(c, hipSetDevice(c->device));
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->pipeline = lanes;
  return GPC_OK;
}

int gpc_hip_pipeline_join(gpc_hip_ctx* c) {
  if (!c) return GPC_E_INVALID;
  for (auto& l : c->lanes)
    if (l.s && l.used) HIPCHK(c, hipStreamWaitEvent(c->stream, l.e_join, 0));
  return GPC_OK;
}

int gpc_hip_debug_pipeline_events(gpc_hip_ctx* c, void* wait_before_preprocess, void* wait_before_hash, void* record_after_hash,
                                  void* record_after_join) {
  if (!c) return GPC_E_INVALID;
  c->dbg_wait_pre = (hipEvent_t)wait_before_preprocess;
  c->dbg_wait_hash = (hipEvent_t)wait_before_hash;
  c->dbg_rec_hash = (hipEvent_t)record_after_hash;
  c->dbg_rec_join = (hipEvent_t)record_after_join;
  return GPC_OK;
}

static int batch_streams(gpc_hip_ctx* c) {
  if (c->s_in) return GPC_OK;
  HIPCHK(c, c->s_in.create(hipStreamNonBlocking));
  HIPCHK(c, c->s_out.create(hipStreamNonBlocking));
  HIPCHK(c, c->s_cnt.create(hipStreamNonBlocking));  // the counts: never queued behind bulk copies
  for (int i = 0; i < 4; ++i) {
    HIPCHK(c, c->e_in[i].create(hipEventDisableTiming));
    HIPCHK(c, c->e_comp[i].create(hipEventDisableTiming));
    HIPCHK(c, c->e_cnt[i].create(hipEventDisableTiming));
    HIPCHK(c, c->e_out[i].create(hipEventDisableTiming));
  }
  return GPC_OK;
}

// Host buffers in, supports out.  The batch goes through the device in chunks: while chunk k is matched
// on the context's stream, chunk k+1 is uploaded on a second stream and the supports of chunk k-1 go
// back on a third (PCIe is full duplex), so the call costs about what the longer direction of the link
// costs -- the results' way back -- instead of upload + kernels + download one after the other.
// The only host waits are for a chunk's counts, which say how many supports of each pair to fetch.
static int match_batch_unpacked(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs,
                                const gpc_settings* s, gpc_support* out, int cap, int32_t* counts, int32_t* ncand) {
  if (!c || !rawL || !rawR || !out || !counts || npairs <= 0 || cap <= 0) return GPC_E_INVALID;
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  const int chunk = npairs >= 8 ? (npairs >= 32 ? 8 : npairs / 4) : npairs;  // >= 4 chunks once there are 8 pairs
  const int nch = (npairs + chunk - 1) / chunk;
  CHK(ensure(c, c->raw, 2 * 2 * n * chunk));  // two slots x two sides
  CHK(ensure(c, c->out, sizeof(gpc_support) * (size_t)cap * npairs));
  CHK(ensure(c, c->counts, sizeof(int32_t) * npairs));
  CHK(ensure(c, c->ncand, sizeof(int32_t) * 2 * npairs));
  CHK(batch_streams(c));
  CHK(pinned_counts(c, npairs));  // (a copy straight into the caller's pageable arrays blocks the host, see gpc_hip_match_batch)
  // Pageable arrays never reach hipMemcpy (gpc_hip_ctx::h_xfer): images pass through the page-locked bounce buffer, results
  // through a page-locked landing area (two slots of a chunk each), copied by the worker threads
  const bool bounce = !device_view_of_host(rawL) || !device_view_of_host(rawR);
  const bool land = !device_view_of_host(out);
  if (bounce || land) CHK(ensure_pool(c));
  if (bounce) {
    const size_t need = 2 * 2 * n * (size_t)chunk;
    if (need > c->h_in.cap) {
      HIPCHK(c, hipStreamSynchronize(c->s_in));
      CHK(ensure_pinned(c, c->h_in, need));
    }
  }
  const size_t slot_bytes = sizeof(gpc_support) * (size_t)cap * chunk;
  if (land && 2 * slot_bytes > c->h_stage.cap) {
    c->pool.wait_all();
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    CHK(ensure_pinned(c, c->h_stage, 2 * slot_bytes));
  }
  int32_t* hc = c->h_cnt.p;
  int32_t* hn = c->h_cnt.p + npairs;
  int status = GPC_OK;
  // fetch the supports of chunk k (its counts are on their way: wait for them, then one copy per pair)
  auto collect = [&](int k) -> int {
    const int p0 = k * chunk, pc = (p0 + chunk <= npairs) ? chunk : npairs - p0;
    HIPCHK(c, hipEventSynchronize(c->e_cnt[k & 1]));
    memcpy(counts + p0, hc + p0, sizeof(int32_t) * pc);
    if (ncand) memcpy(ncand + 2 * p0, hn + 2 * p0, sizeof(int32_t) * 2 * pc);
    if (land) c->pool.wait_slot(k & 1);  // the copies of chunk k-2 have left this landing slot
    gpc_support* lslot = land ? reinterpret_cast<gpc_support*>((uint8_t*)c->h_stage.p + (size_t)(k & 1) * slot_bytes) : nullptr;
    for (int p = p0; p < p0 + pc; ++p) {
      const int ncopy = counts[p] < cap ? counts[p] : cap;
      if (counts[p] > cap) status = GPC_E_CAPACITY;
      if (ncopy > 0)
        HIPCHK(c, hipMemcpyAsync(land ? lslot + (size_t)(p - p0) * cap : out + (size_t)p * cap,
                                 (gpc_support*)c->out.p + (size_t)p * cap, sizeof(gpc_support) * (size_t)ncopy,
                                 hipMemcpyDeviceToHost, c->s_out));
    }
    if (land) HIPCHK(c, hipEventRecord(c->e_out[k & 1], c->s_out));
    return GPC_OK;
  };
  // landing slot of chunk k -> the caller's array, by the workers
  auto deliver = [&](int k) -> int {
    if (!land) return GPC_OK;
    const int p0 = k * chunk, pc = (p0 + chunk <= npairs) ? chunk : npairs - p0;
    HIPCHK(c, hipEventSynchronize(c->e_out[k & 1]));
    const gpc_support* lslot = reinterpret_cast<const gpc_support*>((uint8_t*)c->h_stage.p + (size_t)(k & 1) * slot_bytes);
    for (int p = p0; p < p0 + pc; ++p) {
      const int ncopy = counts[p] < cap ? counts[p] : cap;
      const size_t bytes = sizeof(gpc_support) * (size_t)ncopy, step = 256 * 1024;
      for (size_t at = 0; at < bytes; at += step) {
        ExpandJob j = {};
        j.slot = k & 1;
        j.copy_src = reinterpret_cast<const uint8_t*>(lslot + (size_t)(p - p0) * cap) + at;
        j.copy_dst = reinterpret_cast<uint8_t*>(out + (size_t)p * cap) + at;
        j.copy_bytes = at + step <= bytes ? step : bytes - at;
        c->pool.push(j);
      }
    }
    return GPC_OK;
  };
  for (int k = 0; k < nch; ++k) {
    const int slot = k & 1, p0 = k * chunk, pc = (p0 + chunk <= npairs) ? chunk : npairs - p0;
    uint8_t* d_l = (uint8_t*)c->raw.p + (size_t)slot * 2 * n * chunk;
    uint8_t* d_r = d_l + n * chunk;
    if (k >= 2) HIPCHK(c, hipStreamWaitEvent(c->s_in, c->e_comp[slot], 0));  // chunk k-2 has read this slot
    const uint8_t *srcL = rawL + (size_t)p0 * n, *srcR = rawR + (size_t)p0 * n;
    if (bounce) {
      uint8_t* bl = (uint8_t*)c->h_in.p + (size_t)slot * 2 * n * chunk;
      uint8_t* br = bl + n * chunk;
      if (k >= 2) HIPCHK(c, hipEventSynchronize(c->e_in[slot]));  // the upload of chunk k-2 has left this bounce slot
      const size_t bytes = n * pc, step = 256 * 1024;
      for (int side = 0; side < 2; ++side)
        for (size_t at = 0; at < bytes; at += step) {
          ExpandJob j = {};
          j.slot = 7;
          j.copy_src = (side ? srcR : srcL) + at;
          j.copy_dst = (side ? br : bl) + at;
          j.copy_bytes = at + step <= bytes ? step : bytes - at;
          c->pool.push(j);
        }
      c->pool.wait_slot(7);
      srcL = bl;
      srcR = br;
    }
    HIPCHK(c, hipMemcpyAsync(d_l, srcL, n * pc, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipMemcpyAsync(d_r, srcR, n * pc, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipEventRecord(c->e_in[slot], c->s_in));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->e_in[slot], 0));
    CHK(gpc_hip_match_batch_device(c, d_l, d_r, W, H, pc, s, (gpc_support*)c->out.p + (size_t)p0 * cap, cap,
                                   (int32_t*)c->counts.p + p0, (int32_t*)c->ncand.p + 2 * p0));
    HIPCHK(c, hipEventRecord(c->e_comp[slot], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_cnt, c->e_comp[slot], 0));
    HIPCHK(c, hipMemcpyAsync(hc + p0, (int32_t*)c->counts.p + p0, sizeof(int32_t) * pc, hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipMemcpyAsync(hn + 2 * p0, (int32_t*)c->ncand.p + 2 * p0, sizeof(int32_t) * 2 * pc, hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipEventRecord(c->e_cnt[slot], c->s_cnt));
    if (k >= 1) CHK(collect(k - 1));
    if (k >= 2) CHK(deliver(k - 2));
  }
  CHK(collect(nch - 1));
  if (nch >= 2) CHK(deliver(nch - 2));
  CHK(deliver(nch - 1));
  if (land) c->pool.wait_all();
  HIPCHK(c, hipStreamSynchronize(c->s_out));
  HIPCHK(c, hipStreamSynchronize(c->s_cnt));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHK(check_join_err(c));
  return status;
}

// ------------------------------------------------------------------ frame sequences

// nframes frames in HBM -> the correspondences of the nframes - 1 consecutive pairs.  One k_preprocess and one k_hash over
// the frames (sides = 1: image f = frame f); k_seq_stats expands the frames' statistics into the pair layout, which stands
// in for the context's statistics while the matcher runs (pair p reads the code images of frames p and p + 1).
int gpc_hip_match_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                  gpc_correspondence* d_out, int cap_per_pair, int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_frames || !d_out || !d_counts || nframes < 2 || cap_per_pair <= 0) return GPC_E_INVALID;
  CHK(match_usable(c, s, W, H, true));
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));  // (sequences run on the context itself)
  const size_t n = (size_t)W * H;
  const int npairs = nframes - 1;
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * nframes));
  CHK(ensure(c, c->sstats, sizeof(int32_t) * GPC_STAT_STRIDE * 2 * npairs));
  CHK(run_preprocess(c, d_frames, nullptr, W, H, nframes, 1, s->gradient_threshold, true));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, nframes, false, (uint32_t*)c->codes.p));
  const int nthr = 2 * npairs * GPC_STAT_STRIDE;  // (>= nframes)
  hipLaunchKernelGGL(gpc::k_seq_stats, dim3((nthr + 255) / 256), dim3(256), 0, c->stream, (const int32_t*)c->stats.p,
                     (int32_t*)c->sstats.p, d_ncand, nframes);
  HIPCHK(c, hipGetLastError());
  std::swap(c->stats, c->sstats);
  const int st = run_match(c, W, H, npairs, s, 1, (const uint8_t*)c->grad.p, d_out, cap_per_pair, d_counts, nullptr, nullptr,
                           true);
  std::swap(c->stats, c->sstats);
  return st;
}

// Host frames in, correspondences out, in chunks of at most K frames (consecutive chunks share a frame): chunk k + 1 is
// uploaded on the batch pipeline's input stream while chunk k is matched on the context's stream; the counts of a chunk
// come back on the counts stream, and its records are fetched once they are known.
int gpc_hip_match_sequence(gpc_hip_ctx* c, const uint8_t* frames, int W, int H, int nframes, const gpc_settings* s,
                           gpc_correspondence* out, int cap, int32_t* counts, int32_t* ncand) {
  if (!c || !frames || !out || !counts || nframes < 2 || cap <= 0) return GPC_E_INVALID;
  CHK(match_usable(c, s, W, H, true));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H;
  const int npairs = nframes - 1;
  const int K = c->seq_frames > 0 ? c->seq_frames : 16;
  const int step = K - 1;                                   // frames a chunk moves on
  const int nch = (npairs + step - 1) / step;
  const int kf = nframes < K ? nframes : K;                 // frames of the largest chunk
  const size_t slot = pad16(n * kf);
  CHK(batch_streams(c));
  CHK(pinned_counts(c, nframes));                           // counts [npairs] + candidates per frame [nframes]
  CHK(ensure(c, c->raw, 2 * slot));
  CHK(ensure(c, c->out, sizeof(gpc_correspondence) * (size_t)cap * npairs));
  CHK(ensure(c, c->counts, sizeof(int32_t) * npairs));
  CHK(ensure(c, c->ncand, sizeof(int32_t) * nframes));
  const bool bounce = !device_view_of_host(frames);
  uint8_t* h_arena = nullptr;
  if (bounce) {  // pageable frames: two slots of the page-locked arena
    uint8_t* d_arena = nullptr;
    CHK(xfer_reserve(c, 2 * slot, &d_arena));
    h_arena = c->h_xfer.p;
    CHK(ensure_pool(c));
  }
  int32_t* hc = c->h_cnt.p;
  int32_t* hn = c->h_cnt.p + npairs;
  gpc_correspondence* d_out = (gpc_correspondence*)c->out.p;
  auto first = [&](int k) { return k * step; };
  auto frames_of = [&](int k) { return nframes - first(k) < K ? nframes - first(k) : K; };
  auto upload = [&](int k) -> int {
    const int sl = k & 1, f0 = first(k), fc = frames_of(k);
    uint8_t* d_in = (uint8_t*)c->raw.p + (size_t)sl * slot;
    if (k >= 2) HIPCHK(c, hipStreamWaitEvent(c->s_in, c->e_comp[sl], 0));  // chunk k-2 has read this slot
    const uint8_t* src = frames + (size_t)f0 * n;
    if (bounce) {
      uint8_t* b = h_arena + (size_t)sl * slot;
      if (k >= 2) HIPCHK(c, hipEventSynchronize(c->e_in[sl]));  // the upload of chunk k-2 has left this arena slot
      host_copy(c, b, src, n * fc, true);
      host_copy_wait(c);
      src = b;
    }
    HIPCHK(c, hipMemcpyAsync(d_in, src, n * fc, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipEventRecord(c->e_in[sl], c->s_in));
    return GPC_OK;
  };
  int status = GPC_OK;
  auto collect = [&](int k) -> int {
    const int p0 = first(k), pc = frames_of(k) - 1;
    HIPCHK(c, hipEventSynchronize(c->e_cnt[k & 1]));
    memcpy(counts + p0, hc + p0, sizeof(int32_t) * pc);
    for (int p = p0; p < p0 + pc; ++p) {
      const int ncopy = counts[p] < cap ? counts[p] : cap;
      if (counts[p] > cap) status = GPC_E_CAPACITY;
      if (ncopy > 0)
        HIPCHK(c, hipMemcpyAsync(out + (size_t)p * cap, d_out + (size_t)p * cap, sizeof(gpc_correspondence) * (size_t)ncopy,
                                 hipMemcpyDeviceToHost, c->s_out));
    }
    return GPC_OK;
  };
  CHK(upload(0));
  for (int k = 0; k < nch; ++k) {
    const int sl = k & 1, f0 = first(k), fc = frames_of(k);
    if (k + 1 < nch) CHK(upload(k + 1));  // (queued before this chunk's matcher: the device-wide ones wait on the host)
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->e_in[sl], 0));
    CHK(gpc_hip_match_sequence_device(c, (const uint8_t*)c->raw.p + (size_t)sl * slot, W, H, fc, s, d_out + (size_t)f0 * cap,
                                      cap, (int32_t*)c->counts.p + f0, (int32_t*)c->ncand.p + f0));
    HIPCHK(c, hipEventRecord(c->e_comp[sl], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_cnt, c->e_comp[sl], 0));
    HIPCHK(c, hipMemcpyAsync(hc + f0, (int32_t*)c->counts.p + f0, sizeof(int32_t) * (fc - 1), hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipMemcpyAsync(hn + f0, (int32_t*)c->ncand.p + f0, sizeof(int32_t) * fc, hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipEventRecord(c->e_cnt[sl], c->s_cnt));
    if (k >= 1) CHK(collect(k - 1));
  }
  CHK(collect(nch - 1));
  HIPCHK(c, hipStreamSynchronize(c->s_out));
  HIPCHK(c, hipStreamSynchronize(c->s_cnt));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (ncand) memcpy(ncand, hn, sizeof(int32_t) * nframes);
  return status;
}

}  // extern "C"

// (a part of this translation unit: see the note below the includes at the top)
#include "host_staging.h"

extern "C" {

// ------------------------------------------------------------------ scoring against ground truth

static_assert(sizeof(gpc_score) == sizeof(gpc::ScoreDev), "gpc_score and the kernels' view of it");
static_assert(GPC_SCORE_MAX_THR == SC_MAX_THR, "threshold slots");

// fl(thr * thr) per threshold, -1 beyond n_thr; GPC_E_INVALID for a count outside 1 .. 8 or a threshold that is negative or not finite
static int score_thresholds(const float* thr, int n_thr, gpc::ScoreThr& t) {
  if (!thr || n_thr < 1 || n_thr > GPC_SCORE_MAX_THR) return GPC_E_INVALID;
  for (int k = 0; k < GPC_SCORE_MAX_THR; ++k) {
    if (k >= n_thr) {
      t.t2[k] = -1.f;
      continue;
    }
    const volatile float v = thr[k];
    if (!(v >= 0.f) || !(v <= 3.402823466e38f)) return GPC_E_INVALID;
    const volatile float sq = v * v;  // (one float32 rounding, whatever the host compiler's excess precision)
    t.t2[k] = sq;
  }
  return GPC_OK;
}

static int truth_ok(const gpc_truth* truth, bool corr) {
  if (!truth || !truth->u) return GPC_E_INVALID;
  if (corr ? !truth->v : truth->v != nullptr) return GPC_E_INVALID;
  return GPC_OK;
}

// k_score_matchable reads four pixels of a truth plane with one 16-byte load and four ignore bytes with one 4-byte load
static int truth_aligned(const gpc_truth* truth) {
  if (((uintptr_t)truth->u & 15u) || ((uintptr_t)truth->v & 15u) || ((uintptr_t)truth->ignore & 3u)) return GPC_E_INVALID;
  return GPC_OK;
}

// d_scores is cleared on the stream, then the records kernel runs over d_rec[npairs][cap]
static int score_records(gpc_hip_ctx* c, const void* d_rec, bool corr, long cap, const int32_t* d_counts, int W, int H,
                         int npairs, const gpc_truth* truth, const gpc::ScoreThr& t, gpc_score* d_scores) {
  HIPCHK(c, hipMemsetAsync(d_scores, 0, sizeof(gpc_score) * (size_t)npairs, c->stream));
  const long nchunk = (cap + SC_CHUNK - 1) / SC_CHUNK;
  const dim3 grid((unsigned)(nchunk < 1024 ? nchunk : 1024), npairs);
  Timed tm(c, KID_SCORE_RECORDS);
  snprintf(c->launch_name[KID_SCORE_RECORDS], sizeof c->launch_name[0], "gpc::k_score_records<%s>", corr ? "true" : "false");
  if (corr)
    hipLaunchKernelGGL((gpc::k_score_records<true>), grid, dim3(SC_THREADS), 0, c->stream, (const gpc::ScRec<true>*)d_rec, cap,
                       d_counts, W, H, truth->u, truth->v, truth->ignore, t, (gpc::ScoreDev*)d_scores);
  else
    hipLaunchKernelGGL((gpc::k_score_records<false>), grid, dim3(SC_THREADS), 0, c->stream, (const gpc::ScRec<false>*)d_rec, cap,
                       d_counts, W, H, truth->u, (const float*)nullptr, truth->ignore, t, (gpc::ScoreDev*)d_scores);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// n_candidates / n_matchable from the gradient images the pipeline just left in c->grad (bit or byte form)
static int score_matchable(gpc_hip_ctx* c, bool flow, int lstride, int W, int H, int npairs, const gpc_truth* truth,
                           gpc_score* d_scores) {
  const long groups = (long)(H - 2 * GPC_R) * W / SC_PX;
  const long nblk = (groups + SC_THREADS - 1) / SC_THREADS;
  const dim3 grid((unsigned)(nblk < 256 ? nblk : 256), npairs);
  const GpcDivW dw = make_divw(W);
  const bool bits = c->grad_is_bits;
  Timed tm(c, KID_SCORE_MATCHABLE);
  snprintf(c->launch_name[KID_SCORE_MATCHABLE], sizeof c->launch_name[0], "gpc::k_score_matchable<%s, %s>", flow ? "true" : "false",
           bits ? "true" : "false");
#define LAUNCH_MATCHABLE(FLOW, BITS)                                                                                          \
  hipLaunchKernelGGL((gpc::k_score_matchable<FLOW, BITS>), grid, dim3(SC_THREADS), 0, c->stream, (const uint8_t*)c->grad.p, \
                     lstride, W, H, dw, truth->u, truth->v, truth->ignore, (gpc::ScoreDev*)d_scores)
  if (flow) {
    if (bits) LAUNCH_MATCHABLE(true, true); else LAUNCH_MATCHABLE(true, false);
  } else {
    if (bits) LAUNCH_MATCHABLE(false, true); else LAUNCH_MATCHABLE(false, false);
  }
#undef LAUNCH_MATCHABLE
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

static int score_records_entry(gpc_hip_ctx* c, const void* d_rec, bool corr, int cap, const int32_t* d_counts, int W, int H,
                               int npairs, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* d_scores) {
  if (!c || !d_rec || !d_counts || !d_scores || npairs <= 0 || cap <= 0 || W <= 0 || H <= 0) return GPC_E_INVALID;
  if ((long)W * H > (1l << 30)) return GPC_E_UNSUPPORTED;
  CHK(truth_ok(truth, corr));
  gpc::ScoreThr t;
  CHK(score_thresholds(thr, n_thr, t));
  HIPCHK(c, hipSetDevice(c->device));
  return score_records(c, d_rec, corr, cap, d_counts, W, H, npairs, truth, t, d_scores);
}

int gpc_hip_score_supports_device(gpc_hip_ctx* c, const gpc_support* d_supports, int cap_per_pair, const int32_t* d_counts, int W,
                                  int H, int npairs, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* d_scores) {
  return score_records_entry(c, d_supports, false, cap_per_pair, d_counts, W, H, npairs, truth, thr, n_thr, d_scores);
}

int gpc_hip_score_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* d_corr, int cap_per_pair,
                                         const int32_t* d_counts, int W, int H, int npairs, const gpc_truth* truth,
                                         const float* thr, int n_thr, gpc_score* d_scores) {
  return score_records_entry(c, d_corr, true, cap_per_pair, d_counts, W, H, npairs, truth, thr, n_thr, d_scores);
}

// match and score, images as all_records takes them: disparities of pairs, flow of frames
static int score_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s,
                       const gpc_truth* truth, const float* thr, int n_thr, gpc_score* d_scores) {
  const bool flow = !d_b;
  CHK(truth_ok(truth, flow));
  CHK(truth_aligned(truth));
  gpc::ScoreThr t;
  CHK(score_thresholds(thr, n_thr, t));
  AllRecords r;
  CHK(all_records_cap(c, s, W, H, flow, &r.cap));
  CHK(all_records(c, d_a, d_b, W, H, npairs, s, nullptr, &r));
  CHK(score_records(c, r.rec, flow, r.cap, r.counts, W, H, npairs, truth, t, d_scores));
  return score_matchable(c, flow, flow ? 1 : 2, W, H, npairs, truth, d_scores);
}

int gpc_hip_score_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                               const gpc_settings* s, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* d_scores) {
  if (!c || !d_rawL || !d_rawR || !d_scores || npairs <= 0) return GPC_E_INVALID;
  return score_match(c, d_rawL, d_rawR, W, H, npairs, s, truth, thr, n_thr, d_scores);
}

int gpc_hip_score_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                  const gpc_truth* truth, const float* thr, int n_thr, gpc_score* d_scores) {
  if (!c || !d_frames || !d_scores || nframes < 2) return GPC_E_INVALID;
  return score_match(c, d_frames, nullptr, W, H, nframes - 1, s, truth, thr, n_thr, d_scores);
}

// a chunk's scores -> the caller's array (120 bytes per pair: through h_cnt), then the chunk is done
static int score_down(Stage& st, size_t region, gpc_score* scores, int n) {
  CHK(st.down(st.c->h_cnt.p, region, sizeof(gpc_score) * (size_t)n));
  CHK(st.wait());
  memcpy(scores, st.c->h_cnt.p, sizeof(gpc_score) * (size_t)n);
  return check_join_err(st.c);
}

// records, counts and truth of at most 16 pairs at a time through the records form
static int score_records_host(gpc_hip_ctx* c, const void* rec, bool corr, int cap, const int32_t* counts, int W, int H, int npairs,
                              const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  if (!c || !rec || !counts || !scores || npairs <= 0 || cap <= 0 || W <= 0 || H <= 0) return GPC_E_INVALID;
  if ((long)W * H > (1l << 30)) return GPC_E_UNSUPPORTED;
  CHK(truth_ok(truth, corr));
  gpc::ScoreThr t;
  CHK(score_thresholds(thr, n_thr, t));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H, esz = corr ? sizeof(gpc_correspondence) : sizeof(gpc_support);
  const int K = npairs < 16 ? npairs : 16;
  Stage st(c);
  const size_t r_rec = st.in(esz * (size_t)cap * K), r_cnt = st.in(sizeof(int32_t) * (size_t)K), r_u = st.in(sizeof(float) * n * K);
  const size_t r_v = st.in(corr ? sizeof(float) * n * K : 0), r_ign = st.in(truth->ignore ? n * K : 0);
  const size_t r_sc = st.out(sizeof(gpc_score) * (size_t)K);
  CHK(st.alloc(sizeof(gpc_score) * (size_t)K));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    // (whole, not by up_records: beside the truth planes the records are the lesser part, and per pair they went up no faster)
    CHK(st.up(r_rec, (const uint8_t*)rec + esz * (size_t)cap * p0, esz * (size_t)cap * pc));
    CHK(st.up(r_cnt, counts + p0, sizeof(int32_t) * (size_t)pc));
    CHK(st.up(r_u, truth->u + n * p0, sizeof(float) * n * pc));
    if (corr) CHK(st.up(r_v, truth->v + n * p0, sizeof(float) * n * pc));
    if (truth->ignore) CHK(st.up(r_ign, truth->ignore + n * p0, n * pc));
    const gpc_truth dt = {(const float*)st.p(r_u), corr ? (const float*)st.p(r_v) : nullptr, truth->ignore ? st.p(r_ign) : nullptr};
    CHK(score_records(c, st.p(r_rec), corr, cap, (const int32_t*)st.p(r_cnt), W, H, pc, &dt, t, (gpc_score*)st.p(r_sc)));
    CHK(score_down(st, r_sc, scores + p0, pc));
  }
  return GPC_OK;
}

int gpc_hip_score_supports(gpc_hip_ctx* c, const gpc_support* supports, int cap_per_pair, const int32_t* counts, int W, int H,
                           int npairs, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  return score_records_host(c, supports, false, cap_per_pair, counts, W, H, npairs, truth, thr, n_thr, scores);
}

int gpc_hip_score_correspondences(gpc_hip_ctx* c, const gpc_correspondence* corr, int cap_per_pair, const int32_t* counts, int W,
                                  int H, int npairs, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  return score_records_host(c, corr, true, cap_per_pair, counts, W, H, npairs, truth, thr, n_thr, scores);
}

// images and truth of a chunk of pairs through score_match; b null: a holds npairs + 1 frames, and chunks share a frame
static int score_match_host(gpc_hip_ctx* c, const uint8_t* a, const uint8_t* b, int W, int H, int npairs, const gpc_settings* s,
                            const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  const bool seq = !b;
  CHK(truth_ok(truth, seq));
  gpc::ScoreThr t;
  CHK(score_thresholds(thr, n_thr, t));
  CHK(match_usable(c, s, W, H, seq));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H;
  // pairs per chunk: 16, or the pairs of 16 frames (GPC_HIP_SEQ_FRAMES: tests)
  const int most = seq ? (c->seq_frames > 1 && c->seq_frames < 16 ? c->seq_frames : 16) - 1 : 16;
  const int K = npairs < most ? npairs : most;
  Stage st(c);
  const size_t r_a = st.in(n * (K + seq)), r_b = st.in(seq ? 0 : n * K), r_u = st.in(sizeof(float) * n * K);
  const size_t r_v = st.in(seq ? sizeof(float) * n * K : 0), r_ign = st.in(truth->ignore ? n * K : 0);
  const size_t r_sc = st.out(sizeof(gpc_score) * (size_t)K);
  CHK(st.alloc(sizeof(gpc_score) * (size_t)K));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_a, a + n * p0, n * (pc + seq)));
    if (!seq) CHK(st.up(r_b, b + n * p0, n * pc));
    CHK(st.up(r_u, truth->u + n * p0, sizeof(float) * n * pc));
    if (seq) CHK(st.up(r_v, truth->v + n * p0, sizeof(float) * n * pc));
    if (truth->ignore) CHK(st.up(r_ign, truth->ignore + n * p0, n * pc));
    const gpc_truth dt = {(const float*)st.p(r_u), seq ? (const float*)st.p(r_v) : nullptr, truth->ignore ? st.p(r_ign) : nullptr};
    CHK(score_match(c, st.p(r_a), seq ? nullptr : st.p(r_b), W, H, pc, s, &dt, thr, n_thr, (gpc_score*)st.p(r_sc)));
    CHK(score_down(st, r_sc, scores + p0, pc));
  }
  return GPC_OK;
}

int gpc_hip_score_batch(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs, const gpc_settings* s,
                        const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  if (!c || !rawL || !rawR || !scores || npairs <= 0) return GPC_E_INVALID;
  return score_match_host(c, rawL, rawR, W, H, npairs, s, truth, thr, n_thr, scores);
}

int gpc_hip_score_sequence(gpc_hip_ctx* c, const uint8_t* frames, int W, int H, int nframes, const gpc_settings* s,
                           const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores) {
  if (!c || !frames || !scores || nframes < 2) return GPC_E_INVALID;
  return score_match_host(c, frames, nullptr, W, H, nframes - 1, s, truth, thr, n_thr, scores);
}

// ------------------------------------------------------------------ point tracks over a frame sequence

static_assert(sizeof(gpc_track) == sizeof(gpc::TrRow) && sizeof(gpc_track) == 16, "gpc_track and the kernels' view of it");
static_assert(sizeof(gpc_correspondence) == sizeof(gpc::TrRec), "gpc_correspondence and the kernels' view of it");

static int track_args(const gpc_hip_ctx* c, const void* corr, int cap, const void* counts, int W, int H, int npairs,
                      const void* next, const void* track_id, const void* tracks, int track_cap, const void* ntracks) {
  if (!c || !corr || !counts || !next || !track_id || !ntracks || npairs < 1 || cap <= 0 || track_cap < 0 || W <= 0 || H <= 0)
    return GPC_E_INVALID;
  if (track_cap > 0 && !tracks) return GPC_E_INVALID;
  // a pixel index takes 30 bits, a record's number in the whole sequence (the largest track id) 31
  // (and a launch has one grid row per pair); the kernels step a record index in int by up to a grid's width past cap
  if ((long)W * H > (1l << 30) || (long)npairs * cap > 0x7FFFFFFFl || cap > (1 << 30) || npairs > 65535) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// The six launches over records already on the device.  The planes are FILLED first (4 bytes per pixel and pair, 16-byte
// stores): the lowest index of duplicate sources is an integer minimum, and a minimum over whatever an earlier call left
// in the plane could keep a stale lower index that a later check can only reject, not replace.
static int track_link(gpc_hip_ctx* c, const gpc_correspondence* d_corr, int cap, const int32_t* d_counts, int W, int H, int P,
                      int32_t* d_next, int32_t* d_track_id, gpc_track* d_tracks, int track_cap, int32_t* d_ntracks) {
  const size_t n = (size_t)W * H;
  const long nchunk = ((long)cap + TR_CHUNK - 1) / TR_CHUNK;
  const long n16 = (long)((n * (size_t)(P - 1) + 3) / 4);  // (the last group may reach into the slack ensure() leaves)
  CHK(ensure(c, c->tr_plane, sizeof(int32_t) * n * (size_t)(P - 1)));
  CHK(ensure(c, c->tr_pred, sizeof(int32_t) * (size_t)cap * P));
  CHK(ensure(c, c->tr_blk, sizeof(int32_t) * (size_t)nchunk * P));
  const gpc::TrRec* rec = (const gpc::TrRec*)d_corr;
  int32_t* plane = (int32_t*)c->tr_plane.p;
  int32_t* pred = (int32_t*)c->tr_pred.p;
  int32_t* blk = (int32_t*)c->tr_blk.p;
  const dim3 sgrid((unsigned)(nchunk < 1024 ? nchunk : 1024), P), cgrid((unsigned)nchunk, P);
  if (n16 > 0) {
    const long fb = (n16 + TR_THREADS - 1) / TR_THREADS;
    Timed t(c, KID_TRACK_FILL);
    hipLaunchKernelGGL(gpc::k_track_fill, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(TR_THREADS), 0, c->stream, (int4*)plane, n16);
  }
  {
    Timed t(c, KID_TRACK_SCATTER);
    hipLaunchKernelGGL(gpc::k_track_scatter, sgrid, dim3(TR_THREADS), 0, c->stream, rec, cap, d_counts, W, H, plane, pred);
  }
  {
    Timed t(c, KID_TRACK_LINK);
    hipLaunchKernelGGL(gpc::k_track_link, sgrid, dim3(TR_THREADS), 0, c->stream, rec, cap, d_counts, W, H, P,
                       (const int32_t*)plane, pred, d_next);
  }
  {
    Timed t(c, KID_TRACK_SETTLE);
    hipLaunchKernelGGL(gpc::k_track_settle, cgrid, dim3(TR_THREADS), 0, c->stream, cap, d_counts, P, (const int32_t*)pred, d_next,
                       blk, (int)nchunk);
  }
  {
    Timed t(c, KID_TRACK_SCAN);
    hipLaunchKernelGGL(gpc::k_track_scan, dim3(1), dim3(1024), 0, c->stream, blk, nchunk * P, d_ntracks);
  }
  {
    Timed t(c, KID_TRACK_WALK);
    hipLaunchKernelGGL(gpc::k_track_walk, cgrid, dim3(TR_THREADS), 0, c->stream, cap, d_counts, P, (const int32_t*)pred,
                       (const int32_t*)d_next, (const int32_t*)blk, (int)nchunk, d_track_id, (gpc::TrRow*)d_tracks, track_cap);
  }
  for (int k = KID_TRACK_FILL; k <= KID_TRACK_WALK; ++k) snprintf(c->launch_name[k], sizeof c->launch_name[0], "gpc::%s", kKernelNames[k]);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int gpc_hip_track_records_device(gpc_hip_ctx* c, const gpc_correspondence* d_corr, int cap_per_pair, const int32_t* d_counts, int W,
                                 int H, int npairs, int32_t* d_next, int32_t* d_track_id, gpc_track* d_tracks, int track_cap,
                                 int32_t* d_ntracks) {
  CHK(track_args(c, d_corr, cap_per_pair, d_counts, W, H, npairs, d_next, d_track_id, d_tracks, track_cap, d_ntracks));
  HIPCHK(c, hipSetDevice(c->device));
  return track_link(c, d_corr, cap_per_pair, d_counts, W, H, npairs, d_next, d_track_id, d_tracks, track_cap, d_ntracks);
}

int gpc_hip_track_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                  gpc_correspondence* d_corr, int cap_per_pair, int32_t* d_counts, int32_t* d_ncand,
                                  int32_t* d_next, int32_t* d_track_id, gpc_track* d_tracks, int track_cap, int32_t* d_ntracks) {
  if (!c || !d_frames || nframes < 2) return GPC_E_INVALID;
  CHK(track_args(c, d_corr, cap_per_pair, d_counts, W, H, nframes - 1, d_next, d_track_id, d_tracks, track_cap, d_ntracks));
  CHK(gpc_hip_match_sequence_device(c, d_frames, W, H, nframes, s, d_corr, cap_per_pair, d_counts, d_ncand));
  return track_link(c, d_corr, cap_per_pair, d_counts, W, H, nframes - 1, d_next, d_track_id, d_tracks, track_cap, d_ntracks);
}

// Host forms (Stage): the whole call in one block, the device form once over it.
namespace {
struct TrackRegions {
  size_t in, corr, cnt, nc, next, id, tab, nt;
};
}  // namespace

// frame_bytes: the frames of the sequence form, whose records and counts come down; 0: the records form, where they go up
static int track_layout(Stage& st, size_t frame_bytes, int P, int cap, int track_cap, TrackRegions* r) {
  const size_t rec = (size_t)P * cap;
  r->in = st.in(frame_bytes);
  r->corr = frame_bytes ? st.out(sizeof(gpc_correspondence) * rec) : st.in(sizeof(gpc_correspondence) * rec);
  r->cnt = frame_bytes ? st.out(sizeof(int32_t) * (size_t)P) : st.in(sizeof(int32_t) * (size_t)P);
  r->nc = st.out(sizeof(int32_t) * (size_t)(P + 1)), r->next = st.out(sizeof(int32_t) * rec), r->id = st.out(sizeof(int32_t) * rec);
  r->tab = st.out(sizeof(gpc_track) * (size_t)track_cap), r->nt = st.out(sizeof(int32_t));
  return st.alloc(sizeof(int32_t) * (2 * (size_t)P + 2));  // counts [P], candidates [P + 1], the number of tracks
}

// counts (and candidate counts) first, then what they say is valid: m_t records, links and ids per pair, min(n, track_cap)
// rows.  corr, counts, ncand: null where the form does not hand them back
static int track_down(Stage& st, const TrackRegions& r, int P, int cap, int track_cap, gpc_correspondence* corr, int32_t* counts,
                      int32_t* ncand, int32_t* next, int32_t* track_id, gpc_track* tracks, int32_t* ntracks) {
  int32_t* hc = st.c->h_cnt.p;
  CHK(st.down(hc, r.cnt, sizeof(int32_t) * (size_t)P));
  if (ncand) CHK(st.down(hc + P, r.nc, sizeof(int32_t) * (size_t)(P + 1)));
  CHK(st.down(hc + 2 * P + 1, r.nt, sizeof(int32_t)));
  CHK(st.wait());
  int status = GPC_OK;
  for (int t = 0; t < P; ++t) {
    const size_t m = (size_t)valid_records(hc[t], cap), at = (size_t)t * cap;
    if (hc[t] > cap) status = GPC_E_CAPACITY;
    if (!m) continue;
    if (corr) CHK(st.down(corr + at, r.corr + sizeof(gpc_correspondence) * at, sizeof(gpc_correspondence) * m));
    CHK(st.down(next + at, r.next + sizeof(int32_t) * at, sizeof(int32_t) * m));
    CHK(st.down(track_id + at, r.id + sizeof(int32_t) * at, sizeof(int32_t) * m));
  }
  const int nt = hc[2 * P + 1];
  if (nt > track_cap) status = GPC_E_CAPACITY;
  if (nt > 0 && track_cap > 0) CHK(st.down(tracks, r.tab, sizeof(gpc_track) * (size_t)(nt < track_cap ? nt : track_cap)));
  CHK(st.wait());
  if (counts) memcpy(counts, hc, sizeof(int32_t) * (size_t)P);
  if (ncand) memcpy(ncand, hc + P, sizeof(int32_t) * (size_t)(P + 1));
  *ntracks = nt;
  CHK(check_join_err(st.c));
  return status;
}

int gpc_hip_track_records(gpc_hip_ctx* c, const gpc_correspondence* corr, int cap, const int32_t* counts, int W, int H, int npairs,
                          int32_t* next, int32_t* track_id, gpc_track* tracks, int track_cap, int32_t* ntracks) {
  CHK(track_args(c, corr, cap, counts, W, H, npairs, next, track_id, tracks, track_cap, ntracks));
  CHK(host_call_begin(c));
  Stage st(c);
  TrackRegions r;
  CHK(track_layout(st, 0, npairs, cap, track_cap, &r));
  CHK(st.up(r.cnt, counts, sizeof(int32_t) * (size_t)npairs));
  CHK(st.up_records(r.corr, corr, sizeof(gpc_correspondence), cap, counts, 0, npairs));
  CHK(track_link(c, (const gpc_correspondence*)st.p(r.corr), cap, (const int32_t*)st.p(r.cnt), W, H, npairs, (int32_t*)st.p(r.next),
                 (int32_t*)st.p(r.id), (gpc_track*)st.p(r.tab), track_cap, (int32_t*)st.p(r.nt)));
  return track_down(st, r, npairs, cap, track_cap, nullptr, nullptr, nullptr, next, track_id, tracks, ntracks);
}

int gpc_hip_track_sequence(gpc_hip_ctx* c, const uint8_t* frames, int W, int H, int nframes, const gpc_settings* s,
                           gpc_correspondence* corr, int cap, int32_t* counts, int32_t* ncand, int32_t* next, int32_t* track_id,
                           gpc_track* tracks, int track_cap, int32_t* ntracks) {
  if (!c || !frames || nframes < 2) return GPC_E_INVALID;
  const int npairs = nframes - 1;
  CHK(track_args(c, corr, cap, counts, W, H, npairs, next, track_id, tracks, track_cap, ntracks));
  CHK(match_usable(c, s, W, H, true));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H;
  Stage st(c);
  TrackRegions r;
  CHK(track_layout(st, n * nframes, npairs, cap, track_cap, &r));
  CHK(st.up(r.in, frames, n * nframes));
  CHK(gpc_hip_track_sequence_device(c, st.p(r.in), W, H, nframes, s, (gpc_correspondence*)st.p(r.corr), cap, (int32_t*)st.p(r.cnt),
                                    (int32_t*)st.p(r.nc), (int32_t*)st.p(r.next), (int32_t*)st.p(r.id), (gpc_track*)st.p(r.tab),
                                    track_cap, (int32_t*)st.p(r.nt)));
  return track_down(st, r, npairs, cap, track_cap, corr, counts, ncand, next, track_id, tracks, ntracks);
}

// ------------------------------------------------------------------ track streams: tracks kept alive across pushes

// What a stream carries from one push to the next, all of it the stream's own device memory (include/gpc_hip.h has the
// byte formula): the last frame's code image, statistics words and (WIDE joins) candidate bytes; the last pair's records,
// count and track ids; the track table and the running total.  The window's `next` is workspace of the stream; planes,
// predecessors and head counts are the context's (tr_plane, tr_pred, tr_blk), as for the offline calls.
struct gpc_hip_track_stream {
  gpc::TrsBook book;
  gpc_settings settings;
  bool have_settings = false;
  DevBlock<uint32_t> codes;       // [H][W], allocated by the first push of frames
  DevBlock<uint8_t> cand;         // [H][W], allocated by the first push of frames under 32-bit Naive codes
  DevBlock<int32_t> fstats;       // GPC_STAT_STRIDE words
  DevBlock<gpc::TrRec> crec;      // [cap]
  DevBlock<int32_t> cid;          // [cap]
  DevBlock<int32_t> words;        // [0] the carried pair's count (clamped), [1] the number of tracks
  DevBlock<gpc_track> table;      // [max(track_cap, 1)]
  DevBuf nextw;                   // [c + k][cap] of the largest push so far
};

namespace {

int trs_check(gpc_hip_ctx* c, gpc_hip_track_stream* s) {
  if (!c || !s) return GPC_E_INVALID;
  for (gpc_hip_track_stream* t : c->track_streams)   // (a destroyed stream, or another context's, is not in the list)
    if (t == s) return GPC_OK;
  return GPC_E_INVALID;
}

// The link steps over the window [carried pair, k new pairs] whose new records are on the device, then the carry of the
// next push.  Only queues work on the context's stream.
int trs_link(gpc_hip_ctx* c, gpc_hip_track_stream* s, const gpc_correspondence* d_corr, const int32_t* d_counts,
             const gpc::TrsPush& p, int32_t* d_prev, int32_t* d_track_id) {
  const int W = s->book.W, H = s->book.H, cap = s->book.cap, k = p.k, cy = p.carry;
  const size_t n = (size_t)W * H;
  const long nchunk = ((long)cap + TR_CHUNK - 1) / TR_CHUNK;
  const long n16 = (long)((n * (size_t)k + 3) / 4);  // (the last group may reach into the slack ensure() leaves)
  CHK(ensure(c, c->tr_plane, sizeof(int32_t) * n * (size_t)k));
  CHK(ensure(c, c->tr_pred, sizeof(int32_t) * (size_t)cap * k));
  CHK(ensure(c, c->tr_blk, sizeof(int32_t) * (size_t)nchunk * k));
  CHK(ensure(c, s->nextw, sizeof(int32_t) * (size_t)cap * (size_t)(cy + k)));
  const gpc::TrRec* rec = (const gpc::TrRec*)d_corr;
  int32_t* plane = (int32_t*)c->tr_plane.p;
  int32_t* pred = (int32_t*)c->tr_pred.p;
  int32_t* blk = (int32_t*)c->tr_blk.p;
  int32_t* next = (int32_t*)s->nextw.p;
  const int32_t* cm = s->words.p;
  int32_t* total = s->words.p + 1;
  const unsigned gx = (unsigned)(nchunk < 1024 ? nchunk : 1024);
  const dim3 sgrid(gx, k), wgrid(gx, cy + k), cgrid((unsigned)nchunk, cy + k);
  {
    const long fb = (n16 + TR_THREADS - 1) / TR_THREADS;
    Timed t(c, KID_TRS_FILL);
    hipLaunchKernelGGL(gpc::k_trs_fill, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(TR_THREADS), 0, c->stream, (int4*)plane, n16);
  }
  {
    Timed t(c, KID_TRS_SCATTER);
    hipLaunchKernelGGL(gpc::k_trs_scatter, sgrid, dim3(TR_THREADS), 0, c->stream, rec, cap, d_counts, W, H, plane, pred);
  }
  {
    Timed t(c, KID_TRS_LINK);
    hipLaunchKernelGGL(gpc::k_trs_link, wgrid, dim3(TR_THREADS), 0, c->stream, (const gpc::TrRec*)s->crec.p, cm, cy, rec, cap, d_counts,
                       W, H, k, (const int32_t*)plane, pred, next);
  }
  {
    Timed t(c, KID_TRS_SETTLE);
    hipLaunchKernelGGL(gpc::k_trs_settle, cgrid, dim3(TR_THREADS), 0, c->stream, cm, cy, cap, d_counts, k, (const int32_t*)pred, next,
                       blk, (int)nchunk);
  }
  {
    Timed t(c, KID_TRS_SCAN);
    hipLaunchKernelGGL(gpc::k_trs_scan, dim3(1), dim3(1024), 0, c->stream, blk, nchunk * k, total);
  }
  {
    Timed t(c, KID_TRS_WALK);
    hipLaunchKernelGGL(gpc::k_trs_walk, cgrid, dim3(TR_THREADS), 0, c->stream, cm, (const int32_t*)s->cid.p, cy, cap, d_counts, k,
                       (const int32_t*)pred, (const int32_t*)next, (const int32_t*)blk, (int)nchunk, s->book.pairs_seen, d_track_id,
                       d_prev, (gpc::TrRow*)s->table.p, s->book.track_cap);
  }
  {
    Timed t(c, KID_TRS_SAVE);
    hipLaunchKernelGGL(gpc::k_trs_save, dim3(gx), dim3(TR_THREADS), 0, c->stream, rec + (size_t)(k - 1) * cap,
                       (const int32_t*)d_track_id + (size_t)(k - 1) * cap, d_counts + (k - 1), cap, s->crec.p, s->cid.p, s->words.p);
  }
  for (int q = KID_TRS_FILL; q <= KID_TRS_SAVE; ++q) snprintf(c->launch_name[q], sizeof c->launch_name[0], "gpc::%s", kKernelNames[q]);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// every refusal of a push of frames that leaves the stream as it is; on GPC_OK *p says what the push produces
int trs_frames_usable(gpc_hip_ctx* c, gpc_hip_track_stream* s, int nframes, gpc::TrsPush* p) {
  CHK(trs_check(c, s));
  if (!s->have_settings) return GPC_E_INVALID;
  CHK(match_usable(c, &s->settings, s->book.W, s->book.H, true));
  return gpc::trs_plan(s->book, gpc::TRS_FRAMES, nframes, c->code_gen, p);
}

// gpc_hip_match_sequence_device with frame 0 of the layout supplied by the carry instead of computed: the new frames are
// images off .. off + nframes - 1 of the codes [nimg][H][W] and of the statistics, k_preprocess and k_hash run over them
// alone and write their statistics words behind slot 0.  Where the joins read candidate bytes (wide_codes) the gradient
// image takes the same layout; otherwise it is the context's as for any sequence (the bit image where that is taken).
int trs_push_frames(gpc_hip_ctx* c, gpc_hip_track_stream* s, const uint8_t* d_frames, int nframes, gpc_correspondence* d_corr,
                    int32_t* d_counts, int32_t* d_ncand, int32_t* d_prev, int32_t* d_track_id, const gpc::TrsPush& p) {
  const int W = s->book.W, H = s->book.H, cap = s->book.cap;
  const size_t n = (size_t)W * H;
  const int off = s->book.frames_seen > 0 ? 1 : 0, nimg = nframes + off, npairs = nimg - 1;
  const bool wide = wide_codes(c);
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));  // (streams run on the context itself, as sequences do)
  if (!s->codes.p) HIPCHK(c, s->codes.alloc(sizeof(uint32_t) * n));
  if (!s->fstats.p) HIPCHK(c, s->fstats.alloc(sizeof(int32_t) * GPC_STAT_STRIDE));
  if (wide && !s->cand.p) HIPCHK(c, s->cand.alloc(n));
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * nimg));
  CHK(ensure(c, c->stats, sizeof(int32_t) * GPC_STAT_STRIDE * nimg));
  if (npairs > 0) CHK(ensure(c, c->sstats, sizeof(int32_t) * GPC_STAT_STRIDE * 2 * npairs));
  uint32_t* codes = (uint32_t*)c->codes.p;
  int32_t* stats = (int32_t*)c->stats.p;
  const int thr = s->settings.gradient_threshold;
  if (wide) {
    CHK(ensure(c, c->smooth, n * nimg));
    CHK(ensure(c, c->grad, n * nimg));
    uint8_t* sm = (uint8_t*)c->smooth.p + n * off;
    uint8_t* gr = (uint8_t*)c->grad.p + n * off;
    CHK(run_preprocess(c, d_frames, nullptr, W, H, nframes, 1, thr, false, sm, gr, stats + GPC_STAT_STRIDE * off));
    CHK(run_hash(c, sm, gr, nullptr, W, H, nframes, false, codes + n * off, 0, 2, stats + GPC_STAT_STRIDE * off));
    if (off) CHK(dev_copy16(c, c->grad.p, s->cand.p, n));
  } else {
    CHK(run_preprocess(c, d_frames, nullptr, W, H, nframes, 1, thr, true, nullptr, nullptr, stats + GPC_STAT_STRIDE * off));
    CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, nframes, false, codes + n * off, 0, 2,
                 stats + GPC_STAT_STRIDE * off));
  }
  if (off) {
    CHK(dev_copy16(c, codes, s->codes.p, sizeof(uint32_t) * n));
    CHK(dev_copy16(c, stats, s->fstats.p, sizeof(int32_t) * GPC_STAT_STRIDE));
  }
  if (d_ncand) {
    Timed t(c, KID_TRS_NCAND);
    snprintf(c->launch_name[KID_TRS_NCAND], sizeof c->launch_name[0], "gpc::k_trs_ncand");
    hipLaunchKernelGGL(gpc::k_trs_ncand, dim3((nframes + 255) / 256), dim3(256), 0, c->stream,
                       (const int32_t*)(stats + GPC_STAT_STRIDE * off), d_ncand, nframes);
    HIPCHK(c, hipGetLastError());
  }
  int st = GPC_OK;
  if (npairs > 0) {
    const int nthr = 2 * npairs * GPC_STAT_STRIDE;
    hipLaunchKernelGGL(gpc::k_seq_stats, dim3((nthr + 255) / 256), dim3(256), 0, c->stream, (const int32_t*)stats,
                       (int32_t*)c->sstats.p, (int32_t*)nullptr, nimg);
    HIPCHK(c, hipGetLastError());
    std::swap(c->stats, c->sstats);
    st = run_match(c, W, H, npairs, &s->settings, 1, (const uint8_t*)c->grad.p, d_corr, cap, d_counts, nullptr, nullptr, true);
    std::swap(c->stats, c->sstats);
    if (st != GPC_OK && st != GPC_E_CAPACITY) return st;
  }
  // the links first (their workspaces may still fail to grow, and nothing of the carry has been touched by then), then the
  // carry of the next push: the last frame's codes, statistics and (wide) candidate bytes
  if (npairs > 0) CHK(trs_link(c, s, d_corr, d_counts, p, d_prev, d_track_id));
  CHK(dev_copy16(c, s->codes.p, codes + n * (size_t)(nimg - 1), sizeof(uint32_t) * n));
  CHK(dev_copy16(c, s->fstats.p, stats + GPC_STAT_STRIDE * (nimg - 1), sizeof(int32_t) * GPC_STAT_STRIDE));
  if (wide) CHK(dev_copy16(c, s->cand.p, (const uint8_t*)c->grad.p + n * (size_t)(nimg - 1), n));
  gpc::trs_commit(s->book, gpc::TRS_FRAMES, nframes, c->code_gen, p);
  return st;
}

// the running total, read back (the stream is waited for); tightens the bound on the ids
int trs_total(gpc_hip_ctx* c, gpc_hip_track_stream* s, int32_t* total) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(total, s->words.p + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
  gpc::trs_tighten(s->book, *total);
  return GPC_OK;
}

}  // namespace

int gpc_hip_track_stream_create(gpc_hip_ctx* c, int W, int H, const gpc_settings* settings, int cap_per_pair, int track_cap,
                                gpc_hip_track_stream** out) {
  if (!c || !out) return GPC_E_INVALID;
  *out = nullptr;
  CHK(gpc::trs_create_check(W, H, cap_per_pair, track_cap));
  if (settings) CHK(check_settings(settings));
  HIPCHK(c, hipSetDevice(c->device));
  gpc_hip_track_stream* s = new gpc_hip_track_stream();
  s->book.W = W, s->book.H = H, s->book.cap = cap_per_pair, s->book.track_cap = track_cap;
  if (settings) s->settings = *settings, s->have_settings = true;
  const size_t cap = (size_t)cap_per_pair;
  if (s->crec.alloc(pad16(sizeof(gpc::TrRec) * cap)) != hipSuccess || s->cid.alloc(pad16(sizeof(int32_t) * cap)) != hipSuccess ||
      s->words.alloc(16) != hipSuccess || s->table.alloc(sizeof(gpc_track) * (size_t)(track_cap > 0 ? track_cap : 1)) != hipSuccess ||
      hipMemsetAsync(s->words.p, 0, 16, c->stream) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(c->err, sizeof(c->err), "track stream of %d records per pair and %d rows: device allocation failed", cap_per_pair, track_cap);
    delete s;
    return GPC_E_HIP;
  }
  c->track_streams.push_back(s);
  *out = s;
  return GPC_OK;
}

int gpc_hip_track_stream_destroy(gpc_hip_ctx* c, gpc_hip_track_stream* s) {
  CHK(trs_check(c, s));
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (size_t k = 0; k < c->track_streams.size(); ++k)
    if (c->track_streams[k] == s) { c->track_streams.erase(c->track_streams.begin() + k); break; }
  delete s;
  return GPC_OK;
}

int gpc_hip_track_stream_reset(gpc_hip_ctx* c, gpc_hip_track_stream* s) {
  CHK(trs_check(c, s));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(s->words.p, 0, 16, c->stream));  // (behind whatever a push has queued)
  gpc::trs_reset(s->book);
  return GPC_OK;
}

int gpc_hip_track_stream_push_device(gpc_hip_ctx* c, gpc_hip_track_stream* s, const uint8_t* d_frames, int nframes,
                                     gpc_correspondence* d_corr, int32_t* d_counts, int32_t* d_ncand, int32_t* d_prev,
                                     int32_t* d_track_id, int* npairs) {
  if (!d_frames || !d_corr || !d_counts || !d_prev || !d_track_id || !npairs) return GPC_E_INVALID;
  gpc::TrsPush p;
  CHK(trs_frames_usable(c, s, nframes, &p));
  const int st = trs_push_frames(c, s, d_frames, nframes, d_corr, d_counts, d_ncand, d_prev, d_track_id, p);
  if (st == GPC_OK || st == GPC_E_CAPACITY) *npairs = p.k;
  return st;
}

int gpc_hip_track_stream_push_records_device(gpc_hip_ctx* c, gpc_hip_track_stream* s, const gpc_correspondence* d_corr,
                                             const int32_t* d_counts, int npairs, int32_t* d_prev, int32_t* d_track_id) {
  if (!d_corr || !d_counts || !d_prev || !d_track_id) return GPC_E_INVALID;
  CHK(trs_check(c, s));
  gpc::TrsPush p;
  CHK(gpc::trs_plan(s->book, gpc::TRS_RECORDS, npairs, c->code_gen, &p));
  HIPCHK(c, hipSetDevice(c->device));
  CHK(trs_link(c, s, d_corr, d_counts, p, d_prev, d_track_id));
  gpc::trs_commit(s->book, gpc::TRS_RECORDS, npairs, c->code_gen, p);
  return GPC_OK;
}

// Host frames in, the new pairs' records, links and ids out: one device block (Stage), the device form once over it.
int gpc_hip_track_stream_push(gpc_hip_ctx* c, gpc_hip_track_stream* s, const uint8_t* frames, int nframes, gpc_correspondence* corr,
                              int32_t* counts, int32_t* ncand, int32_t* prev, int32_t* track_id, int* npairs, int32_t* n_tracks) {
  if (!frames || !corr || !counts || !prev || !track_id || !npairs || !n_tracks) return GPC_E_INVALID;
  gpc::TrsPush p;
  CHK(trs_frames_usable(c, s, nframes, &p));
  CHK(host_call_begin(c));
  const int cap = s->book.cap, k = p.k;
  const size_t n = (size_t)s->book.W * s->book.H, rec = (size_t)k * cap;
  Stage st(c);
  const size_t r_in = st.in(n * nframes), r_corr = st.out(sizeof(gpc_correspondence) * rec), r_cnt = st.out(sizeof(int32_t) * (size_t)k),
               r_nc = st.out(sizeof(int32_t) * (size_t)nframes), r_prev = st.out(sizeof(int32_t) * rec),
               r_id = st.out(sizeof(int32_t) * rec);
  CHK(st.alloc(sizeof(int32_t) * ((size_t)k + nframes + 1)));  // counts [k], candidates [nframes], the number of tracks
  CHK(st.up(r_in, frames, n * nframes));
  int status = trs_push_frames(c, s, st.p(r_in), nframes, (gpc_correspondence*)st.p(r_corr), (int32_t*)st.p(r_cnt),
                               (int32_t*)st.p(r_nc), (int32_t*)st.p(r_prev), (int32_t*)st.p(r_id), p);
  if (status != GPC_OK && status != GPC_E_CAPACITY) return status;
  status = GPC_OK;
  int32_t* hc = c->h_cnt.p;
  if (k) CHK(st.down(hc, r_cnt, sizeof(int32_t) * (size_t)k));
  CHK(st.down(hc + k, r_nc, sizeof(int32_t) * (size_t)nframes));
  HIPCHK(c, hipMemcpyAsync(hc + k + nframes, s->words.p + 1, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  CHK(st.wait());
  for (int t = 0; t < k; ++t) {
    const size_t m = (size_t)valid_records(hc[t], cap), at = (size_t)t * cap;
    if (hc[t] > cap) status = GPC_E_CAPACITY;
    if (!m) continue;
    CHK(st.down(corr + at, r_corr + sizeof(gpc_correspondence) * at, sizeof(gpc_correspondence) * m));
    CHK(st.down(prev + at, r_prev + sizeof(int32_t) * at, sizeof(int32_t) * m));
    CHK(st.down(track_id + at, r_id + sizeof(int32_t) * at, sizeof(int32_t) * m));
  }
  CHK(st.wait());
  memcpy(counts, hc, sizeof(int32_t) * (size_t)k);
  if (ncand) memcpy(ncand, hc + k, sizeof(int32_t) * (size_t)nframes);
  *n_tracks = hc[k + nframes];
  gpc::trs_tighten(s->book, *n_tracks);
  *npairs = k;
  CHK(check_join_err(c));
  return status;
}

int gpc_hip_track_stream_state(gpc_hip_ctx* c, gpc_hip_track_stream* s, int* frames_seen, int* pairs_seen, int32_t* n_tracks) {
  CHK(trs_check(c, s));
  HIPCHK(c, hipSetDevice(c->device));
  int32_t total = 0;
  CHK(trs_total(c, s, &total));
  if (frames_seen) *frames_seen = s->book.frames_seen;
  if (pairs_seen) *pairs_seen = s->book.pairs_seen;
  if (n_tracks) *n_tracks = total;
  return GPC_OK;
}

int gpc_hip_track_stream_table(gpc_hip_track_stream* s, const gpc_track** d_tracks, const int32_t** d_ntracks) {
  if (!s || !d_tracks || !d_ntracks) return GPC_E_INVALID;
  *d_tracks = s->table.p;
  *d_ntracks = s->words.p + 1;
  return GPC_OK;
}

int gpc_hip_track_stream_read_tracks(gpc_hip_ctx* c, gpc_hip_track_stream* s, int first, int n, gpc_track* out, int32_t* n_tracks) {
  CHK(trs_check(c, s));
  if (!n_tracks || (n > 0 && !out)) return GPC_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  int32_t total = 0;
  CHK(trs_total(c, s, &total));
  *n_tracks = total;
  CHK(gpc::trs_read_check(s->book, first, n));
  const long end = (long)first + n < total ? (long)first + n : total;  // rows at total and beyond do not exist yet
  if (end > first) HIPCHK(c, hipMemcpy(out, s->table.p + first, sizeof(gpc_track) * (size_t)(end - first), hipMemcpyDeviceToHost));
  return GPC_OK;
}

}  // extern "C"

// (parts of this translation unit: see the note below the includes at the top)
#include "host_consensus.h"
#include "host_refine.h"
#include "host_pyramid.h"
#include "host_dense.h"
#include "host_quads.h"
#include "host_clean.h"
#include "host_search.h"
#include "host_aggregate.h"
#include "host_propagate.h"
#include "host_gapfill.h"
#include "host_inpaint.h"
#include "host_field_score.h"

extern "C" {

int gpc_hip_match_batch_device_packed(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H,
                                      int npairs, const gpc_settings* s, uint32_t* d_packed, int cap_per_pair,
                                      int32_t* d_rows, int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_packed || !d_rows || !d_counts || npairs <= 0 || cap_per_pair <= 0) return GPC_E_INVALID;
  CHK(check_settings(s));
  if (!s->epipolar_mode || s->use_hashtable) return GPC_E_UNSUPPORTED;  // rows are the unit of the packed form
  if (c->ngroups > 1) return GPC_E_UNSUPPORTED;
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * npairs));
  CHK(run_preprocess(c, d_rawL, d_rawR, W, H, npairs, 2, s->gradient_threshold, true));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * npairs, false,
               (uint32_t*)c->codes.p));
  const PackedOut po = {d_rows, (long)cap_per_pair, (long)H};
  CHK(run_match(c, W, H, npairs, s, 2, (const uint8_t*)c->grad.p, d_packed, cap_per_pair, d_counts, d_ncand, &po));
  return GPC_OK;
}

int gpc_hip_expand_packed(const uint32_t* packed, const int32_t* rows, int H, int n, gpc_support* out) {
  if (!packed || !rows || !out || H < 2 * GPC_R || n < 0) return GPC_E_INVALID;
  expand_rows(packed, rows, GPC_R, H - GPC_R, 0, n, out);
  return GPC_OK;
}

// One pair or two, page-locked `out` (BASELINE configs[1] taken literally: the reference's timed region for ONE pair).
// The chunk pipeline of match_batch_packed is built for the link's throughput: three streams, events, packed records
// and a pool of host threads that expand them -- for one pair that machinery IS the latency (0.20-0.24 ms against
// ~36 us of kernels and ~35 us of link time).  Here everything is queued on the context's stream and the join writes
// the 12-byte supports, the counts and the candidate counts straight into host memory over the link (consecutive
// lanes write consecutive records: whole PCIe write bursts) while it runs; one stream synchronisation ends the call.
static int match_batch_direct(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs,
                              const gpc_settings* s, gpc_support* d_out_host, int cap, int32_t* counts, int32_t* ncand) {
  const size_t n = (size_t)W * H;
  CHK(ensure(c, c->raw, 2 * n * npairs));
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * npairs));
  CHK(pinned_counts(c, npairs));
  int32_t* d_cnt = nullptr;
  HIPCHK(c, hipHostGetDevicePointer((void**)&d_cnt, c->h_cnt.p, 0));
  uint8_t* d_l = (uint8_t*)c->raw.p;
  uint8_t* d_r = d_l + n * npairs;
  // Page-locked images are fetched by a kernel (one launch, both sides) instead of two copy-engine submissions; the
  // byte count is a multiple of 16 (W is), the pointers must be 16-byte aligned (gpc_hip_host_alloc's are)
  const void* vL = c->upload_mode ? device_view_of_host(rawL) : nullptr;
  const void* vR = vL ? device_view_of_host(rawR) : nullptr;
  const bool aligned = (((uintptr_t)vL | (uintptr_t)vR | (uintptr_t)d_l | (uintptr_t)d_r) & 15u) == 0 && (n * npairs) % 16 == 0 &&
                       n * npairs / 16 < (1ull << 31);
  if (vL && vR && aligned && c->upload_mode == 2) {  // the preprocess kernel reads the host's pages itself
    d_l = (uint8_t*)vL;
    d_r = (uint8_t*)vR;
  } else if (vL && vR && aligned) {
    const unsigned n16 = (unsigned)(n * npairs / 16);
    hipLaunchKernelGGL(gpc::k_upload2, dim3((n16 + 255) / 256, 2), dim3(256), 0, c->stream, (const uint4*)vL, (const uint4*)vR,
                       (uint4*)d_l, (uint4*)d_r, n16);
    HIPCHK(c, hipGetLastError());
  } else {  // pageable images (or unaligned ones): CPU copy into the page-locked arena, one upload launch from there
    uint8_t* d_arena = nullptr;
    const size_t side = pad16(n * npairs);
    CHK(xfer_reserve(c, 2 * side, &d_arena));
    memcpy(c->h_xfer.p, rawL, n * npairs);
    memcpy(c->h_xfer.p + side, rawR, n * npairs);
    const unsigned n16 = (unsigned)(side / 16);
    CHK(ensure(c, c->raw, 2 * side));
    d_l = (uint8_t*)c->raw.p;
    d_r = d_l + side;
    hipLaunchKernelGGL(gpc::k_upload2, dim3((n16 + 255) / 256, 2), dim3(256), 0, c->stream, (const uint4*)d_arena,
                       (const uint4*)(d_arena + side), (uint4*)d_l, (uint4*)d_r, n16);
    HIPCHK(c, hipGetLastError());
  }
  CHK(run_preprocess(c, d_l, d_r, W, H, npairs, 2, s->gradient_threshold, true));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * npairs, false, (uint32_t*)c->codes.p));
  CHK(run_match(c, W, H, npairs, s, 0, (const uint8_t*)c->grad.p, d_out_host, cap, d_cnt, d_cnt + npairs));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHK(check_join_err(c));
  int status = GPC_OK;
  for (int p = 0; p < npairs; ++p) {
    counts[p] = c->h_cnt.p[p];
    if (counts[p] > cap) status = GPC_E_CAPACITY;
    if (ncand) {
      ncand[2 * p] = c->h_cnt.p[npairs + 2 * p];
      ncand[2 * p + 1] = c->h_cnt.p[npairs + 2 * p + 1];
    }
  }
  return status;
}

// Host buffers in, supports out, for the epipolar sort-matcher (the reference's sparsematch settings): results
// cross the link PACKED (4 bytes per support + the row counts instead of 12 bytes per support) and worker threads
// expand them into the caller's ndb::Support arrays while the next chunks are uploaded, matched and downloaded.
// Per chunk k:  upload (s_in) -> kernels (stream) -> counts (s_cnt) | download of k-1 (s_out) | expansion of k-2 (pool).
// Device results rotate through 3 slots, the page-locked landing area through 4.
// ph != null: the results are LEFT packed in the caller's arrays (gpc_hip_match_batch_packed) instead of being expanded into `out`
struct PackedHost {
  uint32_t* packed;  // [npairs][cap] words xL | xR << 16
  int32_t* rows;     // [npairs][H] supports per row
};
static int match_batch_packed(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs,
                              const gpc_settings* s, gpc_support* out, int cap, int32_t* counts, int32_t* ncand,
                              const PackedHost* ph = nullptr) {
  if (!c || !rawL || !rawR || (!out && !ph) || !counts || npairs <= 0 || cap <= 0) return GPC_E_INVALID;
  if (ph && (!ph->packed || !ph->rows)) return GPC_E_INVALID;
  const double t_entry = host_ms();
  c->stage_ms[0] = c->stage_ms[1] = c->stage_ms[2] = c->stage_ms[3] = 0.f;
  CHK(check_settings(s));
  if (!s->epipolar_mode || s->use_hashtable) {
    if (ph) return GPC_E_UNSUPPORTED;  // rows are the unit of the packed format: the epipolar sort-matcher's
    return match_batch_unpacked(c, rawL, rawR, W, H, npairs, s, out, cap, counts, ncand);
  }
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  if (!ph && npairs <= c->direct_max && (uint64_t)cap * sizeof(gpc_support) < (1ull << 32))
    if (void* dv = device_view_of_host(out))
      return match_batch_direct(c, rawL, rawR, W, H, npairs, s, (gpc_support*)dv, cap, counts, ncand);
  const size_t n = (size_t)W * H;
  int chunk = npairs < 4 ? npairs : (npairs / 8 < 1 ? 1 : (npairs / 8 > 16 ? 16 : npairs / 8));
  if (c->chunk_pairs > 0) chunk = c->chunk_pairs < npairs ? c->chunk_pairs : npairs;
  // Chunk schedule: full chunks in the middle; the FIRST one is split 1/4 + 3/4 (kernels start after a quarter of an
  // upload) and the LAST one 1/2 + 1/4 + 1/4 (the tail after the last upload -- its kernels, download and expansion --
  // covers 4 pairs instead of 16).  Slots are sized for a full chunk.
  std::vector<int> c_start, c_size;
  {
    int rem = npairs, at = 0;
    auto put = [&](int m) {
      if (m <= 0) return;
      c_start.push_back(at);
      c_size.push_back(m);
      at += m;
      rem -= m;
    };
    // (chunks of 8 split further cost more per-chunk overhead than they hide: 64 pairs 2.05 vs 1.67 ms; 256 pairs, chunks of
    // 16: 5.33 vs 5.87 ms)
    const bool shaped = !c->flat_chunks && chunk >= 16 && npairs >= 4 * chunk;
    if (shaped) {
      put(chunk / 4);
      put(chunk - chunk / 4);
    }
    while (rem > chunk) put(chunk);
    if (shaped && rem >= 4) {
      const int r = rem;
      put(r / 2);
      put(r / 4);
      put(r - r / 2 - r / 4);
    } else {
      put(rem);
    }
  }
  const int nch = (int)c_size.size();
  // (three-byte records x | (x - xR + dispHigh) << xbits were tried for the link: byte stores on the device and a
  // byte shuffle on the host made the call slower, 7.5 vs 6.2 ms per 256 pairs; the link is not the limit any more)
  const size_t rec = 4;
  const size_t hpad = ((size_t)H + 3) & ~(size_t)3;
  // a chunk's results: [row counts: chunk x hpad words | the pairs' records back to back | pad] -- one copy per chunk
  const size_t cb = 4 * hpad * chunk + ((rec * (size_t)cap * chunk + 15) & ~(size_t)15) + 16;
  CHK(ensure(c, c->raw, 2 * 2 * n * chunk));  // two slots x two sides
  CHK(ensure(c, c->packed, 3 * cb + sizeof(int32_t) * 3 * chunk));
  CHK(ensure(c, c->counts, sizeof(int32_t) * npairs));
  CHK(ensure(c, c->ncand, sizeof(int32_t) * 2 * npairs));
  const size_t stage_bytes = 4 * cb;
  if (stage_bytes > c->h_stage.cap) {
    c->pool.wait_all();
    CHK(ensure_pinned(c, c->h_stage, stage_bytes));
  }
  CHK(pinned_counts(c, npairs));
  int32_t* hc = c->h_cnt.p;               // counts
  int32_t* hn = c->h_cnt.p + npairs;      // candidate counts
  CHK(batch_streams(c));
  // Pageable input images (malloc, std::vector, ndb::Buffer): a copy engine cannot read them, and hipMemcpyAsync then stages
  // them itself, synchronously, on the calling thread -- which serialised the whole chunk pipeline (32 pairs: 7.5 ms
  // against 1.1 ms from page-locked memory).  The workers copy a chunk into a page-locked bounce buffer instead (two
  // slots) while the device works on the chunks before it, and the upload runs from there.
  // (from four pairs on: for one pair waking the workers costs more than the runtime's own staging)
  // (every pageable batch, one pair included: memory hipMemcpy has seen stalls the queues when its owner frees it --
  // gpc_hip_ctx::h_xfer)
  const bool bounce = !device_view_of_host(rawL) || !device_view_of_host(rawR);
  if (bounce) {
    const size_t need = 2 * 2 * n * (size_t)chunk;
    if (need > c->h_in.cap) {
      HIPCHK(c, hipStreamSynchronize(c->s_in));
      CHK(ensure_pinned(c, c->h_in, need));
    }
  }
  {  // numThreads_ of the reference's settings asks for that many workers; otherwise what the process may use
    // (measured, 256 pairs: 3 .. 10 workers all keep up with the link -- 8.7 .. 8.9 ms per call, the link's 57 GB/s
    // shared by both directions being the limit; 14 workers on a 16-CPU share: 10.9 ms)
    int nt = c->expand_threads > 0 ? c->expand_threads : (s->num_threads > 1 ? s->num_threads : default_expand_threads());
    nt = nt < 1 ? 1 : (nt > 32 ? 32 : nt);
    c->pool.start(nt, c->have_node_cpus ? &c->node_cpus : nullptr, &c->node_l3);
  }
  uint8_t* d_pk = (uint8_t*)c->packed.p;
  uint8_t* h_pk = (uint8_t*)c->h_stage.p;
  int status = GPC_OK;
  int32_t* d_tot = reinterpret_cast<int32_t*>(d_pk + 3 * cb);  // [3][chunk] scratch of k_pair_totals
  // the counts of chunk k are on their way: wait for them, then fetch the chunk's row counts and records in one copy
  auto download = [&](int k) -> int {
    const int p0 = c_start[k], pc = c_size[k];
    HIPCHK(c, hipEventSynchronize(c->e_cnt[k & 3]));
    memcpy(counts + p0, hc + p0, sizeof(int32_t) * pc);
    if (ncand) memcpy(ncand + 2 * p0, hn + 2 * p0, sizeof(int32_t) * 2 * pc);
    c->pool.wait_slot(k & 3);  // the expansion of chunk k-4 has left this landing slot
    size_t recs = 0;
    for (int i = 0; i < pc; ++i) {
      const int cnt = counts[p0 + i];
      if (cnt > cap) status = GPC_E_CAPACITY;
      recs += (size_t)(cnt < cap ? cnt : cap);
    }
    const size_t bytes = 4 * hpad * chunk + rec * recs;
    HIPCHK(c, hipMemcpyAsync(h_pk + (size_t)(k & 3) * cb, d_pk + (size_t)(k % 3) * cb, bytes, hipMemcpyDeviceToHost, c->s_out));
    HIPCHK(c, hipEventRecord(c->e_out[k & 3], c->s_out));
    return GPC_OK;
  };
  auto expand = [&](int k) -> int {
    const int p0 = c_start[k], pc = c_size[k];
    HIPCHK(c, hipEventSynchronize(c->e_out[k & 3]));
    const int parts = c->pool.size() >= 8 ? 4 : 2;
    const uint8_t* slot = h_pk + (size_t)(k & 3) * cb;
    const uint8_t* recs = slot + 4 * hpad * chunk;
    for (int i = 0; i < pc; ++i) {
      const int32_t* rows = reinterpret_cast<const int32_t*>(slot) + (size_t)i * hpad;
      const int cnt = counts[p0 + i];
      const long limit = cnt < cap ? cnt : cap;
      long first = 0;
      if (ph) {  // the pair's words and row counts as they came over the link: two plain copies instead of the expansion
        ExpandJob j = {};
        j.slot = k & 3;
        int32_t* rdst = ph->rows + (size_t)(p0 + i) * H;   // rows 13 .. H-14 are the device's; the margins hold no support
        memset(rdst, 0, sizeof(int32_t) * GPC_R);
        memset(rdst + H - GPC_R, 0, sizeof(int32_t) * GPC_R);
        j.copy_src = rows + GPC_R;
        j.copy_dst = rdst + GPC_R;
        j.copy_bytes = sizeof(int32_t) * (size_t)(H - 2 * GPC_R);
        c->pool.push(j);
        if (limit > 0) {
          j.copy_src = recs;
          j.copy_dst = ph->packed + (size_t)(p0 + i) * cap;
          j.copy_bytes = rec * (size_t)limit;
          c->pool.push(j);
        }
        recs += rec * (size_t)limit;
        continue;
      }
      for (int q = 0; q < parts; ++q) {
        const int y0 = GPC_R + (int)((long)(H - 2 * GPC_R) * q / parts), y1 = GPC_R + (int)((long)(H - 2 * GPC_R) * (q + 1) / parts);
        if (first < limit && y1 > y0)
          c->pool.push(ExpandJob{reinterpret_cast<const uint32_t*>(recs), rows, H, y0, y1, (int)first, (int)limit,
                                 out + (size_t)(p0 + i) * cap, k & 3});
        for (int y = y0; y < y1; ++y) first += rows[y];
      }
      recs += rec * (size_t)limit;  // the next pair's records follow directly
    }
    return GPC_OK;
  };
  for (int k = 0; k < nch; ++k) {
    const int ev = k & 3, p0 = c_start[k], pc = c_size[k];
    uint8_t* d_l = (uint8_t*)c->raw.p + (size_t)(k & 1) * 2 * n * chunk;
    uint8_t* d_r = d_l + n * chunk;
    if (k >= 2) HIPCHK(c, hipStreamWaitEvent(c->s_in, c->e_comp[(k - 2) & 3], 0));  // chunk k-2 has read this slot
    const uint8_t *srcL = rawL + (size_t)p0 * n, *srcR = rawR + (size_t)p0 * n;
    if (bounce) {
      uint8_t* bl = (uint8_t*)c->h_in.p + (size_t)(k & 1) * 2 * n * chunk;
      uint8_t* br = bl + n * chunk;
      if (k >= 2) HIPCHK(c, hipEventSynchronize(c->e_in[(k - 2) & 3]));  // the upload of chunk k-2 has left this bounce slot
      const int pieces = c->pool.size() > 1 ? c->pool.size() : 1;
      const size_t bytes = n * pc, step = (bytes / pieces + 4095) & ~(size_t)4095;
      for (int side = 0; side < 2; ++side)
        for (size_t at = 0; at < bytes; at += step) {
          ExpandJob j = {};
          j.slot = 7;  // a wait slot of its own: the landing slots of the results use 0 .. 3
          j.copy_src = (side ? srcR : srcL) + at;
          j.copy_dst = (side ? br : bl) + at;
          j.copy_bytes = at + step <= bytes ? step : bytes - at;
          c->pool.push(j);
        }
      c->pool.wait_slot(7);
      srcL = bl;
      srcR = br;
    }
    HIPCHK(c, hipMemcpyAsync(d_l, srcL, n * pc, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipMemcpyAsync(d_r, srcR, n * pc, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipEventRecord(c->e_in[ev], c->s_in));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->e_in[ev], 0));
    if (k >= 3) HIPCHK(c, hipStreamWaitEvent(c->stream, c->e_out[(k - 3) & 3], 0));  // chunk k-3 has left this result slot
    uint8_t* slot = d_pk + (size_t)(k % 3) * cb;
    CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * pc));
    CHK(run_preprocess(c, d_l, d_r, W, H, pc, 2, s->gradient_threshold, true));
    CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * pc, false, (uint32_t*)c->codes.p));
    const PackedOut po = {reinterpret_cast<int32_t*>(slot), 0l, (long)hpad, d_tot + (size_t)(k % 3) * chunk};
    CHK(run_match(c, W, H, pc, s, 2, (const uint8_t*)c->grad.p, slot + 4 * hpad * chunk, cap, (int32_t*)c->counts.p + p0,
                  (int32_t*)c->ncand.p + 2 * p0, &po));
    HIPCHK(c, hipEventRecord(c->e_comp[ev], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_cnt, c->e_comp[ev], 0));
    HIPCHK(c, hipMemcpyAsync(hc + p0, (int32_t*)c->counts.p + p0, sizeof(int32_t) * pc, hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipMemcpyAsync(hn + 2 * p0, (int32_t*)c->ncand.p + 2 * p0, sizeof(int32_t) * 2 * pc, hipMemcpyDeviceToHost, c->s_cnt));
    HIPCHK(c, hipEventRecord(c->e_cnt[ev], c->s_cnt));
    if (k >= 1) CHK(download(k - 1));
    if (k >= 2) CHK(expand(k - 2));
  }
  HIPCHK(c, hipEventSynchronize(c->e_in[(nch - 1) & 3]));  // (queued long before the kernels that follow it: no wait is added)
  c->stage_ms[0] = (float)(host_ms() - t_entry);
  CHK(download(nch - 1));
  c->stage_ms[1] = (float)(host_ms() - t_entry);
  if (nch >= 2) CHK(expand(nch - 2));
  CHK(expand(nch - 1));
  c->stage_ms[2] = (float)(host_ms() - t_entry);
  c->pool.wait_all();
  HIPCHK(c, hipStreamSynchronize(c->s_cnt));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHK(check_join_err(c));
  c->stage_ms[3] = (float)(host_ms() - t_entry);
  return status;
}

int gpc_hip_fed_calls(const gpc_hip_ctx* c) { return c ? c->fed_calls : 0; }

int gpc_hip_match_batch(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs,
                        const gpc_settings* s, gpc_support* out, int cap, int32_t* counts, int32_t* ncand) {
  if (c && c->ngroups > 1) return GPC_E_UNSUPPORTED;
  // One pair into a pageable array: the two-step form (results packed over the link, expanded by the workers): 0.20 ms
  // where the chunk pipeline's machinery took 0.27.  (A page-locked array is written by the kernels themselves: below.)
  if (c && npairs == 1 && rawL && rawR && out && counts && cap > 0 && s && !device_view_of_host(out)) {
    CHK(gpc_hip_match_pair_begin(c, rawL, rawR, W, H, s));
    int n = 0, nl = 0, nr = 0;
    const int st1 = match_fetch(c, out, cap, &n, &nl, &nr);
    c->pend.active = false;
    counts[0] = n;
    if (ncand) { ncand[0] = nl; ncand[1] = nr; }
    return st1;
  }
  const int st = on_gpu_node(c, npairs, [&] { return match_batch_packed(c, rawL, rawR, W, H, npairs, s, out, cap, counts, ncand); });
  if (c && st != GPC_OK && st != GPC_E_CAPACITY && st != GPC_E_INVALID) {
    // An error left the chunk pipeline half way: expansion jobs may still write into `out`, copies may still
    // target the staging slots.  Nothing of this call may be in flight when the caller gets its buffers back.
    c->pool.wait_all();
    if (c->s_in) {
      (void)hipStreamSynchronize(c->s_in);
      (void)hipStreamSynchronize(c->s_out);
      (void)hipStreamSynchronize(c->s_cnt);
    }
    if (c->s_aux) (void)hipStreamSynchronize(c->s_aux);
    (void)hipStreamSynchronize(c->stream);
  }
  return st;
}

int gpc_hip_match_batch_packed(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs,
                               const gpc_settings* s, uint32_t* packed, int cap, int32_t* rows, int32_t* counts, int32_t* ncand) {
  if (c && c->ngroups > 1) return GPC_E_UNSUPPORTED;
  const PackedHost ph = {packed, rows};
  const int st = on_gpu_node(c, npairs, [&] { return match_batch_packed(c, rawL, rawR, W, H, npairs, s, nullptr, cap, counts, ncand, &ph); });
  if (c && st != GPC_OK && st != GPC_E_CAPACITY && st != GPC_E_INVALID && st != GPC_E_UNSUPPORTED) {
    c->pool.wait_all();   // (as in gpc_hip_match_batch: nothing of a failed call may still be in flight)
    if (c->s_in) {
      (void)hipStreamSynchronize(c->s_in);
      (void)hipStreamSynchronize(c->s_out);
      (void)hipStreamSynchronize(c->s_cnt);
    }
    (void)hipStreamSynchronize(c->stream);
  }
  return st;
}

int gpc_hip_host_threads(const gpc_hip_ctx* c) { return c ? c->pool.size() : 0; }

int gpc_hip_batch_stages(const gpc_hip_ctx* c, float* ms4) {
  if (!c || !ms4) return GPC_E_INVALID;
  for (int i = 0; i < 4; ++i) ms4[i] = c->stage_ms[i];
  return GPC_OK;
}

int gpc_hip_hash_plan(gpc_hip_ctx* c, int32_t out[4]) {
  if (!c || !out || !c->hash_plan[0]) return GPC_E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = c->hash_plan[i];
  return GPC_OK;
}

int gpc_hip_host_worker_cpus(gpc_hip_ctx* c, int* cpus, int cap) {
  if (!c || (cap > 0 && !cpus) || cap < 0) return 0;
  return c->pool.worker_cpus(cpus, cap);
}
int gpc_hip_host_numa_node(const gpc_hip_ctx* c) { return (c && c->have_node_cpus) ? c->numa_node : -1; }

// The whole timed region of samples/sparsematch.cpp:45-52 for one pair, queued: images through the arena (or read where
// they lie when page-locked), the batched pipeline for one pair, results into the arena for gpc_hip_match_fetch.
int gpc_hip_match_pair_begin(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, const gpc_settings* s) {
  if (!c || !rawL || !rawR) return GPC_E_INVALID;
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  HIPCHK(c, hipSetDevice(c->device));
  c->pend.active = false;
  c->pre_slot = -1;
  const size_t n = (size_t)W * H;
  int cap_dev = (W - 2 * GPC_R) * (H - 2 * GPC_R) + 1;  // no pair has more supports than an image has candidates
  const bool groups = c->ngroups > 1;   // (group mode: the union stays on the device until match_fetch knows its size)
  if (groups && s->use_hashtable) return GPC_E_UNSUPPORTED;
  const bool packed = s->epipolar_mode && !s->use_hashtable && !c->no_pair_packed && !groups;  // (as in match_preprocessed_begin)
  const size_t rows_bytes = pad16(sizeof(int32_t) * (size_t)H);
  const size_t out_bytes = groups ? 0 : packed ? rows_bytes + pad16(sizeof(uint32_t) * (size_t)cap_dev) : pad16(sizeof(gpc_support) * (size_t)cap_dev);
  CHK(ensure(c, c->raw, 2 * n));
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2));
  CHK(pinned_counts(c, 1));
  int32_t* d_cnt = nullptr;
  HIPCHK(c, hipHostGetDevicePointer((void**)&d_cnt, c->h_cnt.p, 0));
  uint8_t* d_arena = nullptr;
  CHK(xfer_reserve(c, out_bytes + 2 * n, &d_arena));
  const uint8_t* vL = static_cast<const uint8_t*>(device_view_of_host(rawL));
  const uint8_t* vR = vL ? static_cast<const uint8_t*>(device_view_of_host(rawR)) : nullptr;
  if (!vL || !vR || (((uintptr_t)vL | (uintptr_t)vR) & 15u)) {
    memcpy(c->h_xfer.p + out_bytes, rawL, n);
    memcpy(c->h_xfer.p + out_bytes + n, rawR, n);
    vL = d_arena + out_bytes;
    vR = vL + n;
  }
  uint8_t* d_l = (uint8_t*)c->raw.p;
  uint8_t* d_r = d_l + n;
  const unsigned n16 = (unsigned)(n / 16);
  hipLaunchKernelGGL(gpc::k_upload2, dim3((n16 + 255) / 256, 2), dim3(256), 0, c->stream, (const uint4*)vL, (const uint4*)vR,
                     (uint4*)d_l, (uint4*)d_r, n16);
  HIPCHK(c, hipGetLastError());
  CHK(run_preprocess(c, d_l, d_r, W, H, 1, 2, s->gradient_threshold, true));
  c->pend.dev_out = nullptr;
  if (groups) {
    const long cap_u = (long)c->ngroups * (cap_dev - 1) + 1;
    CHK(ensure(c, c->gdense, sizeof(gpc_support) * (size_t)cap_u));
    CHK(run_group_match(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 1, s, 0,
                        (const uint8_t*)c->grad.p, c->gdense.p, cap_u, d_cnt, d_cnt + 1));
    cap_dev = (int)std::min(cap_u, (long)INT32_MAX);
    c->pend.dev_out = c->gdense.p;
  } else {
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2, false, (uint32_t*)c->codes.p));
  if (packed) {
    const PackedOut po = {reinterpret_cast<int32_t*>(d_arena), (long)cap_dev, (long)H};
    CHK(run_match(c, W, H, 1, s, 2, (const uint8_t*)c->grad.p, d_arena + rows_bytes, cap_dev, d_cnt, d_cnt + 1, &po));
  } else {
    CHK(run_match(c, W, H, 1, s, 0, (const uint8_t*)c->grad.p, d_arena, cap_dev, d_cnt, d_cnt + 1));
  }
  }
  c->pend.active = true;
  c->pend.direct = false;
  c->pend.have_ncand = true;
  c->pend.packed = packed;
  c->pend.esz = sizeof(gpc_support);
  c->pend.cap_dev = cap_dev;
  c->pend.H = H;
  return GPC_OK;
}

int gpc_hip_match_pair(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H,
                       const gpc_settings* s, gpc_support* out, int cap, int* n_out, int* n_cand_l,
                       int* n_cand_r) {
  if (!n_out) return GPC_E_INVALID;
  int32_t cnt = 0, nc[2] = {0, 0};
  if (c && c->ngroups > 1) {  // group mode: always the two-step form (gpc_hip_match_batch refuses group mode)
    if (cap < 0 || (cap > 0 && !out)) return GPC_E_INVALID;
    CHK(gpc_hip_match_pair_begin(c, rawL, rawR, W, H, s));
    int n = 0, nl = 0, nr = 0;
    const int st1 = match_fetch(c, out, cap, &n, &nl, &nr);
    c->pend.active = false;
    *n_out = n;
    if (n_cand_l) *n_cand_l = nl;
    if (n_cand_r) *n_cand_r = nr;
    return st1;
  }
  const int st = gpc_hip_match_batch(c, rawL, rawR, W, H, 1, s, out, cap, &cnt, nc);
  *n_out = cnt;
  if (n_cand_l) *n_cand_l = nc[0];
  if (n_cand_r) *n_cand_r = nc[1];
  return st;
}


// ------------------------------------------------------------------ warm-up

// Everything a first call would otherwise pay for inside the caller's timed region (the reference's sample starts its
// clock AFTER readForest, samples/sparsematch.cpp:42-45): the module's code objects, the workspaces of one pair of
// width x height, page-locked staging, streams, events and worker threads -- by running the host entry points once on a
// synthetic textured pair of that size (SURVEY 8d's generator) and throwing the results away.
// settings == NULL: the four matcher modes (epipolar x hashtable) with the reference's sparsematch thresholds.
int gpc_hip_warmup(gpc_hip_ctx* c, int W, int H, const gpc_settings* settings) {
  if (!c) return GPC_E_INVALID;
  CHK(check_dims(W, H));
  CHK(forest_matches(c, W, H));
  if (settings) CHK(check_settings(settings));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)W * H;
  auto mix = [](uint32_t a, uint32_t b) {
    uint32_t h = a * 73856093u ^ b * 19349663u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
  };
  // page-locked images and results: the single-pair path of gpc_hip_match_batch that Forest::matchPair takes
  Pinned<uint8_t> pin;  // (freed on every return)
  const size_t cap = n / 2 + 1;
  CHK(ensure_pinned(c, pin, 2 * n + sizeof(gpc_support) * cap));
  uint8_t *L = pin.p, *R = pin.p + n;
  gpc_support* pout = reinterpret_cast<gpc_support*>(pin.p + 2 * n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W + 8; ++x) {
      const uint8_t v = (uint8_t)((((mix((uint32_t)x >> 2, (uint32_t)y >> 2) & 0xFF) * 3 + (mix((uint32_t)x, (uint32_t)y) & 0x3F)) >> 2));
      if (x < W) R[(size_t)y * W + x] = v;          // R(x) = P(x), L(x) = P(x + 8): disparity 8 everywhere
      if (x >= 8) L[(size_t)y * W + x - 8] = v;
    }
  int st = GPC_OK;
  {
    std::vector<uint8_t> sm[2] = {std::vector<uint8_t>(n), std::vector<uint8_t>(n)}, gr[2] = {std::vector<uint8_t>(n), std::vector<uint8_t>(n)};
    std::vector<int32_t> mk[2];
    int nm[2] = {0, 0};
    const uint8_t* raw[2] = {L, R};
    const int thr = settings ? settings->gradient_threshold : 5;
    const int maxcand = (W - 2 * GPC_R) * (H - 2 * GPC_R);
    for (int side = 0; side < 2 && st == GPC_OK; ++side) {
      st = gpc_hip_preprocess_begin(c, raw[side], W, H, thr);
      mk[side].resize((size_t)maxcand + 1);
      if (st == GPC_OK) st = gpc_hip_preprocess_fetch(c, sm[side].data(), gr[side].data(), mk[side].data(), maxcand, &nm[side]);
    }
    gpc_settings modes[4];
    int nmodes = 0;
    if (settings) modes[nmodes++] = *settings;
    else
      for (int k = 0; k < 4; ++k) modes[nmodes++] = gpc_settings{5, 128, 0, (k & 1) ? 0 : 1, (k >> 1) & 1, 1};
    // (group mode: a union holds up to ngroups times as many records; no hash-table matcher, no gpc_hip_match_batch)
    const bool groups = c->ngroups > 1;
    std::vector<gpc_support> out(((size_t)(nm[0] < nm[1] ? nm[0] : nm[1]) + 1) * (groups ? c->ngroups : 1));
    const int keep = c->resident_mode, hits = c->resident_hits;
    for (int k = 0; k < nmodes && st == GPC_OK; ++k) {
      if (groups && modes[k].use_hashtable) continue;
      int ns = 0;
      for (int pass = 0; pass < 2 && st == GPC_OK; ++pass) {  // from the resident images, then the upload path
        c->resident_mode = pass == 0 ? keep : 0;
        st = gpc_hip_rectified_match(c, sm[0].data(), gr[0].data(), mk[0].data(), nm[0], sm[1].data(), gr[1].data(), mk[1].data(),
                                     nm[1], W, H, &modes[k], out.data(), (int)out.size(), &ns);
      }
      c->resident_mode = keep;
      int32_t cnt = 0, nc[2];
      if (st == GPC_OK && !groups) st = gpc_hip_match_batch(c, L, R, W, H, 1, &modes[k], pout, (int)cap, &cnt, nc);     // page-locked
      if ((st == GPC_OK || st == GPC_E_CAPACITY) && !groups) st = gpc_hip_match_batch(c, sm[0].data(), sm[1].data(), W, H, 1, &modes[k], out.data(), (int)out.size(), &cnt, nc);  // pageable
      if (st == GPC_OK || st == GPC_E_CAPACITY) st = gpc_hip_match_pair_begin(c, sm[0].data(), sm[1].data(), W, H, &modes[k]);   // Forest::matchPair
      if (st == GPC_OK) st = gpc_hip_match_fetch(c, out.data(), (int)out.size(), &ns, nullptr, nullptr);
      if (st == GPC_E_CAPACITY) st = GPC_OK;
    }
    c->resident_mode = keep;
    c->resident_hits = hits;
    std::lock_guard<std::mutex> g(g_res_mu);  // the host copies die with this scope
    c->res[0].valid = c->res[1].valid = false;
  }
  return st;
}

// ------------------------------------------------------------------ fern training (k_train.h)

namespace {

void split_stats(int tp, int fp, int fn, int tot, double w1, gpc_split_stats* s) {
  // Fern.hpp:255-261, same expressions in the same order
  s->tp = tp;
  s->fp = fp;
  s->fn = fn;
  s->tot = tot;
  const double w2 = 1. - w1;
  s->prec = ((tp + fp) == 0) ? 0. : double(tp) / (tp + fp);
  s->rec = ((tp + fn) == 0) ? 0. : double(tp) / (tp + fn);
  s->hmean = (s->prec + s->rec == 0.) ? 0. : s->prec * s->rec / ((1. - w2) * s->prec + w2 * s->rec);
  s->convcomb = (1. - w2) * s->prec + w2 * s->rec;
}

int train_check(gpc_hip_ctx* c, gpc_hip_train_set* t) {
  if (!c || !t || t->owner != c) return GPC_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  return GPC_OK;
}

int train_scratch(gpc_hip_ctx* c, gpc_hip_train_set* t, size_t ncounts, size_t ncand) {
  CHK(ensure(c, t->counts, sizeof(int32_t) * ncounts));
  return ensure(c, t->d_cand, sizeof(gpc::GpcSplit) * ncand);
}

bool split_ok(const gpc_split& p) { return p.i >= 0 && p.i < TS_PATCH && p.j >= 0 && p.j < TS_PATCH; }

// The candidate loop of Fern::train for one level (Fern.hpp:336-352) over counts already taken: tp / fp [num_resamples][ntau],
// `tot` samples counted.  *best and *stats carry over from the level before: a level on which nothing scores above 0 keeps
// the previous winner (:352), and the statistics are those of the last candidate evaluated (:357).
void select_level(const gpc_split* cand, int num_resamples, int taulo, int ntau, const int32_t* tp, const int32_t* fp,
                  int32_t tot, double w1, gpc_split* best, gpc_split_stats* stats) {
  float max_score = 0.f;
  for (int k = 0; k < num_resamples; ++k) {
    gpc_split p = cand[k];                                                  // sampleHyperplane          :339
    for (int q = 0; q < ntau; ++q) {
      p.tau = taulo + q;
      const int a = tp[(size_t)k * ntau + q], b = fp[(size_t)k * ntau + q];
      split_stats(a, b, tot - a - b, tot, w1, stats);                      // evalSplit                  :343
      if (stats->hmean > max_score) {                                       // double against float       :346
        *best = p;
        max_score = (float)stats->hmean;
      }
    }
  }
}

}  // namespace

int gpc_hip_train_set_create(gpc_hip_ctx* c, const uint8_t* triplets, int n, gpc_hip_train_set** out) {
  if (!c || !triplets || n <= 0 || !out) return GPC_E_INVALID;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  std::unique_ptr<gpc_hip_train_set> t(new gpc_hip_train_set());  // (every early return frees the set and d_aos)
  t->owner = c;
  t->n = n;
  t->np = ((long)n + 255) / 256 * 256;
  DevBlock<uint8_t> d_aos;
  const size_t bytes = (size_t)n * 3 * TS_PATCH;
  if (d_aos.alloc(bytes) != hipSuccess || t->planes.alloc((size_t)3 * TS_PATCH * t->np) != hipSuccess ||
      t->flags.alloc((size_t)t->np) != hipSuccess) {
    snprintf(c->err, sizeof(c->err), "training set of %d triplets: device allocation failed", n);
    return GPC_E_HIP;
  }
  if (hipMemcpyAsync(d_aos.p, triplets, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return GPC_E_HIP;
  hipLaunchKernelGGL(gpc::k_ts_transpose, dim3((unsigned)(t->np / 64), 3, 3), dim3(TS_THREADS), 0, c->stream,
                     (const uint8_t*)d_aos.p, n, t->np, t->planes.p);
  if (hipMemsetAsync(t->flags.p, 0, (size_t)t->np, c->stream) != hipSuccess) return GPC_E_HIP;
  hipLaunchKernelGGL(gpc::k_ts_begin, dim3((unsigned)(t->np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream, t->flags.p, n,
                     t->np, 1);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return GPC_E_HIP;
  c->train_sets.push_back(t.get());
  *out = t.release();
  return GPC_OK;
}

int gpc_hip_train_set_destroy(gpc_hip_ctx* c, gpc_hip_train_set* t) {
  if (!c || !t || t->owner != c) return GPC_E_INVALID;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (size_t k = 0; k < c->train_sets.size(); ++k)
    if (c->train_sets[k] == t) { c->train_sets.erase(c->train_sets.begin() + k); break; }
  delete t;
  return GPC_OK;
}

int gpc_hip_train_set_size(const gpc_hip_train_set* t) { return t ? t->n : 0; }

int gpc_hip_train_set_marks(gpc_hip_ctx* c, gpc_hip_train_set* t, const uint8_t* marks_in, uint8_t* marks_out) {
  CHK(train_check(c, t));
  DevBlock<uint8_t> d_mem;  // (freed on every return)
  HIPCHK(c, d_mem.alloc((size_t)t->n));
  uint8_t* d_m = d_mem.p;
  const dim3 grid((unsigned)((t->n + TS_THREADS - 1) / TS_THREADS));
  int st = GPC_OK;
  if (marks_in) {
    if (hipMemcpyAsync(d_m, marks_in, (size_t)t->n, hipMemcpyHostToDevice, c->stream) != hipSuccess) st = GPC_E_HIP;
    hipLaunchKernelGGL(gpc::k_ts_set_marks, grid, dim3(TS_THREADS), 0, c->stream, t->flags.p, (const uint8_t*)d_m, t->n);
  }
  if (marks_out && st == GPC_OK) {
    hipLaunchKernelGGL(gpc::k_ts_get_marks, grid, dim3(TS_THREADS), 0, c->stream, (const uint8_t*)t->flags.p, d_m, t->n);
    if (hipMemcpyAsync(marks_out, d_m, (size_t)t->n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) st = GPC_E_HIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) st = GPC_E_HIP;
  if (st != GPC_OK) snprintf(c->err, sizeof(c->err), "training set marks: HIP copy failed");
  return st;
}

int gpc_hip_train_eval_split(gpc_hip_ctx* c, gpc_hip_train_set* t, const gpc_split* params, int score_until_level,
                             double w1, gpc_split_stats* stats) {
  CHK(train_check(c, t));
  if (!params || !stats || score_until_level < 0) return GPC_E_INVALID;
  const int np_ = score_until_level + 1;
  if (np_ > 64) return GPC_E_UNSUPPORTED;
  for (int l = 0; l < np_; ++l)
    if (!split_ok(params[l])) return GPC_E_INVALID;
  CHK(train_scratch(c, t, 4, 64));
  HIPCHK(c, hipMemcpyAsync(t->d_cand.p, params, sizeof(gpc_split) * np_, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(t->counts.p, 0, sizeof(int32_t) * 4, c->stream));
  hipLaunchKernelGGL((gpc::k_ts_eval_split<false>), dim3((unsigned)(t->np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream,
                     (const uint8_t*)t->planes.p, t->flags.p, t->n, t->np, (const gpc::GpcSplit*)t->d_cand.p, np_, t->counts.p);
  HIPCHK(c, hipGetLastError());
  int32_t h[4];
  HIPCHK(c, hipMemcpyAsync(h, t->counts.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  split_stats(h[0], h[1], h[2], h[3], w1, stats);
  return GPC_OK;
}

int gpc_hip_train_mark_split_samples(gpc_hip_ctx* c, gpc_hip_train_set* t, const gpc_split* params, int num_params) {
  CHK(train_check(c, t));
  if (num_params < 0 || (num_params > 0 && !params)) return GPC_E_INVALID;
  if (num_params > 64) return GPC_E_UNSUPPORTED;
  for (int l = 0; l < num_params; ++l)
    if (!split_ok(params[l])) return GPC_E_INVALID;
  CHK(train_scratch(c, t, 4, 64));
  if (num_params) HIPCHK(c, hipMemcpyAsync(t->d_cand.p, params, sizeof(gpc_split) * num_params, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL((gpc::k_ts_eval_split<true>), dim3((unsigned)(t->np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream,
                     (const uint8_t*)t->planes.p, t->flags.p, t->n, t->np, (const gpc::GpcSplit*)t->d_cand.p, num_params,
                     (int32_t*)nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // params may be freed by the caller
  return GPC_OK;
}

int gpc_hip_train_begin_fern(gpc_hip_ctx* c, gpc_hip_train_set* t, int reset_marks) {
  CHK(train_check(c, t));
  hipLaunchKernelGGL(gpc::k_ts_begin, dim3((unsigned)(t->np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream, t->flags.p, t->n,
                     t->np, reset_marks);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int gpc_hip_train_eval_level(gpc_hip_ctx* c, gpc_hip_train_set* t, const gpc_split* cand, int ncand, int taulo, int tauhi,
                             int32_t* tp, int32_t* fp, int32_t* tot) {
  CHK(train_check(c, t));
  const int ntau = tauhi - taulo;
  if (!cand || ncand <= 0 || !tp || !fp || !tot) return GPC_E_INVALID;
  if (ntau <= 0 || ntau > TS_MAXTAU) return GPC_E_UNSUPPORTED;
  for (int k = 0; k < ncand; ++k)
    if (!split_ok(cand[k])) return GPC_E_INVALID;
  const size_t nc = (size_t)ncand * ntau;
  CHK(train_scratch(c, t, 2 * nc + 1, (size_t)ncand));
  HIPCHK(c, hipMemcpyAsync(t->d_cand.p, cand, sizeof(gpc_split) * ncand, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(t->counts.p, 0, sizeof(int32_t) * (2 * nc + 1), c->stream));
  {
    Timed tm(c, KID_TRAIN_EVAL);
    // longest chunks that still leave >= 4096 workgroups (16 per CU); measured on 1 Mi triplets: 16 Ki-triplet
    // chunks stream 1000 candidates at 7.3 TB/s (4 Ki: 6.4), but starve a 10-candidate launch
    int iters = 64;
    while (iters > 4 && ((t->np + (long)iters * TS_ITER - 1) / ((long)iters * TS_ITER)) * ncand < 4096) iters >>= 1;
    const unsigned chunks = (unsigned)((t->np + (long)iters * TS_ITER - 1) / ((long)iters * TS_ITER));
    hipLaunchKernelGGL(gpc::k_ts_eval_level, dim3(chunks, ncand), dim3(TS_THREADS), 0,
                       c->stream, (const uint8_t*)t->planes.p, (const uint8_t*)t->flags.p, t->np,
                       (const gpc::GpcSplit*)t->d_cand.p, taulo, ntau, iters, t->counts.p, t->counts.p + nc);
  }
  hipLaunchKernelGGL(gpc::k_ts_tot, dim3((unsigned)((t->np / 4 + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0,
                     c->stream, (const uint8_t*)t->flags.p, t->np, t->counts.p + 2 * nc);
  HIPCHK(c, hipGetLastError());
  // one copy back: [tp | fp | tot] are contiguous on the device
  t->h_counts.resize(2 * nc + 1);
  HIPCHK(c, hipMemcpyAsync(t->h_counts.data(), t->counts.p, sizeof(int32_t) * (2 * nc + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(tp, t->h_counts.data(), sizeof(int32_t) * nc);
  memcpy(fp, t->h_counts.data() + nc, sizeof(int32_t) * nc);
  *tot = t->h_counts[2 * nc];
  return GPC_OK;
}

int gpc_hip_train_commit_level(gpc_hip_ctx* c, gpc_hip_train_set* t, const gpc_split* best, int mark_split) {
  CHK(train_check(c, t));
  if (!best || !split_ok(*best)) return GPC_E_INVALID;
  gpc::GpcSplit b = {best->i, best->j, best->tau};
  hipLaunchKernelGGL(gpc::k_ts_commit, dim3((unsigned)(t->np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream,
                     (const uint8_t*)t->planes.p, t->flags.p, t->n, t->np, b, mark_split);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int gpc_hip_train_fern(gpc_hip_ctx* c, gpc_hip_train_set* t, int max_depth, const gpc_split* cand, int num_resamples,
                       int taulo, int tauhi, int only_score_non_split, double w1, gpc_split* fernparams,
                       gpc_split_stats* level_stats) {
  CHK(train_check(c, t));
  if (max_depth <= 0 || !cand || num_resamples < 0 || !fernparams || !level_stats) return GPC_E_INVALID;
  if (max_depth > 64 || tauhi - taulo > TS_MAXTAU) return GPC_E_UNSUPPORTED;
  const int ntau = tauhi > taulo ? tauhi - taulo : 0;
  std::vector<int32_t> tp((size_t)num_resamples * ntau + 1), fp((size_t)num_resamples * ntau + 1);
  gpc_split_stats stats;
  memset(&stats, 0, sizeof stats);
  gpc_split best = {0, 0, 0};                       // SplitParams_t bestParams;            Fern.hpp:316
  for (int l = 0; l < max_depth; ++l) fernparams[l] = gpc_split{0, 0, 0};  // fernparams.resize(maxDepth)  :318
  CHK(gpc_hip_train_begin_fern(c, t, only_score_non_split));                // resetMarkOnSamples        :333
  for (int level = 0; level < max_depth; ++level) {
    int32_t tot = 0;
    if (num_resamples > 0 && ntau > 0)
      CHK(gpc_hip_train_eval_level(c, t, cand + (size_t)level * num_resamples, num_resamples, taulo, tauhi, tp.data(),
                                   fp.data(), &tot));
    select_level(cand + (size_t)level * num_resamples, num_resamples, taulo, ntau, tp.data(), fp.data(), tot, w1, &best,
                 &stats);
    fernparams[level] = best;                                               // :352 (also when nothing scored above 0)
    CHK(gpc_hip_train_commit_level(c, t, &best, only_score_non_split));     // markSplitSamples(level)    :355
    level_stats[level] = stats;                                             // what train() prints        :357
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GPC_OK;
}

// Forest::trainAndExport's loop over the ferns (training.hpp:113-135) without its copies: every fern's bootstrap is a
// multiplicity per triplet of the ONE resident set, and the ferns of a group advance level by level in the same launches
// (k_train_forest.h).  Per level the host reads the group's counts once, runs the reference's selection (select_level, as
// gpc_hip_train_fern does) and sends the winners back.  The per-fern state, the staging block and every other workspace
// are owners local to the call: released when it returns, whichever way.
int gpc_hip_train_forest(gpc_hip_ctx* c, gpc_hip_train_set* t, int nferns, int max_depth, const gpc_split* cand,
                         int num_resamples, int taulo, int tauhi, int only_score_non_split, double w1, const int32_t* draws,
                         int draws_per_fern, gpc_split* fernparams, gpc_split_stats* level_stats) {
  CHK(train_check(c, t));
  if (nferns <= 0 || max_depth <= 0 || !cand || num_resamples < 0 || !fernparams || !level_stats ||
      (draws && draws_per_fern <= 0))
    return GPC_E_INVALID;
  // (a fern's candidates of one level are one grid dimension)
  if (max_depth > 64 || tauhi - taulo > TS_MAXTAU || num_resamples > 65535) return GPC_E_UNSUPPORTED;
  const int ntau = tauhi > taulo ? tauhi - taulo : 0;
  const size_t per_fern = (size_t)max_depth * num_resamples;  // hyperplanes of one fern
  for (size_t k = 0; k < (size_t)nferns * per_fern; ++k)
    if (!split_ok(cand[k])) return GPC_E_INVALID;
  if (draws)
    for (size_t k = 0; k < (size_t)nferns * draws_per_fern; ++k)
      if (draws[k] < 0 || draws[k] >= t->n) return GPC_E_INVALID;
  for (size_t k = 0; k < (size_t)nferns * max_depth; ++k) fernparams[k] = gpc_split{0, 0, 0};  // fernparams.resize(maxDepth)
  memset(level_stats, 0, sizeof(gpc_split_stats) * (size_t)nferns * max_depth);
  if (num_resamples == 0 || ntau == 0) return GPC_OK;  // nothing is evaluated: Fern::train leaves zeros (Fern.hpp:316-357)

  const int n = t->n;
  const long np = t->np;
  // fern f's multiplicities m[np] and one past its last drawn triplet, rounded up to a lane's 4; false: more than 255 copies
  auto count = [&](int f, uint8_t* m, int32_t* lim) -> bool {
    if (!draws) {
      memset(m, 1, (size_t)n);
      memset(m + n, 0, (size_t)(np - n));
      *lim = (n + 3) & ~3;
      return true;
    }
    memset(m, 0, (size_t)np);
    const int32_t* d = draws + (size_t)f * draws_per_fern;
    int32_t hi = 0;
    for (int k = 0; k < draws_per_fern; ++k) {
      if (m[d[k]] == 255) return false;
      ++m[d[k]];
      if (d[k] > hi) hi = d[k];
    }
    *lim = (hi + 4) & ~3;
    return true;
  };
  auto too_many = [&]() {
    snprintf(c->err, sizeof(c->err), "gpc_hip_train_forest: one fern draws a triplet more than 255 times");
    return GPC_E_UNSUPPORTED;
  };

  // ferns per group: (fern, candidate) is one grid dimension; 1 GiB of flags and multiplicities, 256 MiB of counters at most
  const size_t nc = (size_t)num_resamples * ntau;
  size_t G = (size_t)nferns;
  G = std::min(G, (size_t)65535 / num_resamples);
  G = std::min(G, std::max<size_t>(1, ((size_t)1 << 29) / (size_t)np));
  G = std::min(G, std::max<size_t>(1, ((size_t)1 << 26) / (2 * nc + 1)));
  if (c->train_group > 0) G = std::min(G, (size_t)c->train_group);
  if (draws && G < (size_t)nferns) {  // several groups: nothing is launched before every fern's multiplicities are known to fit
    std::vector<uint8_t> m((size_t)np);
    int32_t lim;
    for (int f = 0; f < nferns; ++f)
      if (!count(f, m.data(), &lim)) return too_many();
  }

  // page-locked staging: [multiplicities G x np | hyperplanes G x per_fern | winners G | lim G | counters G x (2 nc + 1)]
  const size_t ncounts = G * (2 * nc + 1);
  const size_t o_cand = G * (size_t)np, o_best = o_cand + sizeof(gpc_split) * G * per_fern, o_lim = o_best + sizeof(gpc_split) * G,
               o_cnt = o_lim + sizeof(int32_t) * G;
  Pinned<uint8_t> h_mem;
  DevBlock<uint8_t> d_flags, d_mult;
  DevBlock<gpc::GpcSplit> d_cand;  // the group's hyperplanes of every level, then its winners of the current one
  DevBlock<int32_t> d_cnt;         // counters of the current level [tp | fp | tot], then lim
  HIPCHK(c, h_mem.alloc(o_cnt + sizeof(int32_t) * ncounts, hipHostMallocDefault));
  HIPCHK(c, d_flags.alloc(G * (size_t)np));
  HIPCHK(c, d_mult.alloc(G * (size_t)np));
  HIPCHK(c, d_cand.alloc(sizeof(gpc_split) * (G * per_fern + G)));
  HIPCHK(c, d_cnt.alloc(sizeof(int32_t) * (ncounts + G)));
  uint8_t* h_mult = h_mem.p;
  gpc_split* h_cand = reinterpret_cast<gpc_split*>(h_mem.p + o_cand);
  gpc_split* h_best = reinterpret_cast<gpc_split*>(h_mem.p + o_best);
  int32_t* h_lim = reinterpret_cast<int32_t*>(h_mem.p + o_lim);
  int32_t* h_cnt = reinterpret_cast<int32_t*>(h_mem.p + o_cnt);
  gpc::GpcSplit* d_best = d_cand.p + G * per_fern;
  int32_t* d_lim = d_cnt.p + ncounts;
  std::vector<gpc_split> best(G);
  std::vector<gpc_split_stats> stats(G);

  for (int f0 = 0; f0 < nferns; f0 += (int)G) {
    const int g = std::min((int)G, nferns - f0);
    long span = 0;  // triplets any fern of the group reads
    for (int f = 0; f < g; ++f) {
      if (!count(f0 + f, h_mult + (size_t)f * np, &h_lim[f])) return too_many();  // (one group: nothing launched yet)
      span = std::max(span, (long)h_lim[f]);
    }
    memcpy(h_cand, cand + (size_t)f0 * per_fern, sizeof(gpc_split) * g * per_fern);
    HIPCHK(c, hipMemcpyAsync(d_mult.p, h_mult, (size_t)g * np, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cand.p, h_cand, sizeof(gpc_split) * g * per_fern, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_lim, h_lim, sizeof(int32_t) * g, hipMemcpyHostToDevice, c->stream));
    {
      Timed tm(c, KID_TF_BEGIN);
      hipLaunchKernelGGL(gpc::k_tf_begin, dim3((unsigned)(np / TS_THREADS), g), dim3(TS_THREADS), 0, c->stream, d_flags.p, n, np);
    }
    for (int f = 0; f < g; ++f) {
      best[f] = gpc_split{0, 0, 0};                     // SplitParams_t bestParams;            Fern.hpp:316
      memset(&stats[f], 0, sizeof(gpc_split_stats));
    }
    const size_t gnc = (size_t)g * nc, gcounts = 2 * gnc + g;
    // chunk length as in gpc_hip_train_eval_level: the longest that still leaves >= 4096 workgroups
    int iters = 64;
    while (iters > 4 && ((span + (long)iters * TS_ITER - 1) / ((long)iters * TS_ITER)) * g * num_resamples < 4096) iters >>= 1;
    const unsigned chunks = (unsigned)((span + (long)iters * TS_ITER - 1) / ((long)iters * TS_ITER));
    for (int level = 0; level < max_depth; ++level) {
      HIPCHK(c, hipMemsetAsync(d_cnt.p, 0, sizeof(int32_t) * gcounts, c->stream));
      {
        Timed tm(c, KID_TF_EVAL);
        hipLaunchKernelGGL(gpc::k_tf_eval, dim3(chunks, (unsigned)(g * num_resamples)), dim3(TS_THREADS), 0, c->stream,
                           (const uint8_t*)t->planes.p, (const uint8_t*)d_flags.p, (const uint8_t*)d_mult.p,
                           (const int32_t*)d_lim, np, (const gpc::GpcSplit*)d_cand.p + (size_t)level * num_resamples,
                           (int)per_fern, num_resamples, taulo, ntau, iters, d_cnt.p, d_cnt.p + gnc);
      }
      {
        Timed tm(c, KID_TF_TOT);
        hipLaunchKernelGGL(gpc::k_tf_tot, dim3((unsigned)std::min<long>((span / 4 + TS_THREADS - 1) / TS_THREADS, 32), g), dim3(TS_THREADS), 0,
                           c->stream, (const uint8_t*)d_flags.p, (const uint8_t*)d_mult.p, (const int32_t*)d_lim, np,
                           d_cnt.p + 2 * gnc);
      }
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(h_cnt, d_cnt.p, sizeof(int32_t) * gcounts, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // the level's one read-back
      for (int f = 0; f < g; ++f) {
        select_level(h_cand + (size_t)f * per_fern + (size_t)level * num_resamples, num_resamples, taulo, ntau,
                     h_cnt + (size_t)f * nc, h_cnt + gnc + (size_t)f * nc, h_cnt[2 * gnc + f], w1, &best[f], &stats[f]);
        fernparams[(size_t)(f0 + f) * max_depth + level] = best[f];    // :352 (also when nothing scored above 0)
        level_stats[(size_t)(f0 + f) * max_depth + level] = stats[f];  // what train() prints        :357
        h_best[f] = best[f];
      }
      if (level + 1 == max_depth) break;  // (the marks of the bootstrap go with it: nothing reads the last level's)
      HIPCHK(c, hipMemcpyAsync(d_best, h_best, sizeof(gpc_split) * g, hipMemcpyHostToDevice, c->stream));
      {
        Timed tm(c, KID_TF_COMMIT);
        hipLaunchKernelGGL(gpc::k_tf_commit, dim3((unsigned)((span + TS_THREADS - 1) / TS_THREADS), g), dim3(TS_THREADS), 0,
                           c->stream, (const uint8_t*)t->planes.p, d_flags.p, (const uint8_t*)d_mult.p, (const int32_t*)d_lim, np,
                           (const gpc::GpcSplit*)d_best, only_score_non_split);
      }
      HIPCHK(c, hipGetLastError());
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GPC_OK;
}

// ------------------------------------------------------------------ training-set extraction

// Feature::extractAllTriplets (Feature.hpp:191-245) for a batch of frame pairs, straight into a device training set
// (k_extract.h).  The keep rule depends on the points alone, so the host decides which triplets stay and where each goes
// (column order[k] of kept triplet k, or k); the frames are smoothed chunk by chunk -- run_preprocess, the `smooth` output
// of preprocessImage in the context's arithmetic -- and each chunk's kernel gathers the patches of its own columns.
// The frames handed to the _device entry point must be device memory of the context's GPU, first byte and last: a host
// address (pageable memory, a CPU tensor) would make the kernels fault.
static bool on_this_device(const gpc_hip_ctx* c, const uint8_t* p, size_t bytes) {
  for (const uint8_t* q : {p, p + bytes - 1}) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // pageable host memory: not an error of this library
      return false;
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->device) return false;
  }
  return true;
}

static int extract_triplets(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, bool on_device, int W, int H, int nframes,
                            const gpc_triplet_points* pts, const int32_t* frame_first, const int32_t* order,
                            gpc_hip_train_set** out, int* n_kept) {
  if (out) *out = nullptr;
  if (n_kept) *n_kept = 0;
  if (!c || !rawL || !rawR || !frame_first || !out || !n_kept || nframes < 0) return GPC_E_INVALID;
  CHK(check_dims(W, H));
  if (frame_first[0] != 0) return GPC_E_INVALID;
  for (int f = 0; f < nframes; ++f)
    if (frame_first[f + 1] < frame_first[f]) return GPC_E_INVALID;
  const int total = frame_first[nframes];
  if (total > 0 && !pts) return GPC_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (on_device && nframes > 0) {
    const size_t bytes = (size_t)nframes * W * H;
    if (!on_this_device(c, rawL, bytes) || !on_this_device(c, rawR, bytes)) {
      snprintf(c->err, sizeof(c->err), "gpc_hip_extract_triplets_device: the frames are not device memory of device %d", c->device);
      return GPC_E_INVALID;
    }
  }
  // Feature.hpp:208-214: all three points more than 20 px inside the image
  auto inside = [W, H](int x, int y) { return x > 20 && y > 20 && x < W - 20 && y < H - 20; };
  std::vector<int32_t> kept, kept_frame;
  for (int f = 0; f < nframes; ++f)
    for (int k = frame_first[f]; k < frame_first[f + 1]; ++k) {
      const gpc_triplet_points& p = pts[k];
      if (inside(p.rx, p.ry) && inside(p.px, p.py) && inside(p.nx, p.ny)) {
        kept.push_back(k);
        kept_frame.push_back(f);
      }
    }
  const int n = (int)kept.size();
  std::vector<int32_t> col_src(n);  // column -> kept index
  if (order) {
    std::vector<uint8_t> seen(n, 0);
    for (int k = 0; k < n; ++k) {
      const int32_t o = order[k];
      if (o < 0 || o >= n || seen[o]) return GPC_E_INVALID;
      seen[o] = 1;
      col_src[o] = k;
    }
  } else {
    for (int k = 0; k < n; ++k) col_src[k] = k;
  }
  if (n == 0) return GPC_OK;

  // chunks of frame pairs: 64 MiB of smoothed frames by default (pixel offsets of a chunk stay below 2^31)
  const size_t npx = (size_t)W * H;
  int per_chunk = c->extract_frames;
  if (per_chunk <= 0) per_chunk = (int)std::max<size_t>(1, (size_t(64) << 20) / (2 * npx));
  per_chunk = (int)std::max<size_t>(1, std::min<size_t>(per_chunk, (size_t(1) << 31) / (2 * npx)));
  const int nchunks = (nframes + per_chunk - 1) / per_chunk;
  const long np = ((long)n + 255) / 256 * 256;
  // column groups per chunk: a group of four columns goes to every chunk one of its columns comes from; padding columns
  // (n .. np) are zeroed by whichever record holds them, groups of padding only by the chunk of the last triplet
  std::vector<std::vector<gpc::ExGroup>> work(nchunks);
  const int last_chunk = kept_frame[col_src[n - 1]] / per_chunk;
  for (long q = 0; q < np / 4; ++q) {
    int ch[4];
    for (int b = 0; b < 4; ++b) {
      const long col = 4 * q + b;
      ch[b] = col < n ? kept_frame[col_src[col]] / per_chunk : -1;
    }
    for (int b = 0; b < 4; ++b) {
      const int mine = ch[b] >= 0 ? ch[b] : (ch[0] < 0 && b == 0 ? last_chunk : -1);
      if (mine < 0) continue;
      bool first = true;  // one record per (group, chunk)
      for (int b2 = 0; b2 < b; ++b2)
        if (ch[b2] == ch[b] && ch[b] >= 0) first = false;
      if (!first) continue;
      gpc::ExGroup g;
      g.q = (int32_t)q;
      for (int b2 = 0; b2 < 4; ++b2) {
        const long col = 4 * q + b2;
        if (col >= n) {
          for (int p = 0; p < 3; ++p) g.off[4 * p + b2] = EX_ZERO;
        } else if (ch[b2] != mine) {
          for (int p = 0; p < 3; ++p) g.off[4 * p + b2] = EX_KEEP;
        } else {
          const int k = col_src[col];
          const gpc_triplet_points& t = pts[kept[k]];
          const long fl = kept_frame[k] - (long)mine * per_chunk;
          // smooth of the chunk: [frame][side][H][W]; top-left pixel of the 27x27 patch
          g.off[4 * 0 + b2] = (int32_t)(((2 * fl + 0) * H + t.ry - 13) * (long)W + t.rx - 13);
          g.off[4 * 1 + b2] = (int32_t)(((2 * fl + 1) * H + t.py - 13) * (long)W + t.px - 13);
          g.off[4 * 2 + b2] = (int32_t)(((2 * fl + 1) * H + t.ny - 13) * (long)W + t.nx - 13);
        }
      }
      work[mine].push_back(g);
    }
  }

  gpc_hip_train_set* t = new gpc_hip_train_set();
  t->owner = c;
  t->n = n;
  t->np = np;
  // the chunk workspaces (smoothed frames, the gradient image run_preprocess also writes, uploaded frames, column groups:
  // about 4 x 64 MiB at the default chunk size) are given back when the call ends; the page-locked transfer arena is the
  // context's, shared with the other host-buffer entry points, and stays
  auto release_ws = [c]() {
    (void)c->ext_raw.reset();
    (void)c->ext_smooth.reset();
    (void)c->ext_grad.reset();
    (void)c->ext_groups.reset();
  };
  auto fail = [&](int st) {
    (void)hipStreamSynchronize(c->stream);
    release_ws();
    delete t;
    return st;
  };
  if (t->planes.alloc((size_t)3 * TS_PATCH * np) != hipSuccess || t->flags.alloc((size_t)np) != hipSuccess) {
    snprintf(c->err, sizeof(c->err), "training set of %d triplets: device allocation failed", n);
    return fail(GPC_E_HIP);
  }
  const bool bits_before = c->grad_is_bits;  // (run_preprocess records what kind of gradient image c->grad holds)
  for (int ch = 0; ch < nchunks; ++ch) {
    const std::vector<gpc::ExGroup>& gl = work[ch];
    if (gl.empty()) continue;  // no triplet of these frames is kept: they are not even smoothed
    const int f0 = ch * per_chunk, nf = std::min(per_chunk, nframes - f0);
    const size_t side_bytes = npx * nf, group_bytes = pad16(sizeof(gpc::ExGroup) * gl.size());
    int st = GPC_OK;
    uint8_t* d_arena = nullptr;
    // the page-locked arena carries the chunk's column groups (and, from host memory, its frames): the previous chunk's
    // copies out of it must be done before it is written again
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(GPC_E_HIP);
    if ((st = xfer_reserve(c, group_bytes + (on_device ? 0 : 2 * side_bytes), &d_arena)) != GPC_OK) return fail(st);
    if ((st = ensure(c, c->ext_smooth, 2 * side_bytes)) != GPC_OK || (st = ensure(c, c->ext_grad, 2 * side_bytes)) != GPC_OK ||
        (st = ensure(c, c->ext_groups, group_bytes)) != GPC_OK)
      return fail(st);
    memcpy(c->h_xfer.p, gl.data(), sizeof(gpc::ExGroup) * gl.size());
    const uint8_t *d_L = rawL + f0 * npx, *d_R = rawR + f0 * npx;
    if (!on_device) {
      if ((st = ensure(c, c->ext_raw, 2 * side_bytes)) != GPC_OK) return fail(st);
      memcpy(c->h_xfer.p + group_bytes, rawL + f0 * npx, side_bytes);
      memcpy(c->h_xfer.p + group_bytes + side_bytes, rawR + f0 * npx, side_bytes);
      if ((st = dev_copy16(c, c->ext_raw.p, d_arena + group_bytes, 2 * side_bytes)) != GPC_OK) return fail(st);
      d_L = (const uint8_t*)c->ext_raw.p;
      d_R = d_L + side_bytes;
    }
    if ((st = dev_copy16(c, c->ext_groups.p, d_arena, group_bytes)) != GPC_OK) return fail(st);
    st = run_preprocess(c, d_L, d_R, W, H, nf, 2, 10, false, (uint8_t*)c->ext_smooth.p, (uint8_t*)c->ext_grad.p);
    c->grad_is_bits = bits_before;
    if (st != GPC_OK) return fail(st);
    const unsigned nblk = (unsigned)((gl.size() + EX_GROUPS - 1) / EX_GROUPS);
    hipLaunchKernelGGL(gpc::k_extract_gather, dim3(nblk, 3, 3), dim3(TS_THREADS), 0, c->stream, (const uint8_t*)c->ext_smooth.p, W,
                       (const gpc::ExGroup*)c->ext_groups.p, (int)gl.size(), np, t->planes.p);
    if (hipGetLastError() != hipSuccess) return fail(GPC_E_HIP);
  }
  if (hipMemsetAsync(t->flags.p, 0, (size_t)np, c->stream) != hipSuccess) return fail(GPC_E_HIP);
  hipLaunchKernelGGL(gpc::k_ts_begin, dim3((unsigned)(np / TS_THREADS)), dim3(TS_THREADS), 0, c->stream, t->flags.p, n, np, 1);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return fail(GPC_E_HIP);
  release_ws();
  c->train_sets.push_back(t);
  *out = t;
  *n_kept = n;
  return GPC_OK;
}

int gpc_hip_extract_triplets(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int nframes,
                             const gpc_triplet_points* pts, const int32_t* frame_first, const int32_t* order,
                             gpc_hip_train_set** out, int* n_kept) {
  return extract_triplets(c, rawL, rawR, false, W, H, nframes, pts, frame_first, order, out, n_kept);
}

int gpc_hip_extract_triplets_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int nframes,
                                    const gpc_triplet_points* pts, const int32_t* frame_first, const int32_t* order,
                                    gpc_hip_train_set** out, int* n_kept) {
  return extract_triplets(c, d_rawL, d_rawR, true, W, H, nframes, pts, frame_first, order, out, n_kept);
}

int gpc_hip_train_set_read(gpc_hip_ctx* c, gpc_hip_train_set* t, int first, int n, uint8_t* aos) {
  CHK(train_check(c, t));
  if (first < 0 || n < 0 || (long)first + n > t->n || (n > 0 && !aos)) return GPC_E_INVALID;
  const int step = 16384;  // triplets per pass through the page-locked arena (36 MB)
  for (int done = 0; done < n; done += step) {
    const int m = std::min(step, n - done);
    const size_t bytes = (size_t)m * 3 * TS_PATCH;
    uint8_t* d_arena = nullptr;
    CHK(xfer_reserve(c, bytes, &d_arena));
    hipLaunchKernelGGL(gpc::k_ts_read, dim3((unsigned)((m + 63) / 64), 3, 3), dim3(TS_THREADS), 0, c->stream, (const uint8_t*)t->planes.p,
                       t->np, first + done, m, d_arena);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(aos + (size_t)done * 3 * TS_PATCH, c->h_xfer.p, bytes);
  }
  return GPC_OK;
}

// ------------------------------------------------------------------ measurement

// Host-only test hook (tests/cpp/sanitize_host.cpp: AddressSanitizer / UBSan / ThreadSanitizer builds of this file run on
// the CPU, no device): the expansion pool exactly as gpc_hip_match_batch drives it -- `npairs` pairs of packed records back
// to back (pair i: counts[i] supports, cut at `cap`; rows[i * hpad + y] of them in row y), every pair split into `parts`
// row ranges, `threads` workers, landing slots rotating like the chunks' -- plus the copy jobs of the pageable path.
// Not part of the C ABI (include/gpc_hip.h does not declare it).
extern "C" int gpc_hip_debug_expand_pool(const uint32_t* packed, const int32_t* rows, int hpad, int H, int npairs,
                                         const int32_t* counts, int cap, int threads, int parts, gpc_support* out,
                                         const uint8_t* copy_src, uint8_t* copy_dst, size_t copy_bytes) {
  if (!packed || !rows || !counts || !out || threads < 1 || parts < 1 || H < 2 * GPC_R + 1) return GPC_E_INVALID;
  ExpandPool pool;
  pool.start(threads, nullptr);
  const uint32_t* recs = packed;
  for (int i = 0; i < npairs; ++i) {
    const int32_t* r = rows + (size_t)i * hpad;
    const long limit = counts[i] < cap ? counts[i] : cap;
    long first = 0;
    if ((i & 3) == 3) pool.wait_slot((i + 1) & 3);  // (a landing slot is reused only when its jobs are done)
    for (int q = 0; q < parts; ++q) {
      const int y0 = GPC_R + (int)((long)(H - 2 * GPC_R) * q / parts), y1 = GPC_R + (int)((long)(H - 2 * GPC_R) * (q + 1) / parts);
      if (first < limit && y1 > y0)
        pool.push(ExpandJob{recs, r, H, y0, y1, (int)first, (int)limit, out + (size_t)i * cap, i & 3});
      for (int y = y0; y < y1; ++y) first += r[y];
    }
    recs += limit;
  }
  if (copy_bytes) {
    const size_t step = (copy_bytes / (size_t)threads + 4095) & ~(size_t)4095;
    for (size_t at = 0; at < copy_bytes; at += step) {
      ExpandJob j = {};
      j.slot = 7;
      j.copy_src = copy_src + at;
      j.copy_dst = copy_dst + at;
      j.copy_bytes = at + step <= copy_bytes ? step : copy_bytes - at;
      pool.push(j);
    }
    pool.wait_slot(7);
  }
  pool.wait_all();
  pool.stop();
  return GPC_OK;
}

// Host-only test hook (tests/cpp/sanitize_host.cpp, sanitizer builds on the CPU; not part of the C ABI): the fingerprint the
// resident-image records are held against (sampled or every byte) and the overlap test that drops them.
extern "C" int gpc_hip_debug_fingerprint(const uint8_t* smooth, const uint8_t* grad, size_t n, const int32_t* mask, int n_mask,
                                         int full, uint64_t* fp, const void* a, size_t na, const void* b, size_t nb, int* overlap) {
  if (!smooth || !grad || !fp || n_mask < 0 || (n_mask > 0 && !mask)) return GPC_E_INVALID;
  *fp = fingerprint(smooth, grad, n, mask, n_mask, full != 0);
  if (overlap) *overlap = ranges_overlap(a, na, b, nb) ? 1 : 0;
  return GPC_OK;
}

// What the owners hold, over every context of the process (tests/test_gpu_resources.py): live device blocks, their bytes,
// live page-locked blocks, live streams + events.  What callers own through gpc_hip_host_alloc is not counted.
extern "C" int gpc_hip_debug_live_resources(uint64_t out[4]) {
  if (!out) return GPC_E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = g_live[i].load();
  return GPC_OK;
}

#ifdef GPC_WGLIFE
// diagnostic build only (tools/exp/join_wg_lives.py): per workgroup of the last k_row_join_fused launch start, end, rows | place
extern "C" int gpc_hip_debug_join_workgroups(gpc_hip_ctx* c, unsigned long long* out, int n_wg) {
  if (!c || !out || n_wg < 1 || n_wg > 4096) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(gpc::g_rjf_wg), 3 * sizeof(unsigned long long) * (size_t)n_wg));
  return GPC_OK;
}
#endif
#ifdef GPC_STAMPS
// diagnostic build only: read and clear the s_memtime phase sums of k_row_join
extern "C" int gpc_hip_debug_stamps(gpc_hip_ctx* c, unsigned long long* out16) {
  if (!c || !out16) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(gpc::g_rj_stamps), 16 * sizeof(unsigned long long)));
  unsigned long long zero[16] = {0};
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(gpc::g_rj_stamps), zero, sizeof zero));
  return GPC_OK;
}
// the same for the phases of k_hash
extern "C" int gpc_hip_debug_htjoin_stamps(gpc_hip_ctx* c, unsigned long long* out16) {
  if (!c || !out16) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(gpc::g_hj_stamps), 16 * sizeof(unsigned long long)));
  const unsigned long long zero[16] = {0};
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(gpc::g_hj_stamps), zero, sizeof zero));
  return GPC_OK;
}
// per workgroup of the last k_hash launches: start, end (s_memrealtime), HW_ID | XCC_ID << 32 (3 words each, 8192 workgroups)
extern "C" int gpc_hip_debug_hash_workgroups(gpc_hip_ctx* c, unsigned long long* out, int n_wg) {
  if (!c || !out || n_wg < 1 || n_wg > 8192) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(gpc::g_ht_wg), 3 * sizeof(unsigned long long) * (size_t)n_wg));
  return GPC_OK;
}
extern "C" int gpc_hip_debug_hash_stamps(gpc_hip_ctx* c, unsigned long long* out16) {
  if (!c || !out16) return GPC_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(gpc::g_ht_stamps), 16 * sizeof(unsigned long long)));
  unsigned long long zero[16] = {0};
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(gpc::g_ht_stamps), zero, sizeof zero));
  return GPC_OK;
}
#endif

int gpc_hip_enable_kernel_timing(gpc_hip_ctx* c, int enable) {
  if (!c) return GPC_E_INVALID;
  c->timing = enable != 0;
  return GPC_OK;
}

int gpc_hip_set_kernel_timing_mask(gpc_hip_ctx* c, unsigned mask) {
  if (!c) return GPC_E_INVALID;
  c->timing_mask = mask;
  return GPC_OK;
}

int gpc_hip_reset_kernel_timing(gpc_hip_ctx* c) {
  if (!c) return GPC_E_INVALID;
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto& s : c->spans) c->free_spans.push_back(std::move(s));
  c->spans.clear();
  return GPC_OK;
}

// the slots the 32-bit timing mask addresses; the slots behind them (gpc_hip_kernel_slots) are bracketed whenever timing is on
int gpc_hip_kernel_count(void) { return KID_COUNT < 32 ? KID_COUNT : 32; }

int gpc_hip_kernel_slots(void) { return KID_COUNT; }

const char* gpc_hip_kernel_name(int index) {
  return (index >= 0 && index < KID_COUNT) ? kKernelNames[index] : "";
}

const char* gpc_hip_kernel_launch_name(const gpc_hip_ctx* c, int index) {
  return (c && index >= 0 && index < KID_COUNT) ? c->launch_name[index] : "";
}

int gpc_hip_kernel_time(gpc_hip_ctx* c, int index, float* total_ms, int* launches) {
  if (!c || index < 0 || index >= KID_COUNT) return GPC_E_INVALID;
  CHK(drain_lanes(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float tot = 0.f;
  int cnt = 0;
  for (auto& s : c->spans) {
    if (s.kid != index) continue;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, s.a, s.b));
    tot += ms;
    ++cnt;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  return GPC_OK;
}

}  // extern "C"
