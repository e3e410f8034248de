/*
 * gpc_hip.h -- C ABI of libgpc_hip.so, the MI355X (gfx950) implementation of the
 * openGPC sparse-stereo hot path: preprocess (3x3 box, binary Sobel, candidate
 * mask) -> fern hash codes -> unique-code collision matching -> disparity filter.
 *
 * This is the drop-in boundary.  The reference has no FFI layer (header-only C++),
 * so each entry point names the reference function it stands in for; the C++ API
 * in include/gpc/inference.hpp forwards to these exactly where the reference's
 * Forest methods call the raw-pointer kernels of lib/gpc/filter.hpp.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns a gpc_status (0 = ok);
 *   - images are 8-bit, row-major, `width` a multiple of 16 (reference asserts this,
 *     filter.hpp:294,405,549), tightly packed (stride == width); width <= 16384 and
 *     width * height <= 2^30, larger images are refused with GPC_E_UNSUPPORTED (the reference
 *     has no such limit);
 *   - outputs are caller-allocated with an explicit capacity; the true count is
 *     always returned, GPC_E_CAPACITY if it did not fit (the first `cap` entries are
 *     valid);
 *   - a context belongs to one device and one host thread at a time (the reference's
 *     Forest is stateless and re-entrant; use one context per thread);
 *   - there is NO CPU fallback: without a usable gfx950 device gpc_hip_create fails.
 */
#ifndef GPC_HIP_H
#define GPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPC_HIP_ABI_VERSION 1
#define GPC_MAX_TESTS 32   /* readForest keeps the first 32 tests, inference.hpp:426 */
#define GPC_PATCH_RADIUS 13 /* 27x27 patch; also the candidate margin, inference.hpp:322 */

typedef enum {
  GPC_OK = 0,
  GPC_E_INVALID = 1,      /* bad argument (null pointer, width % 16, size mismatch)      */
  GPC_E_NO_DEVICE = 2,    /* no HIP device / not gfx950 / HIP runtime error at create    */
  GPC_E_HIP = 3,          /* a HIP call failed; see gpc_hip_last_error                   */
  GPC_E_CAPACITY = 4,     /* output did not fit; count returned is the true count        */
  GPC_E_NO_FOREST = 5,    /* match/hash called before gpc_hip_set_forest                 */
  GPC_E_FOREST_RANGE = 6, /* a test offset leaves the 27x27 patch                        */
  GPC_E_IO = 7,           /* forest file could not be opened / parsed                    */
  GPC_E_UNSUPPORTED = 8   /* a size / setting this build cannot honour (width > 16384, ...) */
} gpc_status;

/* == ndb::Support, lib/gpc/buffer.hpp:91-97 (12 bytes) */
typedef struct {
  int32_t x, y;
  float d;
} gpc_support;

/* == ndb::Correspondence, lib/gpc/buffer.hpp:99-102 (two ndb::Point) */
typedef struct {
  int32_t src_x, src_y, tar_x, tar_y;
} gpc_correspondence;

/* == gpc::inference::InferenceSettings, lib/gpc/inference.hpp:71-131 */
typedef struct {
  int32_t gradient_threshold; /* gradientThreshold_ (uint8_t), default 10 */
  int32_t disp_high;          /* dispHigh_, default 128                    */
  int32_t vertical_tolerance; /* verticalTolerance_, default 1             */
  int32_t epipolar_mode;      /* epipolarMode_, default 0                  */
  int32_t use_hashtable;      /* useHashtable_: 1 = ndb::Hashmatch matcher */
  int32_t num_threads;        /* numThreads_: accepted, ignored            */
} gpc_settings;

/* == gpc::inference::Forest::FilterMask, lib/gpc/inference.hpp:137-156 */
typedef struct {
  int32_t mask[2 * GPC_MAX_TESTS]; /* mask[2t]=ix+iy*width, mask[2t+1]=jx+jy*width */
  int32_t tau[GPC_MAX_TESTS];
  int32_t num_tests;
  int32_t type;      /* 0: all tau == 0 (gpcFilter), 1: gpcFilterTau */
  int32_t width, height;
  int32_t discarded; /* tests dropped beyond the 32nd                */
} gpc_filter_mask;

typedef struct gpc_hip_ctx gpc_hip_ctx;

/* ---- library / context ------------------------------------------------------ */
int gpc_hip_abi_version(void);
const char* gpc_hip_status_string(int status);
int gpc_hip_device_count(int* count);
/* Creates a context on `device` with its own HIP stream. */
int gpc_hip_create(int device, gpc_hip_ctx** ctx);
int gpc_hip_destroy(gpc_hip_ctx* ctx);
/* Last HIP error text of this context (static storage inside the context). */
const char* gpc_hip_last_error(const gpc_hip_ctx* ctx);
/* Borrow an externally owned hipStream_t (e.g. torch's current stream); NULL restores
 * the context's own stream.  The caller waits for the old stream before switching: work still in flight on it shares the
 * context's workspaces with whatever is queued on the new one, and nothing orders the two. */
int gpc_hip_set_stream(gpc_hip_ctx* ctx, void* hip_stream);
int gpc_hip_synchronize(gpc_hip_ctx* ctx);
/* Pre-size device workspaces for `max_pairs` pairs of width x height (optional; the
 * entry points below grow them on demand, which costs a hipMalloc + sync). */
int gpc_hip_reserve(gpc_hip_ctx* ctx, int width, int height, int max_pairs);

/* Pays, outside the caller's timed region, for everything a first call would otherwise pay inside it: the library's code
 * objects, the workspaces of one pair of width x height, page-locked staging, streams and worker threads.  The reference's
 * sample starts its clock after Forest::readForest(path, width, height) (samples/sparsematch.cpp:42-45) -- the one call
 * that knows the image size -- so the C++ API calls this from there; a C caller does it after gpc_hip_set_forest (the
 * forest must be set: GPC_E_NO_FOREST otherwise).  Runs the host entry points once on a synthetic pair and discards the
 * results.  settings == NULL: all four matcher modes (epipolar x hashtable). */
int gpc_hip_warmup(gpc_hip_ctx* ctx, int width, int height, const gpc_settings* settings);

/* The reference has two arithmetic variants chosen at BUILD time (samples/CMakeLists.txt:13-20):
 * SSE=ON (-D_INTRINSICS_SSE, the default and the parity target of this library) and SSE=OFF
 * (boxNaive / sobelNaive / gpcFilter(Tau)Naive, filter.hpp:157-282), which produce different
 * smooth images, masks and codes.  A context starts in GPC_ARITH_SSE. */
#define GPC_ARITH_SSE 0
#define GPC_ARITH_NAIVE 1
int gpc_hip_set_arithmetic(gpc_hip_ctx* ctx, int mode);

/* Page-locked host memory (hipHostMalloc) for the host-buffer entry points: with pageable
 * buffers the PCIe copies run at a fraction of the link rate.  Free with gpc_hip_host_free. */
int gpc_hip_host_alloc(gpc_hip_ctx* ctx, uint64_t bytes, void** ptr);
int gpc_hip_host_free(gpc_hip_ctx* ctx, void* ptr);

/* ---- forest ------------------------------------------------------------------ */
/* Forest::readForest (inference.hpp:404-446): parses the text forest for an image of
 * `width` x `height`.  Host only.  A missing file yields GPC_E_IO and an empty mask of
 * type 0, as the reference does. */
int gpc_hip_read_forest(const char* path, int width, int height, gpc_filter_mask* out);
int gpc_hip_parse_forest(const char* text, int width, int height, gpc_filter_mask* out);
/* Uploads the tests (what gpcFilter/gpcFilterTau receive as `fastmask`/`tau`,
 * filter.hpp:547,619).  Offsets are decoded back to (dx,dy) with |d| <= 13. */
int gpc_hip_set_forest(gpc_hip_ctx* ctx, const gpc_filter_mask* fm);

/* ---- all trees of a forest (group mode) ------------------------------------------ */
/* The forest's ferns, in file order, packed greedily into GROUPS of at most 32 tests: a group takes the next fern while
 * its test count stays <= 32; a fern of more than 32 tests is cut into chunks of 32 (the remainder last), each a group of
 * its own.  Group g equals what gpc_hip_read_forest returns for a file holding only group g's ferns (offsets for
 * `width`, type 1 iff one of the group's own taus is nonzero, discarded = 0).  groups[0 .. *n_groups) are written;
 * *n_groups is the true group count (GPC_E_CAPACITY if it exceeds cap).  More than GPC_MAX_GROUPS groups:
 * GPC_E_UNSUPPORTED.  Truncated or garbage text: GPC_E_IO, as gpc_hip_parse_forest.  Host only. */
#define GPC_MAX_GROUPS 32
int gpc_hip_read_forest_groups(const char* path, int width, int height, gpc_filter_mask* groups, int cap, int* n_groups);
int gpc_hip_parse_forest_groups(const char* text, int width, int height, gpc_filter_mask* groups, int cap, int* n_groups);
/* Enters group mode (n_groups == 1 behaves exactly like gpc_hip_set_forest(ctx, groups)); gpc_hip_set_forest leaves it.
 * Every group has the same width and height.  In group mode each group is matched as today's forest is (same arithmetic,
 * settings and disparity filter), and gpc_hip_match_pair (+ _begin / gpc_hip_match_fetch), gpc_hip_rectified_match,
 * gpc_hip_stereo_match (+ their _begin forms) and gpc_hip_match_batch_device return the UNION: group 0's records in
 * today's order, then group 1's records not equal to one already emitted, and so on (supports compared by (x, y, d),
 * correspondences by (src_x, src_y, tar_x, tar_y)).  A union holds up to n_groups * min(nL, nR) records: size outputs
 * for that or fetch again on GPC_E_CAPACITY.  Candidate counts are unchanged.
 * GPC_E_UNSUPPORTED in group mode: use_hashtable = 1, gpc_hip_match_batch, gpc_hip_match_batch_packed,
 * gpc_hip_match_batch_device_packed, gpc_hip_hash_codes, two lanes (gpc_hip_set_pipeline(ctx, 2)). */
int gpc_hip_set_forest_groups(gpc_hip_ctx* ctx, const gpc_filter_mask* groups, int n_groups);
/* Dense code images of every group of the current forest, codes[n_groups][height][width]: plane g holds what
 * gpc_hip_hash_codes gives for group g alone.  Outside group mode n_groups = 1 (the forest of gpc_hip_set_forest). */
int gpc_hip_hash_codes_groups(gpc_hip_ctx* ctx, const uint8_t* smooth, const uint8_t* grad, int width, int height,
                              uint32_t* codes);

/* ---- host-buffer entry points (drop-in for the Forest methods) ---------------- */
/* Forest::preprocessImage (inference.hpp:302-333): box + clearBoundary, sobel on the
 * raw image, ascending candidate indices with the 13-pixel margin.
 * smooth, grad: width*height bytes; mask: capacity mask_cap ints. */
int gpc_hip_preprocess(gpc_hip_ctx* ctx, const uint8_t* raw, int width, int height,
                       int gradient_threshold, uint8_t* smooth, uint8_t* grad,
                       int32_t* mask, int mask_cap, int* n_mask);
/* The same in two steps, so that the caller can allocate while the device works (the by-value PreprocessedImage of
 * Forest::preprocessImage, inference.hpp:161-165, 302-333): _begin QUEUES the kernels -- the device writes smooth, grad and
 * the candidate list into page-locked staging memory of the context over the link -- and returns; _fetch waits, copies the
 * three results into the caller's arrays with the library's worker threads (any may be NULL; the candidate count is
 * returned; GPC_E_CAPACITY if mask_cap is short, the first mask_cap indices are delivered).  An image has at most
 * (width - 26) * (height - 26) candidates.  Exactly one _fetch per _begin, no other call on the context in between.
 *
 * Resident images.  The image also STAYS on the device (the last two per context), and the arrays handed to _fetch (or to
 * gpc_hip_preprocess) are remembered as its host copies.  gpc_hip_rectified_match / gpc_hip_stereo_match recognise them --
 * same addresses, same sizes, same arithmetic mode, and a fingerprint of their contents (66 words spread over each array)
 * unchanged -- and then hash and match from the device copies instead of uploading smooth, grad and mask again: the
 * reference's by-value PreprocessedImage without its round trip over the link.  Anything else (copies of the arrays,
 * edited arrays, arrays from another context) takes the upload path; the results are the same either way.  A caller that
 * EDITS a delivered array in place in a way 66 samples can miss must set GPC_HIP_RESIDENT=2 (every byte is hashed) or
 * GPC_HIP_RESIDENT=0 (never resident).  Every library call that writes over a remembered array forgets it. */
int gpc_hip_preprocess_begin(gpc_hip_ctx* ctx, const uint8_t* raw, int width, int height, int gradient_threshold);
int gpc_hip_preprocess_fetch(gpc_hip_ctx* ctx, uint8_t* smooth, uint8_t* grad, int32_t* mask, int mask_cap, int* n_mask);
/* Match calls of this context served from resident images so far (tests, diagnostics). */
int gpc_hip_resident_hits(const gpc_hip_ctx* ctx);

/* ndb::gpcFilter / gpcFilterTau as called by evalFastMaskOnSubsetSSE
 * (inference.hpp:266-292): dense code image, width*height uint32, zero where the
 * reference leaves its zero-filled buffer untouched. */
int gpc_hip_hash_codes(gpc_hip_ctx* ctx, const uint8_t* smooth, const uint8_t* grad,
                       int width, int height, uint32_t* codes);
/* Forest::rectifiedMatch (inference.hpp:375-393) on already preprocessed images.
 * maskL/maskR are the candidate index lists of the PreprocessedImage. */
int gpc_hip_rectified_match(gpc_hip_ctx* ctx, const uint8_t* smoothL, const uint8_t* gradL,
                            const int32_t* maskL, int n_maskL, const uint8_t* smoothR,
                            const uint8_t* gradR, const int32_t* maskR, int n_maskR,
                            int width, int height, const gpc_settings* settings,
                            gpc_support* out, int cap, int* n_out);
/* Forest::stereoMatch (inference.hpp:344-361): correspondences, no disparity filter. */
int gpc_hip_stereo_match(gpc_hip_ctx* ctx, const uint8_t* smoothL, const uint8_t* gradL,
                         const int32_t* maskL, int n_maskL, const uint8_t* smoothR,
                         const uint8_t* gradR, const int32_t* maskR, int n_maskR,
                         int width, int height, const gpc_settings* settings,
                         gpc_correspondence* out, int cap, int* n_out);
/* The whole timed region of samples/sparsematch.cpp:45-52 for one pair:
 * preprocessImage x2 + rectifiedMatch, raw host images in, supports out. */
int gpc_hip_match_pair(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR,
                       int width, int height, const gpc_settings* settings,
                       gpc_support* out, int cap, int* n_out, int* n_cand_l, int* n_cand_r);

/* The three calls above in two steps each: *_begin queues the work and returns (the results go to page-locked memory of
 * the context), gpc_hip_match_fetch waits and copies min(count, cap) records into `out` (gpc_support for the rectified and
 * pair forms, gpc_correspondence for the stereo form) with the library's worker threads; *n_out is the true count
 * (GPC_E_CAPACITY when it exceeds cap: fetch again with a larger array -- the results stay until the next call on the
 * context).  n_cand_l / n_cand_r are filled after gpc_hip_match_pair_begin only.  Between the two steps the caller can
 * allocate (and let the allocator zero) the array the results go to: that is what a std::vector<ndb::Support> of the
 * reference's API costs, and here it runs beside the kernels instead of after them. */
int gpc_hip_rectified_match_begin(gpc_hip_ctx* ctx, const uint8_t* smoothL, const uint8_t* gradL,
                                  const int32_t* maskL, int n_maskL, const uint8_t* smoothR,
                                  const uint8_t* gradR, const int32_t* maskR, int n_maskR,
                                  int width, int height, const gpc_settings* settings);
int gpc_hip_stereo_match_begin(gpc_hip_ctx* ctx, const uint8_t* smoothL, const uint8_t* gradL,
                               const int32_t* maskL, int n_maskL, const uint8_t* smoothR,
                               const uint8_t* gradR, const int32_t* maskR, int n_maskR,
                               int width, int height, const gpc_settings* settings);
int gpc_hip_match_pair_begin(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR,
                             int width, int height, const gpc_settings* settings);
int gpc_hip_match_fetch(gpc_hip_ctx* ctx, void* out, int cap, int* n_out, int* n_cand_l, int* n_cand_r);

/* ---- device-resident batch entry points ------------------------------------- */
/* `npairs` raw pairs already in HBM ([npairs][height][width] each side) -> supports in
 * HBM: d_out[npairs][cap_per_pair], d_counts[npairs] (true counts), and, if non-NULL,
 * d_ncand[npairs][2] candidate counts.
 * With the reference's sparsematch settings (epipolar_mode = 1, use_hashtable = 0) the call is
 * ASYNCHRONOUS on the context's stream: three launches are queued and it returns.
 * With epipolar_mode = 0 or use_hashtable = 1 (the device-wide matchers) the HOST WAITS once inside the
 * call (the hash-table matcher once per planning attempt): those matchers partition the records by code /
 * bucket range and read a few words back to learn whether every partition fits a workgroup (if not -- heavily
 * repeated codes -- the whole batch takes the radix-sort path instead).  The wait is for an event in the middle
 * of what the call queues, not for the stream; part of their work runs on a second stream of the context that
 * is joined back into the context's stream before the call returns.  In either case the outputs may be read
 * only after gpc_hip_synchronize (or another wait on the stream).
 * The join that writes the supports (three launches: the last one) places a row behind the rows before it with a
 * bounded wait on other workgroups; a wait that ran out (not observed so far) makes the kernel store the number of
 * that launch into a host-visible word, and the outputs of that launch must not be used.  The word is examined by
 * gpc_hip_synchronize and by every entry point that synchronises itself (they return GPC_E_HIP, gpc_hip_last_error
 * names the launch), and -- for callers that gave the context their own stream and wait on it themselves -- at the
 * top of the NEXT call that queues such a join and in gpc_hip_destroy (which then returns GPC_E_HIP after freeing
 * everything): such callers should call gpc_hip_synchronize once before trusting a batch they did not wait for
 * through this library.
 * A pair with more than cap_per_pair records: the call still returns GPC_OK (the counts stay on the device, the host
 * never sees them); d_counts holds the true count, the pair's first cap_per_pair records are valid and nothing is written
 * behind them -- compare d_counts with cap_per_pair after the wait. */
int gpc_hip_match_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR,
                               int width, int height, int npairs, const gpc_settings* settings,
                               gpc_support* d_out, int cap_per_pair, int32_t* d_counts,
                               int32_t* d_ncand);
/* A STREAM of batches (the same context called again and again): with two lanes, consecutive gpc_hip_match_batch_device
 * calls (epipolar sort-matcher) alternate between two sets of workspaces on two streams of the context's own, and batch
 * k+1's preprocess and hash kernels run beside batch k's join (measured: 0.905 instead of 0.945 ms per 256 pairs).  In
 * this mode
 *   - a call's inputs are what the context's stream has produced when the call is made;
 *   - a call's outputs are complete after gpc_hip_synchronize, or -- for a caller that waits on a stream of its own
 *     (gpc_hip_set_stream) -- after that stream has passed gpc_hip_pipeline_join, which makes it wait for every call
 *     queued so far;
 *   - two calls are in flight at a time: consecutive calls need distinct output arrays.
 * lanes = 1 (the default) is the strict form above: everything on the context's stream, call by call. */
int gpc_hip_set_pipeline(gpc_hip_ctx* ctx, int lanes);
int gpc_hip_pipeline_join(gpc_hip_ctx* ctx);
/* Same from/to host memory (pinned or pageable), synchronous.  With the reference's sparsematch settings
 * (epipolar mode, sort matcher) the results cross PCIe packed (4 bytes per support, see below) and are expanded
 * into `out` by worker threads of the library while later chunks are still on the link: settings->num_threads > 1
 * asks for that many workers, otherwise the CPUs the process may use minus two.  The records delivered are
 * bit-identical to the device path's. */
int gpc_hip_match_batch(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR,
                        int width, int height, int npairs, const gpc_settings* settings,
                        gpc_support* out, int cap_per_pair, int32_t* counts, int32_t* ncand);

/* Host threads gpc_hip_match_batch last used to expand packed results (0 before the first such call).  Default:
 * settings->num_threads if > 1, else the CPUs this process may use -- divided by LOCAL_WORLD_SIZE when a launcher
 * starts one process per GPU -- less the feeding thread, between 2 and 8. */
int gpc_hip_host_threads(const gpc_hip_ctx* ctx);
/* Where the last gpc_hip_match_batch / gpc_hip_match_batch_packed call of the context spent its time: the host's clock,
 * in ms since the call's entry, when it saw [0] the last chunk's upload complete, [1] the last chunk's kernels done (its
 * counts arrived), [2] the last chunk of packed records landed in host memory, [3] the expansion / delivery done (the
 * call returned).  All 0 for calls that took another path (one or two pairs written directly, the device-wide matchers). */
int gpc_hip_batch_stages(const gpc_hip_ctx* ctx, float* ms4);
/* The launch plan of the context's most recent k_hash launch: out = {tile height in rows (32 or 40), tiles a workgroup
 * walks, workgroups per tile column (the grid's y), the flat workgroup index the launch's last round starts at}.  Host
 * values recorded when the launch was queued: the call does not synchronise.  GPC_E_INVALID before the first launch. */
int gpc_hip_hash_plan(gpc_hip_ctx* ctx, int32_t out[4]);
/* The CPU each worker thread last ran a job on, or started on if it has run none yet (returns the number of workers;
 * fills at most cap entries). */
int gpc_hip_host_worker_cpus(gpc_hip_ctx* ctx, int* cpus, int cap);
/* Batch calls of this context that ran their chunk pipeline on a thread bound to the GPU's NUMA node because the caller's
 * thread was on another socket (GPC_HIP_NO_FEEDER=1: never). */
int gpc_hip_fed_calls(const gpc_hip_ctx* ctx);
/* The NUMA node of the host this context's GPU hangs off (the expansion workers are bound to its CPUs), -1 if unknown. */
int gpc_hip_host_numa_node(const gpc_hip_ctx* ctx);

/* ---- frame sequences (optical flow) ------------------------------------------ */
/* Forest::stereoMatch of every consecutive pair (f[t], f[t+1]) of a frame sequence already in HBM ([nframes][height][width]);
 * d_out[nframes-1][cap_per_pair], d_counts[nframes-1] true counts, d_ncand[nframes] (optional) candidates per FRAME.
 * Record t is what stereoMatch(preprocessImage(f[t]), preprocessImage(f[t+1]), fm, settings) returns, in its order, for
 * every matcher (epipolar_mode 0 / 1 x use_hashtable 0 / 1) and either arithmetic.  Every frame is preprocessed and hashed
 * once: one k_preprocess and one k_hash launch over the nframes images, the joins read pair t's images at frames t, t + 1.
 * Waiting is as for gpc_hip_match_batch_device: with epipolar_mode = 1 and use_hashtable = 0 the call only queues work on
 * the context's stream; the device-wide matchers (epipolar_mode = 0 or use_hashtable = 1) wait on the host once inside
 * the call.  The outputs may be read after gpc_hip_synchronize (or another wait on the stream).
 * A pair with more than cap_per_pair records: true counts, each pair's first cap_per_pair records valid, nothing written
 * behind them; the device form returns GPC_OK as gpc_hip_match_batch_device does (compare d_counts with cap_per_pair after
 * the wait), the host form below GPC_E_CAPACITY.
 * nframes < 2, null pointers or a bad size: GPC_E_INVALID; no forest: GPC_E_NO_FOREST; group mode (ngroups > 1):
 * GPC_E_UNSUPPORTED.  With two lanes (gpc_hip_set_pipeline(ctx, 2)) the lanes are drained and the call runs on the
 * context's stream. */
int gpc_hip_match_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                  const gpc_settings* settings, gpc_correspondence* d_out, int cap_per_pair,
                                  int32_t* d_counts, int32_t* d_ncand);
/* The same from / to host memory (pageable or page-locked), synchronous.  The frames go through the device in chunks of
 * at most 16 frames (15 pairs); consecutive chunks share one frame, which is uploaded, preprocessed and hashed again in
 * the next chunk (1/15 more of that work for long sequences).  While chunk k is matched, chunk k+1 is uploaded on a
 * stream of its own.  Pageable frames pass through the context's page-locked arena: a _begin call still pending on the
 * context is waited for first and then ended, as every later call on the context ends it (its _fetch returns
 * GPC_E_INVALID).  ncand[nframes] is optional. */
int gpc_hip_match_sequence(gpc_hip_ctx* ctx, const uint8_t* frames, int width, int height, int nframes,
                           const gpc_settings* settings, gpc_correspondence* out, int cap_per_pair,
                           int32_t* counts, int32_t* ncand);

/* ---- packed results ------------------------------------------------------------ */
/* Forest::rectifiedMatch (inference.hpp:375-393) in epipolar mode emits supports row by row, so a support
 * {x, y, float(x - xR)} (ndb::Support, buffer.hpp:91-97) is fully described by one 32-bit word x | xR << 16 plus
 * the number of supports per row: 4 bytes instead of 12.  d_packed[npairs][cap_per_pair] receives the words in
 * the reference's output order, d_rows[npairs][height] the per-row counts (rows outside 13 .. height-14 are not
 * written), d_counts[npairs] the true totals.  Epipolar sort-matcher only (GPC_E_UNSUPPORTED otherwise).
 * Asynchronous on the context's stream. */
int gpc_hip_match_batch_device_packed(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR,
                                      int width, int height, int npairs, const gpc_settings* settings,
                                      uint32_t* d_packed, int cap_per_pair, int32_t* d_rows,
                                      int32_t* d_counts, int32_t* d_ncand);
/* The same from / to HOST memory, synchronous (the chunk pipeline of gpc_hip_match_batch without its last stage): the
 * records stay as they crossed the link -- packed[npairs][cap_per_pair] words, rows[npairs][height] per-row counts (rows
 * outside 13 .. height-14 hold 0), counts[npairs] the true totals (GPC_E_CAPACITY when one exceeds cap_per_pair; the pair's
 * first cap_per_pair records are delivered).  For callers that consume supports row by row, or that expand them later /
 * elsewhere with gpc_hip_expand_packed: a batch of 256 pairs of 1024x436 leaves 209 MB in host memory where the
 * ndb::Support arrays of gpc_hip_match_batch are 625 MB -- with one process per GPU on an 8-GPU node those 12-byte records
 * are what the host's memory bandwidth runs out on.  Epipolar sort-matcher only (GPC_E_UNSUPPORTED otherwise). */
int gpc_hip_match_batch_packed(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR, int width, int height,
                               int npairs, const gpc_settings* settings, uint32_t* packed, int cap_per_pair,
                               int32_t* rows, int32_t* counts, int32_t* ncand);
/* Host only: the first n supports of one pair from its packed words and row counts. */
int gpc_hip_expand_packed(const uint32_t* packed, const int32_t* rows, int height, int n, gpc_support* out);

/* ---- fern training: the scoring loop -------------------------- */
/* Replaces Fern::evalSplit (Fern.hpp:209-262), Fern::markSplitSamples (Fern.hpp:271-291) and the
 * level / resample / tau loops of Fern::train (Fern.hpp:312-372) over a device-resident training
 * set.  A triplet is three 27x27 byte patches (ref, pos, neg), 729 bytes each in the byte order of
 * Feature::storeAllTriplets (Feature.hpp:247-256); a test is (i, j, tau) with i, j linear indices
 * into a patch (Feature::params, Feature.hpp:84-89; Feature::getDecisions, Feature.hpp:101-109).
 * Marks: one byte per triplet, bit 0 = pos.split, bit 1 = neg.split (GPCDescriptor::split).
 * Hyperplane SAMPLING stays with the caller (Feature::sampleHyperplane draws from std::mt19937);
 * these entry points score what was drawn. */
typedef struct gpc_hip_train_set gpc_hip_train_set;
typedef struct gpc_split {
  int32_t i, j, tau;
} gpc_split;
typedef struct gpc_split_stats { /* splitStats, Fern.hpp:52-68 */
  double prec, rec, hmean, convcomb;
  int32_t tp, fp, fn, tot;
} gpc_split_stats;

/* Uploads `n` triplets (n * 3 * 729 bytes of host memory) and lays them out for the device.
 * All marks start cleared.  The set belongs to `ctx` and is destroyed with it at the latest. */
int gpc_hip_train_set_create(gpc_hip_ctx* ctx, const uint8_t* triplets, int n, gpc_hip_train_set** out);
int gpc_hip_train_set_destroy(gpc_hip_ctx* ctx, gpc_hip_train_set* set);
int gpc_hip_train_set_size(const gpc_hip_train_set* set);
/* marks_in != NULL: replace the marks; marks_out != NULL: read them back (after the replacement) */
int gpc_hip_train_set_marks(gpc_hip_ctx* ctx, gpc_hip_train_set* set, const uint8_t* marks_in, uint8_t* marks_out);
/* Fern::evalSplit over params[0 .. score_until_level] (at most 64 levels: the reference's code
 * words have 64 bits).  w1 = OptimizerSettings::w1_. */
int gpc_hip_train_eval_split(gpc_hip_ctx* ctx, gpc_hip_train_set* set, const gpc_split* params,
                             int score_until_level, double w1, gpc_split_stats* stats);
/* Fern::markSplitSamples over params[0 .. num_params) */
int gpc_hip_train_mark_split_samples(gpc_hip_ctx* ctx, gpc_hip_train_set* set, const gpc_split* params,
                                     int num_params);
/* Fern::train for one fern with the hyperplane samples supplied by the caller:
 * cand[level * num_resamples + k] is the k-th draw of sampleHyperplane at `level` (its tau is
 * ignored: the loop over [taulo, tauhi) overwrites it, Fern.hpp:341-342).  Keeps the reference's
 * selection rule (first candidate whose hmean exceeds the float maximum so far; a level on which
 * nothing scores above 0 inherits the previous level's parameters) and returns per level the
 * parameters chosen and the statistics train() prints (those of the LAST candidate evaluated).
 * max_depth <= 64, tauhi - taulo <= 64. */
int gpc_hip_train_fern(gpc_hip_ctx* ctx, gpc_hip_train_set* set, int max_depth, const gpc_split* cand,
                       int num_resamples, int taulo, int tauhi, int only_score_non_split, double w1,
                       gpc_split* fernparams, gpc_split_stats* level_stats);
/* One level of the above in pieces, for callers that sample adaptively: begin a fern, score
 * `ncand` candidates of the current level for every tau in [taulo, tauhi) (tp/fp: [ncand][ntau],
 * fn = *tot - tp - fp), then fix the level's winner. */
int gpc_hip_train_begin_fern(gpc_hip_ctx* ctx, gpc_hip_train_set* set, int reset_marks);
int gpc_hip_train_eval_level(gpc_hip_ctx* ctx, gpc_hip_train_set* set, const gpc_split* cand, int ncand,
                             int taulo, int tauhi, int32_t* tp, int32_t* fp, int32_t* tot);
int gpc_hip_train_commit_level(gpc_hip_ctx* ctx, gpc_hip_train_set* set, const gpc_split* best, int mark_split);
/* Forest::trainAndExport's loop over the ferns (training.hpp:113-135) over ONE resident set, without a copy of any triplet:
 *   cand    [nferns][max_depth][num_resamples]: cand[(f * max_depth + level) * num_resamples + k] is fern f's k-th draw of
 *           sampleHyperplane at `level` (its tau is ignored, as in gpc_hip_train_fern);
 *   draws   [nferns][draws_per_fern]: draws[f * draws_per_fern + d] is the index into `set` of fern f's d-th bootstrap draw
 *           (repeats are the point; draws_per_fern may exceed the set's size).  NULL: every fern trains on the whole set,
 *           each triplet once;
 *   fernparams, level_stats   [nferns][max_depth].
 * Fern f's output is exactly what gpc_hip_train_fern returns for a training set that holds the triplets set[draws[f][0]],
 * set[draws[f][1]], ... with all marks cleared -- what trainAndExport + Fern::train compute on their subSample: tp, fp, fn
 * and tot are sums over the draws, a triplet drawn m times counts m times.  The set's own marks are neither read nor
 * changed (the reference's bootstraps are copies it throws away).  On the device a bootstrap is one byte of multiplicity
 * and one byte of flags per triplet and fern; all ferns advance level by level in the same launches, in groups where
 * nferns * num_resamples or the workspaces ask for it, and the host reads one block of counts per level and group.
 * GPC_E_INVALID, before anything is launched: null pointers (draws excepted), nferns <= 0, max_depth <= 0, num_resamples < 0,
 * draws_per_fern <= 0 with draws, a draw outside [0, size), a hyperplane outside the patch.  GPC_E_UNSUPPORTED, before
 * anything is launched: max_depth > 64, tauhi - taulo > 64, num_resamples > 65535, and a fern that draws one triplet more
 * than 255 times (up to 255 the counts are exact; no count ever wraps).  With num_resamples == 0 or tauhi <= taulo nothing
 * is evaluated and the outputs are zeros, as Fern::train leaves them.  Every workspace is released before the call returns.
 * Synchronous. */
int gpc_hip_train_forest(gpc_hip_ctx* ctx, gpc_hip_train_set* set, int nferns, int max_depth, const gpc_split* cand,
                         int num_resamples, int taulo, int tauhi, int only_score_non_split, double w1,
                         const int32_t* draws, int draws_per_fern, gpc_split* fernparams, gpc_split_stats* level_stats);

/* ---- training-set extraction ---------------------------------------------------- */
/* One triplet of keypoints: the reference point in the LEFT frame, the positive and the negative point in the RIGHT
 * frame (the kptsL / kptsR / kptsN lists of SintelOpticalFlow.hpp:487-489 and SintelStereo.hpp:396-398). */
typedef struct gpc_triplet_points {
  int32_t rx, ry, px, py, nx, ny;
} gpc_triplet_points;

/* Feature::extractAllTriplets (Feature.hpp:191-245) for `nframes` frame pairs, straight into a device training set.
 *   rawL, rawR   [nframes][height][width] raw 8-bit frames (host memory here, HBM for the _device form);
 *   pts          the triplets of all frames back to back, frame f's at [frame_first[f], frame_first[f + 1]);
 *   frame_first  nframes + 1 ascending offsets, frame_first[0] = 0.
 * Smoothing is the `smooth` output of preprocessImage (3x3 box + clearBoundary, inference.hpp:306-313) in the context's
 * arithmetic (gpc_hip_set_arithmetic).  A triplet is KEPT when all three points satisfy x > 20 && y > 20 && x < width-20
 * && y < height-20 (Feature.hpp:208-214); kept triplets are numbered in frame order, then point order.  Patch bytes are
 * those of getPatch(.., x, y, 27) (buffer.hpp:534-544): byte 27 * ix + iy = pixel (x + ix - 13, y + iy - 13).
 * order == NULL: kept triplet k becomes triplet k of the set; otherwise it becomes triplet order[k], and `order` must be a
 * permutation of 0 .. n_kept-1 -- how a caller applies the reference's final std::random_shuffle (SintelOpticalFlow.hpp:160,
 * SintelStereo.hpp:152) without a host copy of the set.
 * The result is an ordinary training set with all marks cleared (every gpc_hip_train_* call takes it); *n_kept = its size.
 * Nothing kept: GPC_OK, *n_kept = 0, *out = NULL.  GPC_E_INVALID for null pointers, width % 16, descending frame_first and
 * an order that is not a permutation (which must hold n_kept entries: the caller computes n_kept with the keep rule
 * above).  The frames are processed in chunks (64 MiB of smoothed frames by default), so the
 * device workspace stays bounded however many frames there are.  Synchronous. */
int gpc_hip_extract_triplets(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR, int width, int height,
                             int nframes, const gpc_triplet_points* pts, const int32_t* frame_first,
                             const int32_t* order, gpc_hip_train_set** out, int* n_kept);
/* The same with rawL / rawR in HBM ([nframes][height][width] each); pts, frame_first and order stay in host memory.
 * Frames that are not device memory of the context's GPU (checked at their first and last byte) are refused with
 * GPC_E_INVALID before anything is launched.  The chunk workspaces of both forms are released before the call returns. */
int gpc_hip_extract_triplets_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                    int nframes, const gpc_triplet_points* pts, const int32_t* frame_first,
                                    const int32_t* order, gpc_hip_train_set** out, int* n_kept);
/* The inverse of gpc_hip_train_set_create's layout: triplets [first, first + n) of the set into `aos`, n * 3 * 729 bytes in
 * the byte order of Feature::storeAllTriplets (Feature.hpp:254-263).  Synchronous. */
int gpc_hip_train_set_read(gpc_hip_ctx* ctx, gpc_hip_train_set* set, int first, int n, uint8_t* aos);

/* ---- scoring against ground truth ------------------------------------------------ */
/* How good a result is, as exact counts per pair: the share of the records that lie within a few pixels of ground truth
 * (precision = n_within[k] / n_judged) and the share of the matchable pixels that were found (recall = n_within[k] /
 * n_matchable) -- the pair of figures the Global Patch Collider is evaluated by and Fern.hpp's trainer optimises.  Records,
 * candidate images and truth stay in HBM; a handful of integers per pair come back.  The library returns counts only. */
#define GPC_SCORE_MAX_THR 8
typedef struct gpc_truth {          /* device pointers (host pointers in the host forms), one entry per pair */
  const float*   u;                 /* [P][H][W]  stereo: disparity g >= 0, true right x = x - g.  flow: du    */
  const float*   v;                 /* [P][H][W]  flow: dv.  Must be NULL for supports                          */
  const uint8_t* ignore;            /* [P][H][W]  nonzero = do not judge this source pixel.  May be NULL        */
} gpc_truth;
typedef struct gpc_score {          /* one per pair; every field an exact count */
  int64_t n_records;                /* records looked at: min(count, cap)                                       */
  int64_t n_ignored;                /* source pixel set in `ignore`                                             */
  int64_t n_no_truth;               /* not ignored, truth not finite or |u| or |v| >= 1e9 (.flo "unknown")      */
  int64_t n_judged;                 /* the rest: n_records == n_ignored + n_no_truth + n_judged                 */
  int64_t n_within[GPC_SCORE_MAX_THR]; /* judged records with e2 <= thr[k]^2; entries >= n_thr are 0            */
  int64_t sum_e2_q8;                /* sum over judged records of (int64)(min(e2, 1048576.f) * 256.f + 0.5f);    */
                                    /* min is fminf: an e2 that is NaN or +inf contributes the clamp, 2^28       */
  int64_t n_candidates;             /* match-and-score forms: candidates of the left image (frame t); else 0    */
  int64_t n_matchable;              /* match-and-score forms: see below; else 0                                 */
} gpc_score;
/* The error of a record, in float32 with one rounding per operation (no fused multiply-add):
 *   correspondence (sx, sy, tx, ty), truth (u, v) read at (sx, sy):
 *     ex = float(tx - sx) - u; ey = float(ty - sy) - v; e2 = fl(fl(ex * ex) + fl(ey * ey));
 *   support (x, y, d), truth g read at (x, y): ex = d - g; e2 = fl(ex * ex);
 *   n_within[k] counts e2 <= fl(thr[k] * thr[k]).
 * A judged record whose own values make e2 NaN or +inf (a support with d = NaN or +-inf) stays judged, is within no
 * threshold, and adds the clamp to sum_e2_q8.
 * thr: n_thr floats, 1 <= n_thr <= GPC_SCORE_MAX_THR, each finite and >= 0 (GPC_E_INVALID otherwise).  A record whose
 * source pixel lies outside the image is invalid input; nothing is read for it and it counts as n_no_truth.
 * n_matchable counts the left candidates (x, y) that are not ignored, whose truth is usable, whose true target --
 * (x - R(g), y) for stereo, (x + R(u), y + R(v)) for flow, R = roundf, half away from zero -- lies inside the candidate
 * margin [13, W-13) x [13, H-13) and is itself a candidate of the right image (frame t + 1).  A candidate is what
 * gpc_hip_preprocess lists: gradient set, inside the margin.
 *
 * Records the caller already holds on the device, in the layout gpc_hip_match_batch_device / gpc_hip_match_sequence_device
 * write them: d_records[npairs][cap_per_pair], d_counts[npairs] true counts (may exceed cap_per_pair: min(count, cap) are
 * read).  Pure functions of their arguments: no forest is needed, d_counts is read on the device, and the calls only queue
 * work on the context's stream (read d_scores[npairs], which they overwrite, after gpc_hip_synchronize or another wait on
 * the stream).  Supports take truth->v == NULL, correspondences need truth->v. */
int gpc_hip_score_supports_device(gpc_hip_ctx* ctx, const gpc_support* d_supports, int cap_per_pair, const int32_t* d_counts,
                                  int width, int height, int npairs, const gpc_truth* truth, const float* thr, int n_thr,
                                  gpc_score* d_scores);
int gpc_hip_score_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_corr, int cap_per_pair,
                                         const int32_t* d_counts, int width, int height, int npairs, const gpc_truth* truth,
                                         const float* thr, int n_thr, gpc_score* d_scores);
/* Match and score: gpc_hip_match_batch_device with the records kept in a workspace of the context that holds every record
 * of every pair ((width - 26) * (height - 26) + 1 per pair, n_groups times that in group mode), then scored; n_candidates
 * and n_matchable are filled from the candidate images the pipeline left on the device.  Every setting and arithmetic
 * gpc_hip_match_batch_device takes is taken, group mode with the sort matchers included, and what it refuses is refused
 * with the same status.  Waiting is as for gpc_hip_match_batch_device.  With two lanes (gpc_hip_set_pipeline(ctx, 2)) the
 * lanes are drained and the call runs on the context's stream.
 * Alignment: the matchable pass reads four pixels of a plane at a time, so truth->u (and truth->v) must be 16-byte
 * aligned and truth->ignore 4-byte aligned (GPC_E_INVALID otherwise; width % 16 == 0 keeps every pair's plane aligned).
 * The records forms above have no such requirement. */
int gpc_hip_score_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                               int npairs, const gpc_settings* settings, const gpc_truth* truth, const float* thr, int n_thr,
                               gpc_score* d_scores);
/* The same over gpc_hip_match_sequence_device: pair t is frames t and t + 1, truth and d_scores have nframes - 1 entries,
 * correspondences are scored (truth->v is needed).  Group mode: GPC_E_UNSUPPORTED, as for the sequence itself. */
int gpc_hip_score_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                  const gpc_settings* settings, const gpc_truth* truth, const float* thr, int n_thr,
                                  gpc_score* d_scores);
/* Host records [npairs][cap_per_pair], host counts, host truth and host scores through the records forms; synchronous, in
 * chunks of at most 16 pairs through the context's page-locked arena where the arrays are pageable.  No forest needed. */
int gpc_hip_score_supports(gpc_hip_ctx* ctx, const gpc_support* supports, int cap_per_pair, const int32_t* counts, int width,
                           int height, int npairs, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores);
int gpc_hip_score_correspondences(gpc_hip_ctx* ctx, const gpc_correspondence* corr, int cap_per_pair, const int32_t* counts,
                                  int width, int height, int npairs, const gpc_truth* truth, const float* thr, int n_thr,
                                  gpc_score* scores);
/* Host images, host truth, host scores; synchronous.  The pairs (frames) pass through the device forms in chunks of at
 * most 16 -- truth is 8 to 9 bytes per pixel -- through the context's page-locked arena where the arrays are pageable (a
 * _begin call still pending on the context is waited for and ended, as gpc_hip_match_sequence does); consecutive chunks
 * of a sequence share one frame.  The scores equal the device forms' byte for byte. */
int gpc_hip_score_batch(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR, int width, int height, int npairs,
                        const gpc_settings* settings, const gpc_truth* truth, const float* thr, int n_thr, gpc_score* scores);
int gpc_hip_score_sequence(gpc_hip_ctx* ctx, const uint8_t* frames, int width, int height, int nframes,
                           const gpc_settings* settings, const gpc_truth* truth, const float* thr, int n_thr,
                           gpc_score* scores);

/* ---- point tracks over a frame sequence ------------------------------------------- */
/* Which match of pair t + 1 continues which match of pair t: the records of gpc_hip_match_sequence[_device] chained into
 * tracks on the device, so that a video user (structure from motion, stabilisation, long-range evaluation) gets a point's
 * positions over the frames instead of independent lists in code order.  The reference has no counterpart: it matches
 * one pair (Forest::stereoMatch, inference.hpp:344-361) and leaves every use of two results to its caller.  The rule is
 * therefore this library's own; it is made of integers only, so that every implementation of it gives the same bytes.
 *
 * Input: P = npairs lists corr[t][0 .. m_t), m_t = min(counts[t], cap_per_pair) (a negative count reads as 0), for frames
 * of width x height.  A pixel's index is y * width + x.  A record whose source or target lies outside
 * [0, width) x [0, height) takes no part: it is nobody's successor candidate and has none, so it is a track of length 1.
 *   Successor candidate of record i of pair t < P - 1: J = the lowest j < m_{t+1} (among the records that take part) whose
 *     source pixel equals i's target pixel; none if there is no such j.
 *   Link: among the records of pair t with the same J the lowest i gets next[t][i] = J, the others -1; next[P-1][.] = -1.
 *     "Lowest" because the matchers emit a pair's records in a fixed order, so the lowest index is the one choice that
 *     does not depend on which thread arrives first; the sort matchers emit every source and every target pixel at most
 *     once per pair, so for their records the rule never has to choose -- it matters for the hash-table matcher and for
 *     records a caller supplies.  Every record has at most one successor and one predecessor: the links form chains.
 *   Tracks: a head is a record without a predecessor.  Heads are numbered 0, 1, ... by (t ascending, i ascending); that
 *     number is track_id[t][i] of every record on the head's chain.  Row k of the table describes track k.
 * next and track_id are [npairs][cap_per_pair] like the records; entries at i >= m_t are left untouched.  *n_tracks is
 * the true number of tracks; the first min(*n_tracks, track_cap) rows of `tracks` are written (track_cap = 0: `tracks`
 * may be NULL).  npairs * cap_per_pair must not exceed 2^31 - 1, cap_per_pair and width * height 2^30 and npairs 65535
 * (GPC_E_UNSUPPORTED). */
typedef struct gpc_track {
  int32_t first_pair;   /* the head's pair: the point is seen in frames first_pair .. first_pair + length        */
  int32_t first_record; /* the head's index in corr[first_pair]                                                 */
  int32_t length;       /* records on the chain, >= 1                                                           */
  int32_t last_record;  /* index of the chain's last record, in corr[first_pair + length - 1]                   */
} gpc_track;
/* Records already on the device in the layout gpc_hip_match_sequence_device writes.  No forest is needed; d_counts is read
 * on the device, and the call only queues work on the context's stream (six launches: fill the per-pixel planes, scatter
 * the record indices, link, settle shared successors and count heads, scan, walk the chains); read the outputs after
 * gpc_hip_synchronize or another wait on the stream.  Workspaces of the context, grown on demand: 4 bytes per pixel for
 * each of the pairs 1 .. P-1, 4 bytes per record slot. */
int gpc_hip_track_records_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_corr, int cap_per_pair, const int32_t* d_counts,
                                 int width, int height, int npairs, int32_t* d_next, int32_t* d_track_id, gpc_track* d_tracks,
                                 int track_cap, int32_t* d_ntracks);
/* gpc_hip_match_sequence_device exactly as it is (every matcher setting, either arithmetic; its outputs d_corr, d_counts,
 * d_ncand as it documents them, its waiting too), then the links over what it wrote.  Group mode: GPC_E_UNSUPPORTED, as
 * for the sequence itself; no forest: GPC_E_NO_FOREST. */
int gpc_hip_track_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                  const gpc_settings* settings, gpc_correspondence* d_corr, int cap_per_pair, int32_t* d_counts,
                                  int32_t* d_ncand, int32_t* d_next, int32_t* d_track_id, gpc_track* d_tracks, int track_cap,
                                  int32_t* d_ntracks);
/* The same from / to host memory (pageable or page-locked), synchronous.  GPC_E_CAPACITY when a pair's count exceeds
 * cap_per_pair or *n_tracks exceeds track_cap; what is written is then as defined above (the first cap_per_pair records of
 * a pair are the ones linked).  gpc_hip_track_records needs no forest and sends each pair's first m_t records only. */
int gpc_hip_track_records(gpc_hip_ctx* ctx, const gpc_correspondence* corr, int cap_per_pair, const int32_t* counts, int width,
                          int height, int npairs, int32_t* next, int32_t* track_id, gpc_track* tracks, int track_cap,
                          int32_t* n_tracks);
/* Frames in, records (corr, counts, ncand[nframes] optional: as gpc_hip_match_sequence) and their tracks out.  A track may
 * run through every frame, so the sequence is not cut into chunks: all of it is staged on the device and the device form
 * runs once (pageable frames pass through the page-locked arena, as in gpc_hip_match_sequence, with the same effect on a
 * pending _begin).  The call is therefore BOUNDED BY DEVICE MEMORY: it holds
 *   nframes * W * H  +  (nframes - 1) * cap_per_pair * 24  +  track_cap * 16   bytes of staging (16 per record slot, 4
 *   for its link, 4 for its track id; the counts and the padding of each block to 16 bytes are not counted),
 *   (nframes - 2) * W * H * 4  +  (nframes - 1) * cap_per_pair * 4              bytes of linking workspace (plus 4 bytes
 *   per 2048 record slots for the head counts), and
 *   what gpc_hip_match_sequence_device keeps for nframes frames (smoothed image, gradient image and codes: 6 bytes per
 *   pixel and frame, plus the chosen matcher's own workspaces).  Longer videos, and videos without a known end: a track
 *   stream (gpc_hip_track_stream_*, below), which takes the frames in pushes and gives the same ids. */
int gpc_hip_track_sequence(gpc_hip_ctx* ctx, const uint8_t* frames, int width, int height, int nframes,
                           const gpc_settings* settings, gpc_correspondence* corr, int cap_per_pair, int32_t* counts,
                           int32_t* ncand, int32_t* next, int32_t* track_id, gpc_track* tracks, int track_cap, int32_t* n_tracks);

/* ---- track streams: frames pushed as they arrive, tracks kept alive across calls ------ */
/* The tracks above for a video that arrives one frame or a few frames at a time and has no known end.  A stream belongs
 * to a context and carries what linking the next pair needs; nothing in it grows with the length of the video except the
 * track table, whose size is fixed at creation.  The linking rule makes this exact: whether record (t, i) is a head
 * depends on pairs t - 1 and t alone, and heads are numbered by (t ascending, i ascending), so ids can be handed out as
 * pairs arrive.  AFTER ANY SEQUENCE OF PUSHES, EVERYTHING DELIVERED SO FAR IS BYTE-IDENTICAL TO WHAT THE OFFLINE CALL
 * (gpc_hip_track_sequence_device, gpc_hip_track_records_device) OVER THE CONCATENATED FRAMES OR RECORDS RETURNS.
 *
 * Pair numbering: pairs are numbered globally since create or reset; pair g joins frames g and g + 1.
 * A push that produces k pairs fills slots 0 .. k-1 of its outputs, each [k][cap_per_pair] like the offline arrays:
 *   corr, counts   as gpc_hip_match_sequence_device documents them;
 *   ncand          (optional) [nframes]: the candidates of each frame OF THIS PUSH, so that the pushes' arrays laid end to
 *                  end are the offline ncand;
 *   track_id[p][i] the offline track_id of that record;
 *   prev[p][i]     the index, in the preceding global pair, of the record whose offline `next` equals i, or -1.  prev
 *                  replaces next because a pair's next is not known until the following push; prev is its exact inverse
 *                  and is known at once.  For global pair 0 every prev is -1.
 *   Entries at i >= m_t are left untouched.
 * Track table: gpc_track rows with first_pair as a GLOBAL pair index, track_cap of them, in the stream.  New heads write
 *   their row; a continued track has length and last_record updated by the one record that continues it.  Rows with
 *   id >= track_cap are neither written nor updated; ids are still assigned.  The running total is a device word.  After
 *   every push the table and the total equal the offline result over the pairs pushed so far.
 * Id bound: track ids are 31 bits.  The stream keeps a host-side upper bound on the total, += k * min(cap_per_pair,
 *   width * height) per push; a push that could pass 2^31 - 1 returns GPC_E_UNSUPPORTED and changes nothing.  The calls
 *   that read the true total back (the host push, _state, _read_tracks) tighten the bound to it.  The limits of the offline
 *   form apply to ONE push: k <= 65535 (65534 once a pair is carried: the window holds it too) and k * cap_per_pair <=
 *   2^31 - 1.
 *
 * A push yields nframes pairs once a frame has been seen, else nframes - 1; a first push of one frame yields 0 pairs and
 * is valid.  Waiting is as for gpc_hip_match_sequence_device: the epipolar sort matcher only queues on the context's
 * stream, the device-wide matchers wait once on the host inside the call.  A stream is fed EITHER frames OR records
 * between resets: mixing them is GPC_E_INVALID.  Refusals (the stream is left as it was): group mode GPC_E_UNSUPPORTED;
 * no forest (frames) GPC_E_NO_FOREST; nframes < 1, null pointers, no settings at creation (frames), a destroyed stream or
 * a stream of another context GPC_E_INVALID; a forest or arithmetic of the context that CHANGED since the stream's last
 * push of frames (gpc_hip_set_forest* with other tests, gpc_hip_set_arithmetic with another mode: the carried codes are
 * then meaningless) GPC_E_INVALID until _reset.  A pair with more than cap_per_pair records: the stream advances, the
 * first cap_per_pair records are the ones linked, as offline, and the host push returns GPC_E_CAPACITY.
 * The stream owns everything it carries: any other call on the context between two pushes (batches of another size,
 * sequences, offline tracks, consensus, another stream) leaves what it returns unchanged.  With two lanes the lanes are
 * drained, as for sequences.
 *
 * Device memory of a stream (cap = cap_per_pair):
 *   cap * 20  +  max(track_cap, 1) * 16  +  16               bytes from creation (the carried pair's records and ids, the
 *                                                            table, the carried count and the total), and
 *   width * height * 4  +  16                                bytes from the first push of frames (the last frame's code
 *                                                            image and statistics words; smoothed and gradient images are
 *                                                            not carried), plus width * height under Naive arithmetic
 *                                                            with a 32-test forest (the candidate bytes the joins read);
 *   (k + 1) * cap * 4                                        bytes of link workspace of the largest push so far.
 * The context's own workspaces serve a push as they serve the offline calls: 4 * width * height + 4 * cap bytes per pair of
 * the push (planes and predecessors), 4 bytes per 2048 record slots, and what gpc_hip_match_sequence_device keeps for
 * nframes + 1 frames. */
typedef struct gpc_hip_track_stream gpc_hip_track_stream;
/* settings: copied; NULL for a stream that will only be given records.  width, height: the frames' (the records form
 * takes any positive size, as gpc_hip_track_records_device does; the frames form needs what the matchers need). */
int gpc_hip_track_stream_create(gpc_hip_ctx* ctx, int width, int height, const gpc_settings* settings, int cap_per_pair,
                                int track_cap, gpc_hip_track_stream** out);
/* Waits for the context's stream.  gpc_hip_destroy destroys the streams that are left. */
int gpc_hip_track_stream_destroy(gpc_hip_ctx* ctx, gpc_hip_track_stream* s);
/* A new video: frames forgotten, ids restart at 0, the table's rows count as unwritten. */
int gpc_hip_track_stream_reset(gpc_hip_ctx* ctx, gpc_hip_track_stream* s);
/* nframes frames in HBM.  *npairs = k, known when the call returns; the arrays after a wait on the context's stream. */
int gpc_hip_track_stream_push_device(gpc_hip_ctx* ctx, gpc_hip_track_stream* s, const uint8_t* d_frames, int nframes,
                                     gpc_correspondence* d_corr, int32_t* d_counts, int32_t* d_ncand, int32_t* d_prev,
                                     int32_t* d_track_id, int* npairs);
/* The same from / to host memory (pageable or page-locked), synchronous; *n_tracks is the total so far.  GPC_E_CAPACITY
 * when a pair's count exceeds cap_per_pair (a table that is too small shows in *n_tracks > track_cap). */
int gpc_hip_track_stream_push(gpc_hip_ctx* ctx, gpc_hip_track_stream* s, const uint8_t* frames, int nframes,
                              gpc_correspondence* corr, int32_t* counts, int32_t* ncand, int32_t* prev, int32_t* track_id,
                              int* npairs, int32_t* n_tracks);
/* npairs >= 1 pairs of records on the device in the layout gpc_hip_match_sequence_device writes.  No forest is needed;
 * the call only queues work on the context's stream. */
int gpc_hip_track_stream_push_records_device(gpc_hip_ctx* ctx, gpc_hip_track_stream* s, const gpc_correspondence* d_corr,
                                             const int32_t* d_counts, int npairs, int32_t* d_prev, int32_t* d_track_id);
/* Waits for the context's stream.  Every output is optional. */
int gpc_hip_track_stream_state(gpc_hip_ctx* ctx, gpc_hip_track_stream* s, int* frames_seen, int* pairs_seen, int32_t* n_tracks);
/* The table and the total as device pointers, valid until _destroy; read them behind the context's stream. */
int gpc_hip_track_stream_table(gpc_hip_track_stream* s, const gpc_track** d_tracks, const int32_t** d_ntracks);
/* Rows [first, first + n) to host memory, synchronous; rows at *n_tracks and beyond do not exist yet and are not written.
 * first + n > track_cap: GPC_E_CAPACITY (*n_tracks is still delivered). */
int gpc_hip_track_stream_read_tracks(gpc_hip_ctx* ctx, gpc_hip_track_stream* s, int first, int n, gpc_track* out,
                                     int32_t* n_tracks);

/* ---- match filtering: grid motion consensus ---------------------------------------- */
/* Rejects the matches their neighbours do not agree with: grid-based motion statistics (GMS, Bian et al., CVPR 2017) -- a
 * true match is surrounded by matches that move the same way, a false one is not.  The matchers emit every unique-code
 * collision; this is the filter a user of a sparse matcher applies next, and its output is again a record list in the
 * library's layout, so gpc_hip_score_*_device and gpc_hip_track_records_device take it unchanged.  The reference has no
 * counterpart (it matches one pair and leaves the rest to its caller): the rule is this library's own, and it is made of
 * integers only, so that every implementation of it gives the same bytes.
 *
 * Input: P = npairs lists rec[t][0 .. m_t), m_t = min(max(counts[t], 0), cap_per_pair), for images of width x height.
 *   Source and target: (src_x, src_y) -> (tar_x, tar_y) of a correspondence; (x, y) -> (x - (int)d, y) of a support.
 *   A record PARTICIPATES iff source and target lie in [0, width) x [0, height); a support must also have d finite,
 *     d == truncf(d) and |d| < 2^24.  A record that does not participate has keep mask 0 and is counted nowhere.
 *   Grid s in {0, 1, 2, 3} has the offset (ox, oy) = (0, 0), (c/2, 0), (0, c/2), (c/2, c/2), c = cell; shifts = 1 uses
 *     grid 0 only.  The cell of a point is ((x + ox) div c, (y + oy) div c); the grid has gx = (width - 1 + ox) div c + 1
 *     columns and gy = (height - 1 + oy) div c + 1 rows.  The displacement class of a record under grid s is the integer
 *     vector D = cell(target) - cell(source).
 *   For record i with source cell A under grid s, over the participating records j of the same pair:
 *     T_i = the number of j whose source cell lies within Chebyshev distance 1 of A;
 *     S_i = the number of those with D_j == D_i (i itself included);
 *     k_i = the number of grid cells within Chebyshev distance 1 of A (9 inside, fewer at the border, 1 in a 1x1 grid).
 *   i passes under grid s iff S_i * S_i * k_i * alpha_den^2 > alpha_num^2 * T_i (unsigned 64-bit, strict): GMS's
 *     S > alpha * sqrt(T / k) without the square root.
 * Output: keep[t][i] (uint8) has bit s set for every grid i passes under; a record is kept iff keep != 0.  The kept
 * records go to out[t][0 ..] in input order, index[t][n] is the input index of the n-th kept record, out_counts[t] the true
 * number kept; the first min(out_counts[t], cap_out) entries are written.  Entries of keep at i >= m_t and of out / index
 * beyond what is written are left untouched.  keep and index may be NULL.
 * GPC_E_UNSUPPORTED: cap_per_pair > 2^23 (what keeps the products exact: 2^46 * 9 * 2^12 < 2^63),
 * ceil(width / c) * ceil(height / c) > 2^22, npairs > 65535, npairs * cap_per_pair > 2^31 - 1.  GPC_E_INVALID: parameters
 * out of range, null required pointers, npairs < 1, cap_per_pair or cap_out < 1, `out` overlapping the input records.
 * The documented defaults are cell 16, shifts 4, alpha 6 / 1 (GMS's alpha and its shifted grids). */
typedef struct gpc_consensus {
  int32_t cell;       /* cell edge in pixels: even, 4 <= cell <= 256                         */
  int32_t shifts;     /* 1 or 4: grids tried                                                  */
  int32_t alpha_num;  /* 0 <= alpha_num <= 1024                                               */
  int32_t alpha_den;  /* 1 <= alpha_den <= 64;  threshold factor alpha = alpha_num/alpha_den  */
} gpc_consensus;
/* Records already on the device, in the layout the matchers write: d_rec[npairs][cap_per_pair], d_counts[npairs] (read on
 * the device), d_keep[npairs][cap_per_pair], d_out and d_index [npairs][cap_out], d_out_counts[npairs].  Pure functions
 * of their arguments: no forest is needed, and the calls only queue work on the context's stream (per grid: histogram of
 * the source cells, scan, counting sort, count and test; then chunk counts, scan, ordered write); read the outputs after
 * gpc_hip_synchronize or another wait on the stream.  Workspaces of the context, grown on demand: 8 bytes per record slot
 * (9 without d_keep), 8 bytes per pair and grid cell. */
int gpc_hip_consensus_supports_device(gpc_hip_ctx* ctx, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts,
                                      int width, int height, int npairs, const gpc_consensus* prm, uint8_t* d_keep,
                                      gpc_support* d_out, int cap_out, int32_t* d_index, int32_t* d_out_counts);
int gpc_hip_consensus_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_rec, int cap_per_pair,
                                             const int32_t* d_counts, int width, int height, int npairs,
                                             const gpc_consensus* prm, uint8_t* d_keep, gpc_correspondence* d_out, int cap_out,
                                             int32_t* d_index, int32_t* d_out_counts);
/* Match and filter: gpc_hip_match_batch_device / gpc_hip_match_sequence_device exactly as they are, into the workspace
 * of the context that holds every record of every pair (the one gpc_hip_score_batch_device uses), then the filter over
 * it.  Settings, refusals, statuses and waiting are those of the match they wrap; with two lanes
 * (gpc_hip_set_pipeline(ctx, 2)) the lanes are drained and the call runs on the context's stream.  d_raw_counts[P]
 * (optional) receives the unfiltered counts, d_ncand (optional) the candidate counts as the match writes them ([P][2] for
 * the batch, [nframes] for the sequence).  Group mode: the batch form filters the union; the sequence form is
 * GPC_E_UNSUPPORTED, as the sequence itself.  The limits above apply with cap_per_pair = that workspace's capacity,
 * n_groups * (width - 26) * (height - 26) + 1: a call whose every-record capacity exceeds 2^23 (an image of more than
 * about 8.3 million inner pixels, or a group-mode forest on a large one) is GPC_E_UNSUPPORTED here although the match
 * alone would run -- match into an array of the caller's and use the records form with the capacity it needs. */
int gpc_hip_consensus_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                   int npairs, const gpc_settings* settings, const gpc_consensus* prm, gpc_support* d_out,
                                   int cap_out, int32_t* d_out_counts, int32_t* d_raw_counts, int32_t* d_ncand);
int gpc_hip_consensus_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                      const gpc_settings* settings, const gpc_consensus* prm, gpc_correspondence* d_out,
                                      int cap_out, int32_t* d_out_counts, int32_t* d_raw_counts, int32_t* d_ncand);
/* Host records, counts and outputs through the records forms; synchronous, in chunks of at most 16 pairs, pageable arrays
 * through the context's page-locked arena.  Each pair's first m_t records travel; what comes back equals the device forms
 * byte for byte, untouched entries included.  GPC_E_CAPACITY when a pair's kept count exceeds cap_out (out_counts holds
 * the true counts, the first cap_out kept records of such a pair are delivered). */
int gpc_hip_consensus_supports(gpc_hip_ctx* ctx, const gpc_support* rec, int cap_per_pair, const int32_t* counts, int width,
                               int height, int npairs, const gpc_consensus* prm, uint8_t* keep, gpc_support* out, int cap_out,
                               int32_t* index, int32_t* out_counts);
int gpc_hip_consensus_correspondences(gpc_hip_ctx* ctx, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts,
                                      int width, int height, int npairs, const gpc_consensus* prm, uint8_t* keep,
                                      gpc_correspondence* out, int cap_out, int32_t* index, int32_t* out_counts);

/* ---- match refinement: sub-pixel position and photometric cost ------------------------ */
/* A unique-code collision says which pixel matches, not how well or where between pixels.  These calls compare the image
 * windows around the two ends of every match: the sum of absolute differences is the match's cost (a confidence), and the
 * costs at the neighbouring target positions give a parabola whose minimum is the sub-pixel position.  The reference has no
 * counterpart: the rule is this library's own, made of integers only, so every implementation of it gives the same bytes.
 * In a chain refinement comes after the consensus filter (which needs whole d) and before scoring.
 *
 * Input: P = npairs lists rec[t][0 .. m_t), m_t = min(max(counts[t], 0), cap_per_pair); 8-bit images imgL[P][height][width]
 *   and imgR[P][height][width] (whatever the caller passes, raw or smoothed; the sequence form uses frames t and t + 1 of one
 *   [nframes][height][width] array); a radius r, 1 <= r <= 6.  Any width, height >= 1.
 *   Source and target as in the consensus filter: (src_x, src_y) -> (tar_x, tar_y) of a correspondence; (x, y) ->
 *     (x - (int)d, y) of a support, whose d must be finite, d == truncf(d) and |d| < 2^24, or the record is not evaluated.
 *   cost(sx, sy) = sum over |i| <= r, |j| <= r of |imgL[y + j][x + i] - imgR[ty + sy + j][tx + sx + i]|, at most
 *     169 * 255 = 43 095.  Supports use the shifts (-1, 0), (0, 0), (+1, 0); correspondences also (0, -1) and (0, +1).
 *   A record is EVALUATED iff every pixel of every window it needs lies inside the image (the target's window with its
 *     shifts: +-1 in x for supports, in x and y for correspondences).  One that is not gets {0, 0, 0xFFFF, 0}.
 *   Per axis, with c-, c0, c+ the costs at the target's shifts -1, 0, +1: a = c- + c+ - 2 c0, n = c- - c+.  The axis HAS A
 *     MINIMUM iff c0 <= c-, c0 <= c+ and a > 0 (then |n| <= a), and the target's sub-pixel shift in 1/256 pixel is
 *     q = sgn(n) * ((256 |n| + a) div (2 a)): rounded half away from zero, |q| <= 128.  Otherwise q = 0 and the axis flag
 *     stays clear: the integer position is no local photometric minimum, which is itself a verification signal.
 * Output: one gpc_refinement per record; cost = c0; flags bit 0 evaluated, bit 1 minimum in x, bit 2 minimum in y.
 *   Supports have dy_q8 = 0 and never bit 2.  The refined target is (tx + dx_q8 / 256, ty + dy_q8 / 256).  For supports,
 *   `out` (optional) receives {x, y, d - (float)dx_q8 * 0.00390625f} (one float32 subtraction of an exact product; a record
 *   that is not evaluated is copied unchanged): an array gpc_hip_score_supports_device takes as it is.  Entries at i >= m_t
 *   of every output are left untouched.  Nothing is thresholded or compacted.
 * GPC_E_INVALID: r out of range, null required pointers, npairs < 1, cap_per_pair < 1, width or height < 1, `out`
 * overlapping the input records.  GPC_E_UNSUPPORTED: npairs > 65535, npairs * cap_per_pair > 2^31 - 1,
 * width * height > 2^30. */
typedef struct gpc_refinement {
  int16_t dx_q8, dy_q8; /* the target's sub-pixel shift in 1/256 pixel, -128 .. 128 */
  uint16_t cost;        /* c0; 0xFFFF when the record is not evaluated               */
  uint16_t flags;       /* bit 0 evaluated, bit 1 minimum in x, bit 2 minimum in y   */
} gpc_refinement;
/* Records and images already on the device: d_rec and d_ref (and d_out, which may be NULL) [npairs][cap_per_pair],
 * d_counts[npairs] (read on the device), d_imgL and d_imgR [npairs][height][width].  Pure functions of their arguments: no
 * forest is needed, and the calls only queue one launch on the context's stream; no workspace. */
int gpc_hip_refine_supports_device(gpc_hip_ctx* ctx, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts,
                                   const uint8_t* d_imgL, const uint8_t* d_imgR, int width, int height, int npairs, int radius,
                                   gpc_refinement* d_ref, gpc_support* d_out);
int gpc_hip_refine_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_rec, int cap_per_pair,
                                          const int32_t* d_counts, const uint8_t* d_imgL, const uint8_t* d_imgR, int width,
                                          int height, int npairs, int radius, gpc_refinement* d_ref);
/* Match and refine: gpc_hip_match_batch_device / gpc_hip_match_sequence_device exactly as they are -- into the caller's
 * d_supports / d_corr, d_counts and d_ncand (optional), with their settings, refusals, statuses and waiting; with two lanes
 * (gpc_hip_set_pipeline(ctx, 2)) the lanes are drained and the call runs on the context's stream -- then the refinement of
 * what they wrote, over the raw images (frames t and t + 1 for pair t of a sequence).  Group mode: the batch form refines
 * the union; the sequence form is GPC_E_UNSUPPORTED, as the sequence itself. */
int gpc_hip_refine_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                int npairs, const gpc_settings* settings, int radius, gpc_support* d_supports, int cap_per_pair,
                                int32_t* d_counts, int32_t* d_ncand, gpc_refinement* d_ref, gpc_support* d_out);
int gpc_hip_refine_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                   const gpc_settings* settings, int radius, gpc_correspondence* d_corr, int cap_per_pair,
                                   int32_t* d_counts, int32_t* d_ncand, gpc_refinement* d_ref);
/* Host records, counts, images and outputs through the records forms; synchronous, in chunks of at most 16 pairs, pageable
 * arrays through the context's page-locked arena.  Each pair's first m_t records travel; what comes back equals the device
 * forms byte for byte, untouched entries included. */
int gpc_hip_refine_supports(gpc_hip_ctx* ctx, const gpc_support* rec, int cap_per_pair, const int32_t* counts,
                            const uint8_t* imgL, const uint8_t* imgR, int width, int height, int npairs, int radius,
                            gpc_refinement* ref, gpc_support* out);
int gpc_hip_refine_correspondences(gpc_hip_ctx* ctx, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts,
                                   const uint8_t* imgL, const uint8_t* imgR, int width, int height, int npairs, int radius,
                                   gpc_refinement* ref);

/* ---- matching over an image pyramid ---------------------------------------------------- */
/* The matchers see a 27x27 window at one resolution.  These calls run them on every level of an image pyramid and merge
 * what the levels find into one record list in level 0's coordinates: texture coarser than the window, and motion beyond
 * disp_high, show at a coarser level.  The fern tests are offsets within the patch, so the same forest applies at every
 * level: level l sees a 27 * 2^l window of the original image.  The reference has no pyramid: the rules are this library's
 * own, made of integers only, so that every implementation of them gives the same bytes.
 *
 * Levels: 1 <= levels <= GPC_MAX_PYRAMID_LEVELS.  Level 0 is the input; level l has W_l = W >> l and H_l = H_{l-1} / 2
 *   rounded down (an odd last row is dropped).  Every level must be an image the library takes today (W_l % 16 == 0,
 *   W_l >= 42, H_l >= 30), else GPC_E_INVALID: 3 levels need W % 64 == 0, W >= 192, H >= 120.
 * Downsampling: level l's raw image is the 2x2 mean of level l-1's raw image, out[y][x] = (a + b + c + d + 2) >> 2 over
 *   in[2y .. 2y+1][2x .. 2x+1].  Each level is then preprocessed and hashed exactly as an image of its own size is by
 *   gpc_hip_match_batch_device / gpc_hip_match_sequence_device (box and Sobel on that level's raw image).
 * Settings of level l: gradient_threshold, epipolar_mode and use_hashtable unchanged; disp_high_l = disp_high >> l,
 *   vertical_tolerance_l = vertical_tolerance >> l, so a mapped record never exceeds the caller's bounds.
 * Mapping: a level-l support (x, y, d) becomes (x << l, y << l, d * 2^l) (the float stays exact); a correspondence has all
 *   four coordinates shifted left by l.  A level-l pixel is the 2^l x 2^l BLOCK of level-0 pixels [x << l, (x << l) + 2^l) x
 *   [y << l, (y << l) + 2^l); the block's TOP-LEFT CORNER stands for the block, so a coarse record carries up to 2^l - 1
 *   pixels of position it does not resolve.
 * Merge, per pair: level 0's records come first, all of them, in the matcher's order.  Then, for l = 1 .. levels-1 in
 *   turn, level l's mapped records in the matcher's order, a record being kept if and only if its source block holds the
 *   (mapped) source pixel of no record kept from levels < l.  Records of one level never suppress each other; a kept
 *   level-l record does suppress levels > l.  A level-l record whose source lies outside [0, W >> l) x [0, H >> l) (only
 *   records a caller constructs) has no block: it is kept and suppresses nothing.
 * Capacity: the merge is decided on all records, never on the capped ones.  d_counts[npairs] holds the true totals,
 *   d_level_counts[levels][npairs] the true kept counts per level (their sum is the total; they recover each record's
 *   level), d_ncand (optional) the candidate counts of every level, [levels][npairs][2] for pairs and [levels][nframes] for
 *   frames.  A pair's first min(count, cap_per_pair) records are valid and nothing is written behind them.  The device forms
 *   return GPC_OK, the host forms GPC_E_CAPACITY, as gpc_hip_match_batch_device and gpc_hip_match_sequence do.
 * levels == 1: byte for byte what gpc_hip_match_batch_device / gpc_hip_match_sequence_device write; d_level_counts equals
 *   d_counts.
 * Every matcher (epipolar_mode 0 / 1 x use_hashtable 0 / 1) and either arithmetic is taken: the match of a level is the
 *   existing one, with its waiting (the device-wide matchers wait on the host once per level).  Refusals: group mode with
 *   more than one group GPC_E_UNSUPPORTED; no forest GPC_E_NO_FOREST; a forest whose size is not width x height (level 0)
 *   GPC_E_INVALID; more than 65535 pairs GPC_E_UNSUPPORTED.  With two lanes (gpc_hip_set_pipeline(ctx, 2)) the lanes are
 *   drained and the call runs on the context's stream.  After a call the context's forest, its size and the generation of
 *   its codes are what they were: a plain match at width x height needs no gpc_hip_set_forest, and a track stream hashed
 *   before the call still takes frames.
 * Workspaces of the context, grown on demand: the raw images of levels 1 .. levels-1 (a third of the input), every record
 *   of every level ((W_l - 26) * (H_l - 26) + 1 per pair and level), one bit per pixel and pair, one bit per record slot. */
#define GPC_MAX_PYRAMID_LEVELS 4
/* Host only: the geometry check above; widths, heights (optional) receive `levels` entries each. */
int gpc_hip_pyramid_levels(int width, int height, int levels, int32_t* widths, int32_t* heights);
/* One downsampling step over d_src[nimages][height][width], writing d_dst[nimages][height / 2][width / 2].  width % 32 == 0,
 * height >= 2, d_src 8-byte and d_dst 4-byte aligned (GPC_E_INVALID otherwise); nimages <= 65535.  Needs no forest;
 * asynchronous on the context's stream. */
int gpc_hip_pyramid_down_device(gpc_hip_ctx* ctx, const uint8_t* d_src, int width, int height, int nimages, uint8_t* d_dst);
/* The merge alone, over records already on the device: d_rec, caps and d_cnt are HOST arrays of `levels` entries -- level
 * l's records d_rec[l][npairs][caps[l]] (unmapped, as the matcher wrote them at level l), its capacity, and its counts
 * d_cnt[l][npairs] (read on the device; min(max(count, 0), caps[l]) records are read).  width, height describe level 0 and
 * may be any positive size.  Outputs as above.  Needs no forest; the calls only queue work on the context's stream (per
 * level: test and count, scan, write and mark). */
int gpc_hip_pyramid_merge_supports_device(gpc_hip_ctx* ctx, const gpc_support* const* d_rec, const int32_t* caps,
                                          const int32_t* const* d_cnt, int width, int height, int npairs, int levels,
                                          gpc_support* d_out, int cap_per_pair, int32_t* d_counts, int32_t* d_level_counts);
int gpc_hip_pyramid_merge_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* const* d_rec, const int32_t* caps,
                                                 const int32_t* const* d_cnt, int width, int height, int npairs, int levels,
                                                 gpc_correspondence* d_out, int cap_per_pair, int32_t* d_counts,
                                                 int32_t* d_level_counts);
/* Match and merge: raw pairs (frames) in HBM as gpc_hip_match_batch_device (gpc_hip_match_sequence_device) takes them.
 * Every frame of a sequence is downsampled, preprocessed and hashed once per level. */
int gpc_hip_pyramid_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                 int npairs, int levels, const gpc_settings* settings, gpc_support* d_out, int cap_per_pair,
                                 int32_t* d_counts, int32_t* d_level_counts, int32_t* d_ncand);
int gpc_hip_pyramid_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes, int levels,
                                    const gpc_settings* settings, gpc_correspondence* d_out, int cap_per_pair,
                                    int32_t* d_counts, int32_t* d_level_counts, int32_t* d_ncand);
/* The same from / to host memory (pageable or page-locked), synchronous, in chunks of at most 16 pairs (16 frames;
 * consecutive chunks of a sequence share one).  What comes back equals the device forms byte for byte; bytes of `out` the
 * device form does not write stay as they were. */
int gpc_hip_pyramid_batch(gpc_hip_ctx* ctx, const uint8_t* rawL, const uint8_t* rawR, int width, int height, int npairs,
                          int levels, const gpc_settings* settings, gpc_support* out, int cap_per_pair, int32_t* counts,
                          int32_t* level_counts, int32_t* ncand);
int gpc_hip_pyramid_sequence(gpc_hip_ctx* ctx, const uint8_t* frames, int width, int height, int nframes, int levels,
                             const gpc_settings* settings, gpc_correspondence* out, int cap_per_pair, int32_t* counts,
                             int32_t* level_counts, int32_t* ncand);

/* ---- dense maps from sparse matches: hierarchical fill ---------------------------------- */
/* Every call above ends in a record list; these end in a FIELD: one disparity, or one (u, v), per pixel, in 1/256 pixel.
 * This is scattered-data interpolation by a hierarchical ("pull-push") fill: a pixel that has a match keeps it, a pixel
 * without one takes the mean of the matches in the smallest aligned block around it that holds enough of them.  The
 * reference's product is such an image (disparity.png) and the GPC paper hands its matches to an interpolator; the rule
 * here is this library's own, made of integers only, so that every implementation of it gives the same bytes.  The outputs
 * of the consensus filter (whole d), of the refinement (d_ref) and of the pyramid merge (finer records first) are taken
 * unchanged.
 *
 * Input: P = npairs lists rec[t][0 .. m_t), m_t = min(max(counts[t], 0), cap_per_pair), for images of width x height;
 *   optionally one gpc_refinement ref[t][i] per record, as gpc_hip_refine_* writes it.
 *   Source and target as in the consensus filter: (src_x, src_y) -> (tar_x, tar_y) of a correspondence; (x, y) ->
 *     (x - (int)d, y) of a support.
 *   A record PARTICIPATES iff source and target lie in [0, width) x [0, height); a support must also have d finite,
 *     d == truncf(d) and |d| < 2^24; and, when ref is given and max_cost < 0xFFFF, flags bit 0 is set and cost <= max_cost.
 *     With max_cost == 0xFFFF a record that was not evaluated still participates, with shift 0.
 *   Value in 1/256 pixel (Q8): a support has one channel, 256 * (int)d - dx_q8; a correspondence two, u = 256 * (tar_x -
 *     src_x) + dx_q8 and v = 256 * (tar_y - src_y) + dy_q8.  The shift is 0 without ref or when flags bit 0 is clear.  (A
 *     support's value / 256 is the d that gpc_hip_refine_supports_device writes to its `out`.)
 * Level 0: a pixel is OCCUPIED iff some participating record has it as its source; of several, the one with the lowest
 *   input index stands for it (after a pyramid merge or a group union the finer or earlier record wins).  An occupied pixel
 *   has its record's value and level 0.
 * Pull: for l >= 1, cell (X, Y) of level l is the pixel block [X << l, (X + 1) << l) x [Y << l, (Y + 1) << l), clipped to
 *   the image; n_l is the number of occupied pixels in it, S_l the exact integer sum of their values, per channel.  The grid
 *   of level l has ((width - 1) >> l) + 1 columns and ((height - 1) >> l) + 1 rows; Lmax is the first level of one cell.
 * Push: for a pixel (x, y) that is not occupied, l = 1, 2, .. min(max_level, Lmax) in turn: N and SUM are n_l and S_l
 *   summed over the cells of the level-l grid within Chebyshev distance `spread` (0 or 1) of the pixel's cell (x >> l,
 *   y >> l).  At the first l with N >= min_count the pixel's value is sgn(SUM) * ((2 |SUM| + N) div (2 N)) per channel -- the
 *   mean, rounded half away from zero as the refinement rounds -- and its level is l.  If no level qualifies the value is
 *   GPC_DENSE_NONE in every channel and the level 255.
 * Output: value[P][C][height][width] int32 with C = 1 for supports and 2 for correspondences (the u plane, then the v
 *   plane); level[P][height][width] uint8 (optional).  Every pixel of every pair is written.
 * GPC_E_INVALID: a parameter out of range, a null required pointer, npairs < 1, cap_per_pair < 1, width or height < 1,
 * max_cost < 0xFFFF without ref.  GPC_E_UNSUPPORTED: width or height > 32768 (what keeps |value| < 2^24 and every sum below
 * 2^54), width * height > 2^30, npairs > 65535, npairs * cap_per_pair > 2^31 - 1. */
#define GPC_DENSE_NONE (-2147483647 - 1) /* INT32_MIN: no block around the pixel holds min_count matches */
typedef struct gpc_densify {
  int32_t max_level;  /* 1 .. 15; levels above Lmax are never reached            */
  int32_t min_count;  /* 1 .. 65536 matches a block needs before it fills a pixel */
  int32_t spread;     /* 0: the pixel's own cell; 1: its 3x3 cells               */
  int32_t max_cost;   /* 0 .. 0xFFFF; 0xFFFF = no ceiling; needs ref otherwise   */
} gpc_densify;        /* documented defaults: 15, 1, 1, 0xFFFF */
/* Records already on the device, in the layout the matchers write: d_rec and d_ref (which may be NULL) [npairs][cap_per_pair],
 * d_counts[npairs] (read on the device), d_value[npairs][C][height][width], d_level[npairs][height][width] (may be NULL).
 * Pure functions of their arguments: no forest is needed, and the calls only queue work on the context's stream (a memset,
 * claim, pull, the levels above a 32 x 32 tile, push); read the outputs after gpc_hip_synchronize or another wait on the
 * stream.  Workspaces of the context, grown on demand, per pixel and pair: 4 bytes (the owner plane) and at most
 * (4 + 8 C) / 3 + 1 bytes (the cells' counts and sums: a third of a pixel's worth of cells over all levels). */
int gpc_hip_densify_supports_device(gpc_hip_ctx* ctx, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts,
                                    const gpc_refinement* d_ref, int width, int height, int npairs, const gpc_densify* prm,
                                    int32_t* d_value, uint8_t* d_level);
int gpc_hip_densify_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_rec, int cap_per_pair,
                                           const int32_t* d_counts, const gpc_refinement* d_ref, int width, int height, int npairs,
                                           const gpc_densify* prm, int32_t* d_value, uint8_t* d_level);
/* Match, refine and fill: gpc_hip_match_batch_device / gpc_hip_match_sequence_device exactly as they are, into the workspace
 * of the context that holds every record of every pair (the one gpc_hip_consensus_batch_device uses); then, when
 * refine_radius >= 1 (0 .. 6, 0 = none), the refinement of gpc_hip_refine_*_device over the raw images into a workspace of 8
 * bytes per record slot; then the fill, with those refinements as ref.  Settings, refusals, statuses and waiting are those
 * of the match they wrap; with two lanes (gpc_hip_set_pipeline(ctx, 2)) the lanes are drained and the call runs on the
 * context's stream.  d_counts[P] (optional) receives the match's counts, d_ncand (optional) the candidate counts as the
 * match writes them ([P][2] for the batch, [nframes] for the sequence).  Group mode: the batch form fills from the union;
 * the sequence form is GPC_E_UNSUPPORTED, as the sequence itself.  max_cost < 0xFFFF with refine_radius 0: GPC_E_INVALID. */
int gpc_hip_densify_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                 int npairs, const gpc_settings* settings, int refine_radius, const gpc_densify* prm,
                                 int32_t* d_value, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
int gpc_hip_densify_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                    const gpc_settings* settings, int refine_radius, const gpc_densify* prm, int32_t* d_value,
                                    uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
/* Host records, counts, refinements and outputs through the records forms; synchronous, in chunks of at most 16 pairs,
 * pageable arrays through the context's page-locked arena.  Each pair's first m_t records (and refinements) travel; what
 * comes back equals the device forms byte for byte. */
int gpc_hip_densify_supports(gpc_hip_ctx* ctx, const gpc_support* rec, int cap_per_pair, const int32_t* counts,
                             const gpc_refinement* ref, int width, int height, int npairs, const gpc_densify* prm,
                             int32_t* value, uint8_t* level);
int gpc_hip_densify_correspondences(gpc_hip_ctx* ctx, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts,
                                    const gpc_refinement* ref, int width, int height, int npairs, const gpc_densify* prm,
                                    int32_t* value, uint8_t* level);

/* ---- stereo sequences: circular matches closed into quads ----------------------------- */
/* A stereo video is where both kinds of match apply: the supports of (L_t, R_t) and the correspondences of (L_t, L_t+1)
 * and (R_t, R_t+1).  The circular match L_t -> R_t -> R_t+1 -> L_t+1 -> L_t joins them by pixel position; it is the
 * strongest outlier filter a stereo rig gives for free, and what it keeps is a sparse scene-flow record: position,
 * disparity before, image motion, disparity after.  The reference has no counterpart: it matches one pair
 * (Forest::stereoMatch, inference.hpp:344-361) and leaves every use of two results to its caller.  The rule is therefore
 * this library's own; it is made of integers only, so that every implementation of it gives the same bytes.
 *
 * N = nframes stereo frames, P = N - 1 steps, images of width x height, a pixel's index y * width + x.  Inputs: per frame
 * t the supports S[t][0 .. ms_t) of (L_t, R_t), ms_t = min(max(nsup[t], 0), cap_s); per step t FL[t][0 .. mfl_t) of
 * (L_t, L_t+1) and FR[t][0 .. mfr_t) of (R_t, R_t+1), clipped to cap_f in the same way.
 *   A support takes part when 0 <= x < width, 0 <= y < height, d is finite and integral with |d| <= 16384 (tested before
 *     d is converted, so that no conversion is undefined) and 0 <= x - (int)d < width.  Its left pixel is (x, y), its
 *     right pixel (x - d, y).  A flow record takes part when its source and its target lie inside the image.
 *   Lookup: first_S[t](p) is the lowest i that takes part and whose left pixel is p; first_FL[t](p) and first_FR[t](p) the
 *     lowest j that takes part and whose source pixel is p; "none" where there is no such record.
 *   Start: support i of S[t], t < P, when it takes part and i == first_S[t](its left pixel).
 *   Closing, for a start i with left pixel a, right pixel b and disparity d: j = first_FL[t](a) and k = first_FR[t](b) must
 *     both exist; a' = the target of FL[t][j], b' = the target of FR[t][k]; i' = first_S[t+1](a') must exist, with disparity
 *     d'; c' = (a'.x - d', a'.y); the circle closes when |c'.x - b'.x| <= tol and |c'.y - b'.y| <= tol.
 *   Settle: among the starts of step t that close on the same i' the lowest i keeps its quad -- the lowest index is the one
 *     choice that does not depend on which thread arrives first.  So every support of frame t + 1 ends at most one quad of
 *     step t and starts at most one of step t + 1: a consumer chains quads by support1 == support0 of the next step.
 *   Output: the quads of step t by i ascending in quads[t][0 .. min(nq_t, quad_cap)); nquads[t] = nq_t is the true count;
 *     nothing is written behind a step's valid quads.  quad_cap = 0 is allowed, and quads may then be NULL.
 * 0 <= tol <= 255, nframes >= 2, cap_s, cap_f > 0, quad_cap >= 0: GPC_E_INVALID otherwise.  nframes * cap_s,
 * (nframes - 1) * cap_f and (nframes - 1) * quad_cap must not exceed 2^31 - 1, width * height 2^30 and nframes 65535
 * (GPC_E_UNSUPPORTED). */
typedef struct gpc_quad {
  int32_t x, y;     /* a: the point in L_t; in R_t it is (x - d0, y)                                   */
  int32_t d0;       /* d: the disparity at t                                                           */
  int32_t u, v;     /* a' - a: the point in L_t+1 is (x + u, y + v), in R_t+1 (x + u - d1, y + v)       */
  int32_t d1;       /* d': the disparity at t + 1                                                      */
  int32_t support0; /* i:  the start's index in S[t]                                                   */
  int32_t support1; /* i': the index in S[t + 1] the circle closes on                                  */
} gpc_quad;
/* Records already on the device, in the layouts gpc_hip_match_batch_device (d_sup [N][cap_s], d_nsup[N]) and
 * gpc_hip_match_sequence_device (d_flowL, d_flowR [P][cap_f], d_nflowL, d_nflowR [P]) write; d_quads [P][quad_cap],
 * d_nquads[P].  No forest is needed; the counts are read on the device, and the call only queues work on the context's
 * stream (six launches per group of steps: fill the per-pixel planes, scatter the record indices, close, settle and
 * count, scan, write); read the outputs after gpc_hip_synchronize or another wait on the stream.  Workspaces of the
 * context, grown on demand, for a group of g steps: 4 bytes per pixel for each of 3 g + 1 planes, 8 bytes per support slot
 * of g frames (plus 4 bytes per 2048 of them).  g is all P steps where that stays within 1 GiB of planes, else the
 * largest number of steps that does (at least one): the steps then go through the launches in groups, with the same
 * result. */
int gpc_hip_quads_records_device(gpc_hip_ctx* ctx, const gpc_support* d_sup, int cap_s, const int32_t* d_nsup,
                                 const gpc_correspondence* d_flowL, const gpc_correspondence* d_flowR, int cap_f,
                                 const int32_t* d_nflowL, const int32_t* d_nflowR, int width, int height, int nframes, int tol,
                                 gpc_quad* d_quads, int quad_cap, int32_t* d_nquads);
/* The three record sets of a stereo sequence from ONE k_preprocess and ONE k_hash launch over its 2 N images (d_left,
 * d_right: [N][height][width] each): exactly what gpc_hip_match_batch_device(d_left, d_right, stereo_settings),
 * gpc_hip_match_sequence_device(d_left, flow_settings) and gpc_hip_match_sequence_device(d_right, flow_settings) write, in
 * that order, with any matcher setting on either side and either arithmetic.  d_ncand[2][N] (optional): the candidates of
 * the left frames, then of the right frames.  The two settings must share gradient_threshold (GPC_E_INVALID otherwise).
 * Group mode: GPC_E_UNSUPPORTED; no forest: GPC_E_NO_FOREST; with two lanes (gpc_hip_set_pipeline(ctx, 2)) the lanes are
 * drained and the call runs on the context's stream.  Waiting is as gpc_hip_match_batch_device and
 * gpc_hip_match_sequence_device document it.  The images are hashed in the batch's order [t][side]; each side's code
 * images are then copied on the device into a block of their own (4 bytes per pixel and image held twice), which the flow
 * joins read as a sequence's frames. */
int gpc_hip_match_stereo_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                         int nframes, const gpc_settings* stereo_settings, const gpc_settings* flow_settings,
                                         gpc_support* d_sup, int cap_s, int32_t* d_nsup, gpc_correspondence* d_flowL,
                                         gpc_correspondence* d_flowR, int cap_f, int32_t* d_nflowL, int32_t* d_nflowR,
                                         int32_t* d_ncand);
/* gpc_hip_match_stereo_sequence_device, then gpc_hip_quads_records_device over what it wrote: all outputs of both. */
int gpc_hip_quads_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                                  int nframes, const gpc_settings* stereo_settings, const gpc_settings* flow_settings, int tol,
                                  gpc_support* d_sup, int cap_s, int32_t* d_nsup, gpc_correspondence* d_flowL,
                                  gpc_correspondence* d_flowR, int cap_f, int32_t* d_nflowL, int32_t* d_nflowR, int32_t* d_ncand,
                                  gpc_quad* d_quads, int quad_cap, int32_t* d_nquads);
/* The same from / to host memory (pageable or page-locked), synchronous.  GPC_E_CAPACITY when any count exceeds its
 * capacity (a frame's supports cap_s, a step's correspondences cap_f, a step's quads quad_cap); what is written is then as
 * defined above.  gpc_hip_quads_records needs no forest and sends each list's first m records only.  A quad joins records
 * of two frames and three lists, so neither form is cut into chunks: the whole call is staged on the device and the
 * device form runs once.  The calls are therefore BOUNDED BY DEVICE MEMORY: they hold
 *   N * cap_s * 12  +  2 * P * cap_f * 16  +  P * quad_cap * 32   bytes of staging (the sequence form 2 * N * W * H more;
 *   the counts and the padding of each block to 16 bytes are not counted),
 *   the closing workspace stated at gpc_hip_quads_records_device, and (the sequence form) what the matchers keep for 2 N
 *   images: smoothed image, gradient image and codes, 6 bytes per pixel and image, 4 more for each side's copy of the
 *   codes, plus the chosen matchers' own workspaces. */
int gpc_hip_quads_records(gpc_hip_ctx* ctx, const gpc_support* sup, int cap_s, const int32_t* nsup,
                          const gpc_correspondence* flowL, const gpc_correspondence* flowR, int cap_f, const int32_t* nflowL,
                          const int32_t* nflowR, int width, int height, int nframes, int tol, gpc_quad* quads, int quad_cap,
                          int32_t* nquads);
int gpc_hip_quads_sequence(gpc_hip_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int nframes,
                           const gpc_settings* stereo_settings, const gpc_settings* flow_settings, int tol, gpc_support* sup,
                           int cap_s, int32_t* nsup, gpc_correspondence* flowL, gpc_correspondence* flowR, int cap_f,
                           int32_t* nflowL, int32_t* nflowR, int32_t* ncand, gpc_quad* quads, int quad_cap, int32_t* nquads);

/* ---- clean dense fields: cross-check, speckles, median ------------------------------------ */
/* The fill of gpc_hip_densify_* gives a value to every pixel that has min_count matches somewhere around it: occluded
 * regions, the halo of a foreground object and the blocks around a single wrong match are filled too.  This stage takes
 * them out again: the left-right (forward-backward) consistency check, the removal of small connected segments (as
 * OpenCV's filterSpeckles does it) and a small median.  The matcher is symmetric, so the backward field costs no second
 * match: the same records, read from their target's side (gpc_hip_flip_*), fill it.  The reference has no counterpart
 * (it writes disparity.png from the raw supports); the rule is this library's own, made of integers only, so that every
 * implementation of it gives the same bytes.
 *
 * Input: P = npairs fields fwd[P][C][height][width] int32 as gpc_hip_densify_* writes them, C = channels: 1 for a
 *   disparity, 2 for u then v.  GPC_DENSE_NONE means no value; any other int32 is a value.  Optionally bwd[P][C][height]
 *   [width], the field of the reversed records.  All sums and differences below are taken in 64 bits: no input value can
 *   overflow them, and nothing is undefined for INT32_MAX or INT32_MIN + 1.  F_c(p) is fwd at pixel p in channel c, G_c bwd.
 * Each pixel p = (x, y) has one STATE; the first rule that applies decides it:
 *   1 none: F_0(p) is GPC_DENSE_NONE.
 *   2 failed check (only with check_tol_q8 >= 0): r_c = sgn(F_c) * ((|F_c| + 128) >> 8) is the whole-pixel shift, rounded
 *     half away from zero; the target is q = (x - r_0, y) with C = 1 and q = (x + r_0, y + r_1) with C = 2.  The pixel fails
 *     when q is outside the image, or G_0(q) is GPC_DENSE_NONE, or |F_c(p) + G_c(q)| > check_tol_q8 in some channel.  (A
 *     support's value is 256 d with the right pixel at x - d, and its reversed record has d' = -d: F + G is 0 for a
 *     consistent pair, in both record types.)
 *   3 speckle (only with speckle_min > 1): among the pixels that are not in state 1 or 2, two 4-neighbours p, q belong
 *     together iff |F_c(p) - F_c(q)| <= speckle_diff_q8 in every channel; a pixel is a speckle iff its connected
 *     component under the closure of this relation has fewer than speckle_min pixels.
 *   0 kept: every other pixel.
 * Outputs; every element of every output is written:
 *   out[P][C][height][width]: a kept pixel gets, per channel, the lower median of F_c over the kept pixels of its
 *     (2 r + 1)^2 window clipped to the image, r = median_radius: element (n - 1) >> 1 of the n values in ascending order;
 *     with r = 0 that is F_c itself.  The medians read fwd, never out.  Every other pixel gets GPC_DENSE_NONE in every channel.
 *   state[P][height][width] uint8 (optional).
 *   label[P][height][width] int32 (optional): for a pixel not in state 1 or 2 the lowest pixel index y * width + x of its
 *     component, otherwise -1.  Speckle pixels keep their label.  It is computed whenever it is asked for, whatever
 *     speckle_min is.
 *   stats[P][4] int32 (optional): the number of pixels in states 0, 1, 2 and 3.
 * GPC_E_INVALID: a parameter out of range, channels not 1 or 2, check_tol_q8 >= 0 without bwd, a null required pointer, out
 * overlapping fwd or bwd, width, height or npairs < 1.  GPC_E_UNSUPPORTED: width or height > 32768, width * height > 2^30,
 * npairs > 65535 (the limits of the densify block). */
typedef struct gpc_clean {
  int32_t check_tol_q8;    /* -1 = no cross-check; 0 .. 2^24 otherwise, needs bwd                  */
  int32_t speckle_diff_q8; /* 0 .. 2^24: neighbours belong together when they differ by at most it */
  int32_t speckle_min;     /* 0 .. 2^30: a segment of fewer pixels is removed; 0 and 1 = none      */
  int32_t median_radius;   /* 0 (none), 1 (3x3) or 2 (5x5)                                         */
} gpc_clean;               /* documented defaults: 256, 256, 64, 1 */
/* Fields already on the device.  A pure function of its arguments: no forest is needed, and the call only queues work on
 * the context's stream (check; per-tile labelling, the union across tile edges, flatten and the size count where labels
 * or sizes are needed; apply); read the outputs after gpc_hip_synchronize or another wait on the stream.  Workspaces of
 * the context, grown on demand, per pixel and pair: 4 bytes for the labels (the fill's owner plane, which is free by then;
 * d_label itself where it is given) and 4 for the sizes (only with speckle_min > 1). */
int gpc_hip_clean_fields_device(gpc_hip_ctx* ctx, const int32_t* d_fwd, const int32_t* d_bwd, int channels, int width,
                                int height, int npairs, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                                int32_t* d_label, int32_t* d_stats);
/* Reversed records, element-wise: slot i goes to slot i for i < m_t = min(max(d_counts[t], 0), cap_per_pair), so the counts
 * stay valid; nothing else is written.  A correspondence (sx, sy, tx, ty) becomes (tx, ty, sx, sy).  A support (x, y, d)
 * becomes (x - (int)d, y, -d) -- the subtraction wraps in 32 bits, -d flips the sign bit -- provided d is finite, whole and
 * |d| < 2^24; otherwise it becomes (-1, -1, 0), which the fill ignores.  A refinement has dx_q8 and dy_q8 negated (in 16
 * bits); cost and flags are copied.  d_ref and d_ref_out are optional, but go together (GPC_E_INVALID otherwise, as for a
 * null required pointer, npairs or cap_per_pair < 1; GPC_E_UNSUPPORTED: npairs > 65535, npairs * cap_per_pair > 2^31 - 1).
 * d_rec_out may be d_rec and d_ref_out d_ref (in place); any other overlap is undefined.  One launch on the context's stream. */
int gpc_hip_flip_supports_device(gpc_hip_ctx* ctx, const gpc_support* d_rec, const gpc_refinement* d_ref, int cap_per_pair,
                                 const int32_t* d_counts, int npairs, gpc_support* d_rec_out, gpc_refinement* d_ref_out);
int gpc_hip_flip_correspondences_device(gpc_hip_ctx* ctx, const gpc_correspondence* d_rec, const gpc_refinement* d_ref,
                                        int cap_per_pair, const int32_t* d_counts, int npairs, gpc_correspondence* d_rec_out,
                                        gpc_refinement* d_ref_out);
/* Match, refine, fill, flip, fill again, clean: exactly gpc_hip_densify_batch_device / gpc_hip_densify_sequence_device --
 * the same settings, refinement, refusals, statuses, waiting and lane draining, group mode as there -- whose field is the
 * forward field; then the records (and their refinements) are reversed where they lie, the reversed records are filled
 * with the same gpc_densify into the backward field (only with check_tol_q8 >= 0), and gpc_hip_clean_fields_device runs
 * over the two.  d_out is required; d_state, d_label, d_stats as above; d_fwd [P][C][height][width] (optional) receives the
 * forward field and d_level (optional) its levels; d_counts and d_ncand (optional) as in the densify forms.  Workspaces of
 * the context beyond those of the calls it is made of: the backward field, and the forward field where d_fwd is null. */
int gpc_hip_clean_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height, int npairs,
                               const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_clean* prm,
                               int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                               uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
int gpc_hip_clean_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                  const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_clean* prm,
                                  int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                                  uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
/* Host fields and outputs through gpc_hip_clean_fields_device; synchronous, in chunks of at most 16 pairs, pageable arrays
 * through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_clean_fields(gpc_hip_ctx* ctx, const int32_t* fwd, const int32_t* bwd, int channels, int width, int height,
                         int npairs, const gpc_clean* prm, int32_t* out, uint8_t* state, int32_t* label, int32_t* stats);

/* ---- search the image pair around every pixel of a dense field ------------------------------ */
/* The fill of gpc_hip_densify_* gives a pixel the mean of the matches in a block around it: an interpolation, right to a
 * pixel or two on smooth surfaces and wrong across object edges, and no later stage compares the two images at a pixel that
 * had no match of its own.  This stage does, as ELAS does with its supports: the filled value is a prior, and a small search
 * around it in the other image, by the SAD cost and the parabola of gpc_hip_refine_*, replaces it with what the images say.
 * It belongs between the fill and the cleaner.  The reference has no counterpart; the rule is this library's own, made of
 * integers only, so that every implementation of it gives the same bytes.
 *
 * Input: P = npairs fields field[P][C][height][width] int32 in 1/256 pixel as gpc_hip_densify_* writes them, C = channels: 1
 *   for a disparity, 2 for u then v; imgL[P][height][width] and imgR[P][height][width] uint8.  A pixel p is a HOLE iff F_0(p)
 *   is GPC_DENSE_NONE, whatever F_1 holds; every other pixel is VALUED.  All arithmetic on field values is done in 64 bits:
 *   nothing is undefined for INT32_MAX, INT32_MIN + 1 or an F_1 that is GPC_DENSE_NONE.  r = radius, R = range.
 * Per valued pixel p = (x, y):
 *   1 pixels by clamped address: I(img, x, y) = img[clamp(y, 0, height-1)][clamp(x, 0, width-1)], and
 *     cost(p, t) = sum over |i|, |j| <= r of |I(imgL, x+i, y+j) - I(imgR, tx+i, ty+j)|: border pixels are evaluated like any
 *     other.  The largest cost is 81 * 255 = 20655.
 *   2 base target: r_c = sgn(F_c) * ((|F_c| + 128) >> 8), the cleaner's rounding; b = (x - r_0, y) with C = 1 and
 *     b = (x + r_0, y + r_1) with C = 2.
 *   3 candidates: k = (kx, 0), |kx| <= R with C = 1; k = (kx, ky), |kx|, |ky| <= R with C = 2.  Candidate k has the target
 *     t_k = b + k and is ADMISSIBLE iff t_k lies inside the image.  A valued pixel without an admissible candidate is UNMATCHED.
 *   4 best: the admissible candidate with the lexicographically smallest (cost, |kx| + |ky|, ky, kx): on equal cost the
 *     prior wins, then the nearer candidate, then a fixed order.
 *   5 sub-pixel shift (only with subpixel = 1), per axis -- x always, y only with C = 2: when both neighbours of t_best
 *     along the axis lie inside the image (they need not be candidates), their costs c-, c+ and c0 = cost(p, t_best) go
 *     through the parabola of gpc_hip_refine_*: a = c- + c+ - 2 c0, n = c- - c+; the axis has a minimum iff c0 <= c-,
 *     c0 <= c+ and a > 0, and then q = sgn(n) * ((256 |n| + a) div 2a); otherwise q = 0.
 *   6 value: 256 (r_0 - kx) - qx with C = 1; u = 256 (r_0 + kx) + qx and v = 256 (r_1 + ky) + qy with C = 2: the
 *     conventions of the fill.  Admissibility bounds |r_c| by the image size, so nothing overflows.
 *   7 a matched pixel with c0 > max_cost is REJECTED.
 * Outputs; every element of every output is written:
 *   out[P][C][height][width]: the value for a matched pixel that is not rejected (KEPT); GPC_DENSE_NONE in every channel for
 *     holes, unmatched and rejected pixels.  out == field (the same pointer) is allowed and gives the same bytes: a pixel
 *     reads only its own field value.
 *   cost[P][height][width] uint16 (optional): c0 of the best candidate, also for a rejected pixel; 0xFFFF for holes and
 *     unmatched pixels.
 *   choice[P][height][width] uint8 (optional): (ky + R) (2R + 1) + (kx + R) of the best candidate, kx + R with C = 1; 255
 *     for holes and unmatched pixels.
 *   stats[P][4] int32 (optional): the numbers of pixels kept, hole, unmatched and rejected.
 * GPC_E_INVALID: a parameter out of range, channels not 1 or 2, a null required pointer (field, imgL, imgR, out, prm), width,
 * height or npairs < 1, out overlapping field other than being it, out overlapping an image.  GPC_E_UNSUPPORTED: width or
 * height > 32768, width * height > 2^30, npairs > 65535 (the limits of the densify block).  r <= 4 and R <= 2 keep a target
 * row with all its shifts within 2r + 1 + 2(R + 1) <= 15 bytes, one 16-byte load. */
typedef struct gpc_search {
  int32_t radius;    /* r, 1 .. 4: the window is (2 r + 1)^2                                   */
  int32_t range;     /* R, 0 .. 2: candidates within R whole pixels of the base; 0 = verify only */
  int32_t subpixel;  /* 0 or 1                                                                  */
  int32_t max_cost;  /* 0 .. 0xFFFF; 0xFFFF = no ceiling                                        */
} gpc_search;        /* documented defaults: 2, 1, 1, 0xFFFF -- a choice, not a measurement     */
/* A field and its two images already on the device.  A pure function of its arguments: no forest is needed, and the call
 * only queues work on the context's stream (a clear of the stats, one launch); read the outputs after gpc_hip_synchronize or
 * another wait on the stream.  No workspace. */
int gpc_hip_search_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR,
                                 int channels, int width, int height, int npairs, const gpc_search* prm, int32_t* d_out,
                                 uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats);
/* Match, refine, fill, search, flip, fill again, search with the two images exchanged, clean: exactly
 * gpc_hip_clean_batch_device / gpc_hip_clean_sequence_device -- the same settings, refusals, statuses, waiting, lane draining
 * and group-mode behaviour -- with gpc_hip_search_fields_device run in place over the forward field and (only with
 * check_tol_q8 >= 0) over the backward field.  The images are d_rawL and d_rawR (batch), frames t and t + 1 for pair t
 * (sequence).  d_fwd (optional) receives the searched forward field and d_cost [P][height][width] (optional) its costs; every
 * other argument is the clean form's.  No workspace beyond those of the calls it is made of.  Completion
 * (gpc_hip_inpaint_fields_device) over the result is composed by the caller. */
int gpc_hip_search_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height, int npairs,
                                const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_search* search,
                                const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats,
                                int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost);
int gpc_hip_search_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                   const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_search* search,
                                   const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats,
                                   int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost);
/* A host field, images and outputs through gpc_hip_search_fields_device; synchronous, in chunks of at most 16 pairs, pageable
 * arrays through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_search_fields(gpc_hip_ctx* ctx, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels, int width,
                          int height, int npairs, const gpc_search* prm, int32_t* out, uint16_t* cost, uint8_t* choice,
                          int32_t* stats);

/* ---- aggregate the search's costs along scanlines ------------------------------------------- */
/* The search above lets every pixel decide alone: a tie or a near-tie in a weakly textured window is settled by a fixed
 * order, and nothing asks whether the pixel beside it chose the same displacement.  This stage is a second way to choose
 * among the SAME candidates by the SAME costs: before the choice a smoothness term is added along scanlines, in the form of
 * the path aggregation of semi-global matching, which stays in integers.  It sits where the search sits, between the fill
 * and the cleaner.  The search itself is unchanged.
 *
 * Inputs, I, cost(p, t), the base r_c and b, the candidates k, their targets t_k and admissibility are those of steps 1 - 3
 * of the search block.  p1 <= p2 are the penalties; the bits of `paths` name where the predecessor q of p = (x, y) lies:
 *   1: q = (x-1, y), the path runs left to right      2: q = (x+1, y), right to left
 *   4: q = (x, y-1), top to bottom                     8: q = (x, y+1), bottom to top
 * A pixel is LIVE iff it is valued and has at least one admissible candidate; A(p) is the set of its admissible candidates
 * and c(p, k) = cost(p, t_k).  The displacement of a candidate is d(p, k) = t_k - p: (kx - r_0(p), 0) with C = 1,
 * (r_0(p) + kx, r_1(p) + ky) with C = 2.  The penalty of a difference v of two displacements is V(v) = 0 for v = 0, p1 for
 * max(|v_x|, |v_y|) = 1, p2 otherwise.  For a live p, k in A(p) and a direction with predecessor q:
 *   q inside the image and live:  L(p, k) = c(p, k) + min over j in A(q) of [L(q, j) + V(d(p, k) - d(q, j))]
 *                                                   - min over j in A(q) of L(q, j)
 *   otherwise (the border, a hole, an unmatched pixel alike) the path starts anew:  L(p, k) = c(p, k).
 * The bracket less the minimum lies in [0, p2], so 0 <= L <= 20655 + 32767 < 2^16 and a sum over four paths fits 18 bits.
 * (d(p, k) - d(q, j) depends only on k - j and on the difference of the two bases, so an implementation need look only at
 * the label of equal displacement, its up to 8 (C = 2) or 2 (C = 1) neighbours and the overall minimum, not at all pairs;
 * the plain minimum above is the definition.)
 * S(p, k) is the sum of L over the directions in `paths`; with paths = 0, S(p, k) = c(p, k).
 *   4' best: the admissible candidate with the lexicographically smallest (S, |kx| + |ky|, ky, kx).
 * Steps 5 - 7 of the search block follow unchanged, on the RAW costs around t_best: the parabola, the value, the ceiling, so
 * max_cost and the cost output mean what they mean there.  With paths = 0 (any p1, p2) or p1 = p2 = 0 (any paths) S is a
 * positive multiple of c, and out, cost, choice and stats equal those of gpc_hip_search_fields byte for byte.
 * Outputs; every element of every output is written:
 *   out, cost (c0 of the best, raw), choice, stats[P][4]: exactly as the search block defines them.
 *   agg[P][height][width] uint32 (optional): S of the best candidate, also for a rejected pixel; 0xFFFFFFFF for holes and
 *     unmatched pixels.
 * The refusals of the search block apply; p1, p2 or paths out of range give GPC_E_INVALID.  out == field is allowed and
 * gives the same bytes. */
typedef struct gpc_aggregate {
  int32_t radius, range, subpixel, max_cost;  /* as gpc_search, same ranges                                          */
  int32_t p1, p2;                             /* 0 <= p1 <= p2 <= 32767                                              */
  int32_t paths;                              /* 0 .. 15, the bits above                                             */
} gpc_aggregate;     /* documented defaults: 2, 1, 1, 0xFFFF as gpc_search; p1 = 128, p2 = 512, paths = 15: chosen on
                      * four synthetic scenes (the lowest error over all pixels of a small grid, by a margin of 0.1 %:
                      * DESIGN.md 4.20)                                                                              */
/* A field and its two images already on the device.  A pure function of its arguments: no forest is needed, and the call
 * only queues work on the context's stream (a clear of the stats; per group of pairs one launch for the cost volume, one
 * per orientation of the paths and one for the choice); read the outputs after gpc_hip_synchronize or another wait on the
 * stream.  Workspace, owned by the context and grown on demand: per pixel 2 bytes for each of the (2R+3) (C = 1) or
 * (2R+3)^2 (C = 2) cells of the cost volume and 2 bytes per label and direction for the path values -- 10 + 6 d (C = 1),
 * 50 + 18 d (C = 2) bytes at R = 1 with d directions.  Pairs go through the launches in groups sized to stay within 1 GiB,
 * at least one pair a group; the result does not depend on the grouping. */
int gpc_hip_aggregate_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR,
                                    int channels, int width, int height, int npairs, const gpc_aggregate* prm, int32_t* d_out,
                                    uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats, uint32_t* d_agg);
/* gpc_hip_search_batch_device / gpc_hip_search_sequence_device with this stage in the search's place, over the forward
 * field and, only with check_tol_q8 >= 0, over the backward field with the images exchanged: the same settings, refusals,
 * statuses, waiting, lane draining and group-mode behaviour; d_cost as there. */
int gpc_hip_aggregate_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height,
                                   int npairs, const gpc_settings* settings, int refine_radius, const gpc_densify* fill,
                                   const gpc_aggregate* aggregate, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                                   int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts,
                                   int32_t* d_ncand, uint16_t* d_cost);
int gpc_hip_aggregate_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                      const gpc_settings* settings, int refine_radius, const gpc_densify* fill,
                                      const gpc_aggregate* aggregate, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                                      int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts,
                                      int32_t* d_ncand, uint16_t* d_cost);
/* A host field, images and outputs through gpc_hip_aggregate_fields_device; synchronous, in chunks of at most 16 pairs,
 * pageable arrays through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_aggregate_fields(gpc_hip_ctx* ctx, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels,
                             int width, int height, int npairs, const gpc_aggregate* prm, int32_t* out, uint16_t* cost,
                             uint8_t* choice, int32_t* stats, uint32_t* agg);

/* ---- propagate field values between neighbours --------------------------------------------- */
/* The fill interpolates across object edges, so the prior there is off by many pixels, and the search and the aggregation
 * above look at most `range` <= 2 whole pixels around it: at an edge no choice among their candidates can be right.  The
 * right value usually exists a few pixels away, on the correct side of the edge.  This stage is spatial propagation
 * (PatchMatch; the grid candidates of ELAS): a pixel tries the values of its neighbours as candidates and keeps whichever the
 * two images agree with best.  Run at strides that halve from `span` down to 1, a value travels up to about twice `span` (it
 * must be the best at each pixel it passes through).  The stage sits between the fill and the search, which supplies the
 * sub-pixel part afterwards.  The reference has no counterpart; the rule is made of integers only, so that every
 * implementation of it gives the same bytes.
 *
 * Inputs: as in the search block -- field[P][C][height][width] int32 in 1/256 pixel, C = 1 or 2, imgL and imgR
 *   [P][height][width] uint8.  The hole test (F_0 is GPC_DENSE_NONE), the rounding r_c = sgn(F_c) * ((|F_c| + 128) >> 8) in 64
 *   bits, and cost(p, t) with clamped addresses are exactly steps 1 and 2 of the search block.  r = radius, N = iterations.
 * Iterations: iteration i = 0 .. N-1 has the stride s_i = max(1, span >> i).  It reads ONLY the field that iteration i-1
 *   wrote (iteration 0 reads the input) and writes a whole new field: a Jacobi step -- no pixel sees a value written in the
 *   same iteration, so the result does not depend on any order of execution.
 * Per pixel p = (x, y) of iteration i, s = s_i:
 *   1 a hole stays a hole, and every channel is copied as it is.
 *   2 candidate sources, in this fixed order, with index j:  0: p itself   1: (x - s, y)   2: (x + s, y)   3: (x, y - s)
 *     4: (x, y + s)   and with neighbours = 8:  5: (x - s, y - s)   6: (x + s, y - s)   7: (x - s, y + s)   8: (x + s, y + s).
 *     A source outside the image gives no candidate (it is not clamped).  A source that is a hole gives no candidate.
 *   3 candidate j with source q has the whole-pixel displacement r(q): its target is t = (x - r_0(q), y) with C = 1 and
 *     t = (x + r_0(q), y + r_1(q)) with C = 2.  It is ADMISSIBLE iff t lies inside the image.
 *   4 the winner is the admissible candidate with the lexicographically smallest (cost(p, t), j): on equal cost the pixel's
 *     own value wins, then the fixed order.  (A candidate with the same displacement as an earlier one has the same cost and
 *     can never win; an implementation may skip it.)
 *   5 the value written: if j = 0 wins, every channel of p unchanged, sub-pixel bits included; if j > 0 wins, 256 * r_c(q) in
 *     every channel (admissibility bounds |r_c| by the image size, so this cannot overflow); if no candidate is admissible
 *     the pixel is UNMATCHED and its channels are copied unchanged.  The stage replaces values and never removes one.
 * Outputs; every element of every output is written:
 *   out[P][C][height][width]: the field after iteration N-1.  out == field (the same pointer) is allowed and gives the same
 *     bytes.
 *   cost[P][height][width] uint16 (optional): the winner's cost in the LAST iteration; 0xFFFF for holes and unmatched pixels.
 *   choice[P][height][width] uint8 (optional): the winner's j in the last iteration; 255 for holes and unmatched pixels.
 *   stats[P][N][4] int32 (optional), per iteration: the numbers of pixels that kept their own value, holes, unmatched pixels
 *     and pixels moved to a neighbour's value.
 * The refusals and limits of the search block apply; a parameter out of its range gives GPC_E_INVALID.  out may not overlap
 * the images, and may not overlap field other than being it. */
typedef struct gpc_propagate {
  int32_t radius;      /* r, 1 .. 4: the window is (2 r + 1)^2                                  */
  int32_t span;        /* 1 .. 64: the stride of the first iteration                            */
  int32_t iterations;  /* N, 1 .. 16                                                            */
  int32_t neighbours;  /* 4 or 8                                                                */
} gpc_propagate;       /* documented defaults: 2, 1, 6, 8 -- the point of a small grid with the lowest error over
                        * all pixels after propagate -> search on four synthetic scenes  */
/* A field and its two images already on the device.  A pure function of its arguments: no forest is needed, and the call
 * only queues work on the context's stream (a clear of the stats, with out == field and an odd N one copy of the field, and
 * N launches whatever the data); read the outputs after gpc_hip_synchronize or another wait on the stream.  Workspace, owned
 * by the context and grown on demand: one field's bytes (none with N = 1 and out apart from field). */
int gpc_hip_propagate_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR,
                                    int channels, int width, int height, int npairs, const gpc_propagate* prm, int32_t* d_out,
                                    uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats);
/* A host field, images and outputs through gpc_hip_propagate_fields_device; synchronous, in chunks of at most 16 pairs,
 * pageable arrays through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_propagate_fields(gpc_hip_ctx* ctx, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels,
                             int width, int height, int npairs, const gpc_propagate* prm, int32_t* out, uint16_t* cost,
                             uint8_t* choice, int32_t* stats);

/* ---- close holes along scanlines from the background side ----------------------------------- */
/* The cleaner takes out the occluded band beside a foreground object, and the completion below fills it with a weighted
 * mean of both sides of the edge: wrong for every pixel of an occlusion, whatever the weights.  This stage is a choice, not
 * a mean (the gap interpolation of ELAS, the occlusion filling of SGM): along the scanline through a hole, look at the two
 * valued ends of its run of holes; where they agree, interpolate between them; where they disagree the run is a depth edge,
 * and the hole takes the background end.  The stage sits between the cleaner and the completion, which then only closes
 * what is left.  The reference has no counterpart; the rule is made of integers only, so that every implementation of it
 * gives the same bytes.
 *
 * Inputs: P = npairs fields field[P][C][height][width] int32 in 1/256 pixel, C = 1 or 2; optionally guide[P][height][width]
 *   uint8 (required with select = 1).  A pixel is a HOLE iff F_0 is GPC_DENSE_NONE, whatever F_1 holds; every other pixel
 *   is VALUED, and any int32 in F_1 is a value.  All arithmetic is done in 64 bits: nothing is undefined for INT32_MAX or
 *   INT32_MIN + 1.
 * Runs: the RUN of a hole p along an axis (horizontal, vertical) is the maximal line of consecutive holes through p in the
 *   INPUT field; its length is n; its ends are the pixels just before its first and just after its last hole.  An end is a
 *   valued pixel or lies outside the image.  da and db are p's distances to the first (left / upper) end A and to the second
 *   end B: da + db = n + 1.
 * An axis is USABLE for p iff n <= max_gap and either both ends are valued (CLOSED) or exactly one is and border = 1
 *   (HALF-OPEN).
 * The axis's candidate:
 *   half-open: the valued end's value.  Kind BORDER.
 *   closed with |A_c - B_c| <= discon_q8 in every channel: kind CONTINUOUS.  S_c = A_c * db + B_c * da, N = da + db, and
 *     the value is sgn(S_c) * ((2 |S_c| + N) div (2 N)): the fill's rounding, half away from zero; the nearer end weighs
 *     more.
 *   closed otherwise: kind DISCONTINUOUS.  The value is one end's, with all its channels.  m(E) = sum over c of E_c^2 in
 *     unsigned 64 bits, g(E) = |I(p) - I(E)| in the guide.  select = 0 (background): the end with the smaller (m, distance
 *     to p), on equality A -- for a disparity of either sign the farther surface, for a flow the slower one (a stated
 *     heuristic).  select = 1 (guide): the end with the smaller (g, m, distance), on equality A.
 * Between the axes: p takes the candidate of the usable axis with the shorter run, on equal length the horizontal one.  A
 *   hole with no usable axis stays a hole.  Valued pixels never change.  No filled value is ever read: every end is a
 *   pixel valued on input.
 * Outputs; every element of every output is written:
 *   out[P][C][height][width]; a hole that is left gets GPC_DENSE_NONE in every channel.  out == field (the same pointer) is
 *     allowed and gives the same bytes; any other overlap of out with field or with the guide is GPC_E_INVALID.
 *   how[P][height][width] uint8 (optional): 0 valued on input; 1 / 2 / 3 horizontal continuous / discontinuous / border;
 *     4 / 5 / 6 the same, vertical; 255 a hole that is left.
 *   stats[P][4] int32 (optional): pixels filled continuous, filled discontinuous, filled border, holes left.
 * GPC_E_INVALID: a parameter out of its range, channels not 1 or 2, a null required pointer, select = 1 without a guide,
 * width, height or npairs below 1.  GPC_E_UNSUPPORTED: the limits of the densify block (32768, 2^30, 65535). */
typedef struct gpc_gapfill {
  int32_t max_gap;   /* 1 .. 32767: the longest run an axis may close                          */
  int32_t discon_q8; /* 0 .. 2^24: ends further apart than this in a channel are a depth edge  */
  int32_t select;    /* 0 background, 1 guide                                                  */
  int32_t border;    /* 0 or 1: half-open runs are usable                                      */
} gpc_gapfill;       /* 16 bytes.  Documented defaults: 64, 128, 0, 1 -- the point of a grid with the lowest error over all
                      * pixels after gapfill -> complete on four synthetic scenes           */
/* A field (and a guide) already on the device.  A pure function of its arguments: no forest is needed, and the call only
 * queues work on the context's stream (a clear of the stats and three launches whatever the data); read the outputs after
 * gpc_hip_synchronize or another wait on the stream.  Workspace, owned by the context and grown on demand: four planes of
 * uint16 distances, 8 bytes per pixel and pair.  d_guide may be null with select = 0. */
int gpc_hip_gapfill_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, const uint8_t* d_guide, int channels, int width,
                                  int height, int npairs, const gpc_gapfill* prm, int32_t* d_out, uint8_t* d_how,
                                  int32_t* d_stats);
/* A host field, guide and outputs through gpc_hip_gapfill_fields_device; synchronous, in chunks of at most 16 pairs,
 * pageable arrays through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_gapfill_fields(gpc_hip_ctx* ctx, const int32_t* field, const uint8_t* guide, int channels, int width, int height,
                           int npairs, const gpc_gapfill* prm, int32_t* out, uint8_t* how, int32_t* stats);

/* ---- complete cleaned dense fields, guided by the image ------------------------------------ */
/* The cleaner's output is a field with holes: failed checks (occlusions, halos), speckles, and whatever the fill never
 * valued.  This stage closes them by an edge-aware completion: a hole takes the weighted mean of the valued pixels around
 * it, and neighbours that look like it in the image count more, so that occluded background is filled from background.  The
 * hierarchical fill cannot do it: it fills from records, not from a field, and averages across object edges.  The
 * reference has no counterpart; the rule is this library's own, made of integers only, so that every implementation of it
 * gives the same bytes.
 *
 * Input: P = npairs fields field[P][C][height][width] int32 as gpc_hip_densify_* and gpc_hip_clean_* write them, C =
 *   channels: 1 or 2, and a guide guide[P][height][width] uint8: the raw left image, or frame t.  A pixel p is a HOLE iff
 *   F_0(p) is GPC_DENSE_NONE, whatever F_1 holds; every other pixel is VALUED.  I(p) is the guide at p.
 * Weight of neighbour q for pixel p: w(p, q) = 256 >> min(8, |I(p) - I(q)| >> range_shift): 1 .. 256, never 0; with
 *   range_shift = 8 it is 256 always (unguided).
 * Passes k = 1 .. passes.  State F(k) is a function of F(k-1) only (F(0) is the input): no value filled in pass k is read
 *   in pass k.  For a hole p of F(k-1), Q is the set of valued pixels of F(k-1) in p's (2 radius + 1)^2 window clipped to
 *   the image; Wt = sum over Q of w(p, q) and S_c = sum over Q of w(p, q) * F_c(q), both exact in 64 bits (no int32 input
 *   can overflow them: |S| < 2^31 * 2^8 * 289 < 2^49).  If Wt >= min_weight, p becomes valued with sgn(S_c) * ((2 |S_c| +
 *   Wt) div (2 Wt)) in channel c -- the fill's rounding, half away from zero -- and its pass number is k; otherwise it
 *   stays a hole.  Valued pixels never change.
 * Outputs; every element of every output is written:
 *   out[P][C][height][width]: F(passes); a hole gets GPC_DENSE_NONE in every channel (also a hole of the input whose F_1
 *     held something else).
 *   pass[P][height][width] uint8 (optional): 0 for a pixel valued on input, k for a pixel filled in pass k, 255 for a pixel
 *     left a hole.
 *   stats[P][2] int32 (optional): pixels filled, holes left.
 * out == field (the same pointer) is allowed and gives the same bytes; any other overlap of out with field is
 * GPC_E_INVALID, as are a parameter out of range, channels not 1 or 2, a null required pointer (field, guide, out, prm),
 * width, height or npairs < 1.  GPC_E_UNSUPPORTED: width or height > 32768, width * height > 2^30, npairs > 65535 (the
 * limits of the densify block).  Once a pass fills nothing, or no hole is left, later passes change nothing: an
 * implementation skips them, and tiles without holes, unobservably. */
typedef struct gpc_inpaint {
  int32_t radius;      /* 1 .. 8: the window is (2 r + 1)^2, clipped to the image              */
  int32_t range_shift; /* 0 .. 8: the weight halves per 2^range_shift grey levels; 8 = unguided */
  int32_t min_weight;  /* 1 .. 2^24: total weight a hole needs before it is filled              */
  int32_t passes;      /* 1 .. 254                                                              */
} gpc_inpaint;         /* documented defaults: 4, 3, 512, 32 -- a choice, not a measurement     */
/* A field and a guide already on the device.  A pure function of its arguments: no forest is needed, and the call only
 * queues work on the context's stream (two small clears, one launch that starts out and the pass plane, one launch per
 * pass, in place in d_out; a pass with nothing left to do finds that out on the device -- the host reads no count and
 * does not wait); read the outputs after gpc_hip_synchronize or another wait on the stream.  Workspaces of the context,
 * grown on demand: 1 byte per pixel and pair for the pass plane (d_pass itself where it is given), and 4 bytes per 32x32
 * tile and pair plus 1 KiB + 8 bytes per pair of control words. */
int gpc_hip_inpaint_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, const uint8_t* d_guide, int channels, int width,
                                  int height, int npairs, const gpc_inpaint* prm, int32_t* d_out, uint8_t* d_pass,
                                  int32_t* d_stats);
/* Match, refine, fill, flip, fill again, clean, complete: exactly gpc_hip_clean_batch_device / gpc_hip_clean_sequence_device
 * -- the same settings, refusals, statuses, waiting, lane draining and group-mode behaviour -- then
 * gpc_hip_inpaint_fields_device over the cleaned field, guided by d_rawL (batch) or by frame t for pair t (sequence).
 * d_out (required) receives the completed field; d_pass and d_fill_stats (optional) are the pass plane and the stats of
 * the completion; d_cleaned [P][C][height][width] (optional) receives the cleaned field before completion (it may not
 * overlap d_out unless it is d_out, nor d_fwd); every other argument is the clean form's, d_state, d_label and d_stats
 * describing the cleaned field.  Without d_cleaned the cleaner writes d_out and the completion runs in place: no
 * workspace beyond those of the calls it is made of. */
int gpc_hip_inpaint_batch_device(gpc_hip_ctx* ctx, const uint8_t* d_rawL, const uint8_t* d_rawR, int width, int height, int npairs,
                                 const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_clean* prm,
                                 const gpc_inpaint* inpaint, int32_t* d_out, uint8_t* d_pass, int32_t* d_fill_stats,
                                 int32_t* d_cleaned, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                                 uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
int gpc_hip_inpaint_sequence_device(gpc_hip_ctx* ctx, const uint8_t* d_frames, int width, int height, int nframes,
                                    const gpc_settings* settings, int refine_radius, const gpc_densify* fill, const gpc_clean* prm,
                                    const gpc_inpaint* inpaint, int32_t* d_out, uint8_t* d_pass, int32_t* d_fill_stats,
                                    int32_t* d_cleaned, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                                    uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand);
/* A host field, guide and outputs through gpc_hip_inpaint_fields_device; synchronous, in chunks of at most 16 pairs, pageable
 * arrays through the context's page-locked arena.  What comes back equals the device form byte for byte. */
int gpc_hip_inpaint_fields(gpc_hip_ctx* ctx, const int32_t* field, const uint8_t* guide, int channels, int width, int height,
                           int npairs, const gpc_inpaint* prm, int32_t* out, uint8_t* pass, int32_t* stats);

/* ---- score dense fields against ground truth ------------------------------------------------ */
/* How good a field is, as exact counts per pair: end-point error, the share of pixels within a few pixels of truth, the
 * KITTI outlier rate (D1 for a disparity, Fl for a flow), the density, and all of it split by an occlusion class or by the
 * speed of the true motion, as Sintel and KITTI report it.  gpc_hip_score_* above judges sparse records and cannot take a
 * field; this block judges what gpc_hip_densify_*, gpc_hip_search_*, gpc_hip_clean_* and gpc_hip_inpaint_* write, where it
 * lies.  The rule uses integers only, so that every implementation of it gives the same bytes.  The library returns counts
 * only; rates are the caller's divisions.
 *
 * Input: P = npairs fields field[P][C][height][width] int32 in 1/256 pixel as gpc_hip_densify_* writes them, C = channels: 1
 *   for a disparity, 2 for u then v; a gpc_truth (above): u[P][height][width] float, v likewise (it must be NULL with C = 1
 *   and is required with C = 2), ignore[P][height][width] uint8 (optional); cls[P][height][width] uint8 (optional).
 * A pixel is, in this order:
 *   1 IGNORED: ignore is given and nonzero at the pixel.
 *   2 NO TRUTH: a truth value that is read (u; also v with C = 2) is not finite or its absolute value exceeds 32768 (the
 *     image-size limit; the .flo "unknown" sentinel 1e9 lies beyond it).
 *   3 HOLE: F_0 is GPC_DENSE_NONE, whatever F_1 holds (the rule of the search block).
 *   4 JUDGED: every other pixel.
 * Error of a judged pixel, all arithmetic in 64 bits:
 *   t_c = llrintf(256.f * truth_c): the product is exact, the rounding to nearest, ties to even (KITTI's truth is in 1/256
 *     pixel exactly); |t_c| <= 2^23.
 *   d_c = (int64)F_c - t_c, with C = 1 as with C = 2: a disparity field holds 256 d and the truth g is a disparity.
 *   a_c = min(|d_c|, 65536); a_1 = 0 with C = 1.
 *   e2 = min(a_0^2 + a_1^2, 2^32); e = isqrt(e2), the exact floor of the square root.
 *   Errors beyond 256 pixels are clamped; a clamped pixel lies within no threshold because thr_q8 <= 65535.  Nothing is
 *   undefined for INT32_MAX, INT32_MIN + 1 or an F_1 that is GPC_DENSE_NONE.
 * Tallies over judged pixels (gpc_field_tally): n_judged; n_within[k] counts e2 <= thr_q8[k]^2 (entries at k >= n_thr are
 *   0); sum_e_q8 sums e; sum_e2_q16 sums e2; n_outlier counts e2 > out_abs_q8^2 and e2 * 10^6 > m2 * out_rel_pm^2 with m2 =
 *   t_0^2 + t_1^2 (both sides fit uint64: out_rel_pm is per mille and at most 255).  KITTI's rule is out_abs_q8 = 768,
 *   out_rel_pm = 50; out_rel_pm = 0 is the absolute test alone.
 * Bin of a judged pixel: with cls, min(cls, 3); otherwise the number of k < n_speed with m2 >= speed_q8[k]^2 (speed_q8
 *   ascending; Sintel's s0-10 / s10-40 / s40+ is {2560, 10240}); with neither, bin 0.
 * Identities: n_pixels = width * height = n_ignored + n_no_truth + n_hole + all.n_judged, and `all` equals the elementwise
 *   sum of the four bins.
 * err[P][height][width] uint16 (optional): min(e, 0xFFFE) for a judged pixel, 0xFFFF for every other; every element is
 *   written.
 * GPC_E_INVALID: a parameter out of range (of thr_q8 and speed_q8 the entries in use are looked at), reserved not 0, a null
 * required pointer (field, truth, truth->u, prm, scores), channels not 1 or 2, truth->v given with C = 1 or missing with
 * C = 2, width, height or npairs < 1.  GPC_E_UNSUPPORTED: width or height > 32768, width * height > 2^30, npairs > 65535
 * (the limits of the densify block).  No alignment is required beyond each type's own, unlike gpc_hip_score_batch_device. */
typedef struct gpc_field_score_prm {
  int32_t n_thr;        /* 0 .. 8: thresholds in use                                                     */
  int32_t thr_q8[8];    /* 0 .. 65535 each, in 1/256 pixel                                               */
  int32_t out_abs_q8;   /* 0 .. 65535: an outlier's error exceeds this ...                               */
  int32_t out_rel_pm;   /* 0 .. 255: ... and this many per mille of the true magnitude; 0 = absolute only */
  int32_t n_speed;      /* 0 .. 3: speed bounds in use (only without cls)                                */
  int32_t speed_q8[3];  /* 0 .. 2^23 each, ascending, in 1/256 pixel                                     */
  int32_t reserved;     /* must be 0                                                                     */
} gpc_field_score_prm;  /* documented defaults: n_thr 3, thr_q8 {256, 768, 1280}, out 768 / 50, n_speed 0 */
typedef struct gpc_field_tally {  /* every field an exact count or sum over judged pixels */
  int64_t n_judged;
  int64_t n_within[8];
  int64_t n_outlier;
  int64_t sum_e_q8;
  int64_t sum_e2_q16;
} gpc_field_tally;                /* 96 bytes */
typedef struct gpc_field_score {  /* one per pair */
  int64_t n_pixels;
  int64_t n_ignored;
  int64_t n_no_truth;
  int64_t n_hole;
  gpc_field_tally all;
  gpc_field_tally bin[4];
} gpc_field_score;                /* 512 bytes */
/* Fields, truth and class plane already on the device (truth holds device pointers).  A pure function of its arguments: no
 * forest and no workspace are needed, and the call only queues work on the context's stream (a clear of d_scores, one
 * launch); read d_scores[npairs] and d_err after gpc_hip_synchronize or another wait on the stream.  The kernel has no
 * timing slot (the slot table is closed): time it with events on the stream. */
int gpc_hip_score_fields_device(gpc_hip_ctx* ctx, const int32_t* d_field, int channels, int width, int height, int npairs,
                                const gpc_truth* truth, const gpc_field_score_prm* prm, const uint8_t* d_cls,
                                gpc_field_score* d_scores, uint16_t* d_err);
/* Host fields, truth (host pointers), class plane, scores and error plane through gpc_hip_score_fields_device; synchronous,
 * in chunks of at most 16 pairs, pageable arrays through the context's page-locked arena.  What comes back equals the device
 * form byte for byte. */
int gpc_hip_score_fields(gpc_hip_ctx* ctx, const int32_t* field, int channels, int width, int height, int npairs,
                         const gpc_truth* truth, const gpc_field_score_prm* prm, const uint8_t* cls, gpc_field_score* scores,
                         uint16_t* err);

/* ---- measurement -------------------------------------------------------------- */
/* Per-kernel HIP-event timing on the context's stream.  When enabled every launch of
 * the named kernels is bracketed by hipEvents; gpc_hip_kernel_time returns the summed
 * milliseconds and launch count since the last reset (synchronises the stream). */
int gpc_hip_enable_kernel_timing(gpc_hip_ctx* ctx, int enable);
/* Restrict the bracketing to the kernels whose index bit is set (default: all).  Every pair of
 * event records costs a little stream time, so a benchmark times only the kernel it reports.  The mask has 32 bits and
 * gpc_hip_kernel_count() is the number of slots it addresses (at most 32).  gpc_hip_kernel_slots() counts every slot:
 * those from gpc_hip_kernel_count() on (k_search, k_refine, k_pyr_*, k_dense_*, k_tf_*, k_inpaint_*, k_quad_*, k_clean_*) are bracketed whenever timing is enabled, and gpc_hip_kernel_name,
 * gpc_hip_kernel_launch_name and gpc_hip_kernel_time take their indices like any other. */
int gpc_hip_set_kernel_timing_mask(gpc_hip_ctx* ctx, unsigned mask);
int gpc_hip_reset_kernel_timing(gpc_hip_ctx* ctx);
int gpc_hip_kernel_count(void);
int gpc_hip_kernel_slots(void);
const char* gpc_hip_kernel_name(int index);
/* The profiler's (rocprofv3) name of the template instantiation this context last launched under timing slot
 * `index`, e.g. "gpc::k_row_join<4, 256, false>"; "" before the first launch.
 * The slot "k_global_match" names the join launches of the last device-wide match (non-epipolar or hash table) in
 * launch order: " + " between two launches, "[list]" behind a launch whose grid was the planner's work list, e.g.
 * "gpc::k_row_join<8, 1024, false, true>[list] + gpc::k_row_join<4, 1024, false, true>", "gpc::k_ht_join<4, 512>";
 * the radix-sort fallbacks read "gpc::k_g_match" and "gpc::k_ht_pairs". */
const char* gpc_hip_kernel_launch_name(const gpc_hip_ctx* ctx, int index);
int gpc_hip_kernel_time(gpc_hip_ctx* ctx, int index, float* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* GPC_HIP_H */
