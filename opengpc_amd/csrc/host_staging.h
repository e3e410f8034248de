// host_staging.h -- what scoring, tracks, filtering, refinement and densifying share: every record of a call kept on the
// device (AllRecords, all_records), the batch match with the lanes off (match_batch_strict), and Stage, the host
// forms' one staging block.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// (the context, ensure, the lanes, the transfer arena, match_usable); the device forms it calls are declared by the C header.
#pragma once

namespace {

// Every record of every pair of a call, kept on the device: what match-and-score and match-and-filter work on.  A group has
// at most one record per left candidate, a union at most G.
struct AllRecords {
  void* rec;        // [npairs][cap]: gpc_support of pairs, gpc_correspondence of frames
  int32_t* counts;  // [npairs]
  int cap;
};
// lanes = 1 for the duration of the match: it runs on the context itself
struct StrictScope {
  gpc_hip_ctx* c;
  int lanes;
  explicit StrictScope(gpc_hip_ctx* ctx) : c(ctx), lanes(ctx->pipeline) { c->pipeline = 1; }
  ~StrictScope() { c->pipeline = lanes; }
};

// what the match itself refuses is refused here, and a capacity that does not fit an int, before any workspace is made
int all_records_cap(gpc_hip_ctx* c, const gpc_settings* s, int W, int H, bool seq, int* cap) {
  CHK(match_usable(c, s, W, H, seq));
  const long n = (long)(c->ngroups > 1 ? c->ngroups : 1) * (W - 2 * GPC_R) * (H - 2 * GPC_R) + 1;
  if (n > 0x7FFFFFFFl) return GPC_E_UNSUPPORTED;
  *cap = (int)n;
  return GPC_OK;
}

// The plain batch match with the lanes off for the duration of the call: it runs on the context itself.  The caller has
// drained the lanes where they are on.
int match_batch_strict(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                       const gpc_settings* s, gpc_support* d_out, int cap_per_pair, int32_t* d_counts, int32_t* d_ncand) {
  StrictScope strict(c);
  return gpc_hip_match_batch_device(c, d_rawL, d_rawR, W, H, npairs, s, d_out, cap_per_pair, d_counts, d_ncand);
}

// d_b null: d_a holds npairs + 1 frames; else d_a and d_b hold the left and right images of npairs pairs.  r->cap is what
// all_records_cap gave for the call (filtering checks its own limits against it in between)
int all_records(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s,
                int32_t* d_ncand, AllRecords* r) {
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));
  CHK(ensure(c, c->all_rec, (d_b ? sizeof(gpc_support) : sizeof(gpc_correspondence)) * (size_t)r->cap * npairs));
  CHK(ensure(c, c->all_cnt, sizeof(int32_t) * (size_t)npairs));
  r->rec = c->all_rec.p;
  r->counts = (int32_t*)c->all_cnt.p;
  if (!d_b) return gpc_hip_match_sequence_device(c, d_a, W, H, npairs + 1, s, (gpc_correspondence*)r->rec, r->cap, r->counts, d_ncand);
  return match_batch_strict(c, d_a, d_b, W, H, npairs, s, (gpc_support*)r->rec, r->cap, r->counts, d_ncand);
}

// Host forms of scoring, tracks and filtering: lay out -> upload -> device form -> download, over ONE device block
// (c->stage) that a call lays out anew: every host form waits for its stream before it returns, so no two are live together.
//   layout:   in() and out() name the regions in order, each on a 16-byte boundary; alloc() then grows the block once.
//   upload:   page-locked arrays (gpc_hip_host_alloc) are read where they lie.  Pageable ones pass through the page-locked
//             arena (host_copy) in pieces of at most 32 MiB, two of them where one does not hold the regions a call (a
//             chunk) uploads: a piece is written again only when the copies that read it are done (its event, or
//             wait()).  Two, so that a scoring chunk above 32 MiB (16 pairs of 1024x436 with flow truth: 65 MB) still
//             goes up without the host waiting for the device, as it did when scoring reserved a chunk's whole size;
//             tracks and filtering, which had one piece and a wait behind every copy, now hold up to 64 MiB page-locked.
//             in_bytes counts a records region in full, so two pieces may be reserved where the valid records fit one.
//             Tracks and filtering send only the valid records of a pair (up_records).
//   download: small per-pair words land in the page-locked h_cnt and are copied out after the wait; per-pair arrays go to
//             the caller's arrays as they are, clipped to what the device form wrote, so every other byte there stays.
// Scoring goes in chunks of at most 16 pairs (frames: GPC_HIP_SEQ_FRAMES, consecutive chunks share one), one wait per chunk;
// tracks stage the whole call, since links cross pairs; filtering goes in chunks of at most 16 pairs.
struct Stage {
  gpc_hip_ctx* c;
  size_t bytes = 0, in_bytes = 0;  // the block; its regions that are uploaded
  size_t piece = 0, at = 0;        // the arena of this call's pageable uploads: one or two pieces; the fill of the current one
  int pieces = 0, cur = 0;
  bool busy[2] = {false, false};   // copies queued since the last wait() may still read the piece: e_stage[k] says when they are done
  explicit Stage(gpc_hip_ctx* ctx) : c(ctx) {}
  size_t out(size_t n) {
    const size_t region = bytes;
    bytes += pad16(n);
    return region;
  }
  size_t in(size_t n) {
    in_bytes += pad16(n);
    return out(n);
  }
  int alloc(size_t word_bytes) {  // word_bytes: what the call lands in h_cnt at a time
    CHK(ensure(c, c->stage, bytes));
    return pinned_area(c, word_bytes);
  }
  uint8_t* p(size_t region) const { return (uint8_t*)c->stage.p + region; }
  int wait() {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    at = 0;
    busy[0] = busy[1] = false;
    return GPC_OK;
  }
  int next_piece() {  // the other piece (where there is one) is filled while the copies out of this one run
    HIPCHK(c, hipEventRecord(c->e_stage[cur], c->stream));
    busy[cur] = true;
    cur = (cur + 1) % pieces;
    at = 0;
    if (busy[cur]) HIPCHK(c, hipEventSynchronize(c->e_stage[cur]));
    busy[cur] = false;
    return GPC_OK;
  }
  int copy_up(size_t region, const uint8_t* src, size_t n, bool pinned) {
    if (pinned && n) HIPCHK(c, hipMemcpyAsync(p(region), src, n, hipMemcpyHostToDevice, c->stream));
    if (pinned || !n) return GPC_OK;
    if (!piece) {  // (once per call)
      piece = std::min(std::max(in_bytes, pad16(n)), (size_t)32 << 20);
      pieces = in_bytes > piece ? 2 : 1;
      uint8_t* d_arena = nullptr;
      CHK(xfer_reserve(c, pieces * piece, &d_arena));
      CHK(ensure_pool(c));
      for (int k = 0; k < pieces; ++k)
        if (!c->e_stage[k]) HIPCHK(c, c->e_stage[k].create(hipEventDisableTiming));
    }
    for (size_t done = 0; done < n;) {
      if (at == piece) CHK(next_piece());
      const size_t nb = std::min(n - done, piece - at);
      uint8_t* h = c->h_xfer.p + cur * piece + at;
      host_copy(c, h, src + done, nb, true);
      host_copy_wait(c);
      HIPCHK(c, hipMemcpyAsync(p(region) + done, h, nb, hipMemcpyHostToDevice, c->stream));
      at += pad16(nb);
      done += nb;
    }
    return GPC_OK;
  }
  int up(size_t region, const void* src, size_t n) { return copy_up(region, (const uint8_t*)src, n, device_view_of_host(src) != nullptr); }
  // pairs [p0, p0 + pc) of src [..][cap] records of esz bytes -> region [pc][cap]: what lies beyond a pair's count is never read
  int up_records(size_t region, const void* src, size_t esz, int cap, const int32_t* counts, int p0, int pc) {
    const bool pinned = device_view_of_host(src) != nullptr;
    for (int t = 0; t < pc; ++t)
      CHK(copy_up(region + esz * (size_t)t * cap, (const uint8_t*)src + esz * (size_t)(p0 + t) * cap,
                  esz * (size_t)valid_records(counts[p0 + t], cap), pinned));
    return GPC_OK;
  }
  // (a pageable dst is written as it is, not through the arena as the note at h_xfer has it: that would be decided here)
  int down(void* dst, size_t region, size_t n) {
    HIPCHK(c, hipMemcpyAsync(dst, p(region), n, hipMemcpyDeviceToHost, c->stream));
    return GPC_OK;
  }
};

}  // namespace
