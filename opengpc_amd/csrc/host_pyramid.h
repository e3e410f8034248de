// host_pyramid.h -- matching over an image pyramid: downsampling, the per-level matches and their merge, host forms.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h (StrictScope and Stage).
#pragma once

namespace {

static_assert(GPC_MAX_PYRAMID_LEVELS == 4, "a block is at most 8 bits of one plane word (k_pyramid.h)");

// one downsampling step over nimages images already on the device
int pyr_down(gpc_hip_ctx* c, const uint8_t* d_src, int W, int H, int nimages, uint8_t* d_dst) {
  const dim3 grid((W / 8 + PY_DOWN_COLS - 1) / PY_DOWN_COLS, (H / 2 + PY_DOWN_ROWS - 1) / PY_DOWN_ROWS, nimages);
  {
    Timed t(c, KID_PYR_DOWN);
    hipLaunchKernelGGL(gpc::k_pyr_down, grid, dim3(PY_DOWN_COLS * PY_DOWN_ROWS), 0, c->stream, d_src, W, H, d_dst);
  }
  snprintf(c->launch_name[KID_PYR_DOWN], sizeof c->launch_name[0], "gpc::k_pyr_down");
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// The merge over records on the device: d_rec[l] = [npairs][caps[l]] unmapped level-l records, d_cnt[l] their counts.
template <bool CORR>
int pyr_merge(gpc_hip_ctx* c, const void* const* d_rec, const int32_t* caps, const int32_t* const* d_cnt, int W, int H,
              int npairs, int levels, void* d_out, int cap, int32_t* d_counts, int32_t* d_level_counts) {
  if (!c || !d_rec || !d_cnt || !d_out || !d_counts || !d_level_counts) return GPC_E_INVALID;
  CHK(gpc::pyr_merge_check(W, H, npairs, levels, caps, cap));
  for (int l = 0; l < levels; ++l)
    if (!d_rec[l] || !d_cnt[l]) return GPC_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  const int wpr = (W + 31) / 32;
  int most = 0;
  for (int l = 0; l < levels; ++l) most = std::max(most, (caps[l] + PY_CHUNK - 1) / PY_CHUNK);
  CHK(ensure(c, c->py_plane, sizeof(uint32_t) * (size_t)wpr * H * npairs));
  CHK(ensure(c, c->py_flags, sizeof(uint64_t) * (PY_CHUNK / 64) * (size_t)most * npairs));
  CHK(ensure(c, c->py_blk, sizeof(int32_t) * (size_t)most * npairs));
  uint32_t* plane = (uint32_t*)c->py_plane.p;
  unsigned long long* flags = (unsigned long long*)c->py_flags.p;
  int32_t* blk = (int32_t*)c->py_blk.p;
  if (levels > 1) HIPCHK(c, hipMemsetAsync(plane, 0, sizeof(uint32_t) * (size_t)wpr * H * npairs, c->stream));
  const int stride = (int)(sizeof(gpc::PyRec<CORR>) / sizeof(int32_t));
  for (int l = 0; l < levels; ++l) {
    const int nchunk = (caps[l] + PY_CHUNK - 1) / PY_CHUNK;
    const dim3 grid(nchunk, npairs);
    {
      Timed t(c, KID_PYR_KEEP);
      hipLaunchKernelGGL(gpc::k_pyr_keep, grid, dim3(PY_THREADS), 0, c->stream, (const int32_t*)d_rec[l], stride, (long)caps[l],
                         d_cnt[l], l, W >> l, H >> l, (const uint32_t*)plane, wpr, H, flags, blk, nchunk);
    }
    {
      Timed t(c, KID_PYR_SCAN);
      hipLaunchKernelGGL(gpc::k_pyr_scan, dim3(npairs), dim3(nchunk >= 1024 ? 1024 : 64 * ((nchunk + 63) / 64)), 0, c->stream, blk,
                         nchunk, l == 0 ? 1 : 0, d_level_counts + (size_t)l * npairs, d_counts);
    }
    {
      Timed t(c, KID_PYR_WRITE);
      hipLaunchKernelGGL((gpc::k_pyr_write<CORR>), grid, dim3(PY_THREADS), 0, c->stream, (const gpc::PyRec<CORR>*)d_rec[l],
                         (long)caps[l], l, W >> l, H >> l, (const unsigned long long*)flags, (const int32_t*)blk, nchunk,
                         (gpc::PyRec<CORR>*)d_out, (long)cap, plane, wpr, H, l + 1 < levels ? 1 : 0);
    }
    HIPCHK(c, hipGetLastError());
  }
  snprintf(c->launch_name[KID_PYR_KEEP], sizeof c->launch_name[0], "gpc::k_pyr_keep");
  snprintf(c->launch_name[KID_PYR_SCAN], sizeof c->launch_name[0], "gpc::k_pyr_scan");
  snprintf(c->launch_name[KID_PYR_WRITE], sizeof c->launch_name[0], "gpc::k_pyr_write<%s>", CORR ? "true" : "false");
  return GPC_OK;
}

// The forest counts as one of a level's size while that level is matched: its tests are offsets within the 27x27 patch
// (GpcForestDev holds no width), so they apply to an image of any size; what the context remembers of the forest (its
// size, its source, the generation of the codes) is what it was when the scope ends.
struct LevelScope {
  gpc_hip_ctx* c;
  int w, h;
  LevelScope(gpc_hip_ctx* ctx, int W, int H) : c(ctx), w(ctx->forest_w), h(ctx->forest_h) {
    c->forest_w = W;
    c->forest_h = H;
  }
  ~LevelScope() {
    c->forest_w = w;
    c->forest_h = h;
  }
};

// what a pyramid call refuses, before any workspace is made; ws / hs: the levels' sizes
int pyr_usable(gpc_hip_ctx* c, const gpc_settings* s, int W, int H, int levels, int32_t* ws, int32_t* hs) {
  CHK(check_settings(s));
  CHK(gpc::pyr_levels(W, H, levels, ws, hs));
  CHK(forest_matches(c, W, H));
  if (c->ngroups > 1) return GPC_E_UNSUPPORTED;
  if (gpc::pyr_level_cap(W, H) > 0x7FFFFFFFll) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// d_b null: d_a holds npairs + 1 frames (correspondences); else the left and right images of npairs pairs (supports).
// Every level is downsampled from the level before, matched by the plain call at its own size with its own settings into a
// workspace that holds every record, and the levels are merged into the caller's arrays.
template <bool CORR>
int pyr_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, int levels,
              const gpc_settings* s, void* d_out, int cap, int32_t* d_counts, int32_t* d_level_counts, int32_t* d_ncand) {
  int32_t ws[GPC_MAX_PYRAMID_LEVELS], hs[GPC_MAX_PYRAMID_LEVELS];
  CHK(pyr_usable(c, s, W, H, levels, ws, hs));
  if (npairs > 65535) return GPC_E_UNSUPPORTED;
  if (levels > 1) {  // (the downsampling step reads 8 bytes at a time)
    CHK(gpc::pyr_down_check(d_a, d_out, W, H, CORR ? npairs + 1 : npairs));
    if (!CORR) CHK(gpc::pyr_down_check(d_b, d_out, W, H, npairs));
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));
  StrictScope strict(c);
  const int nimg = CORR ? npairs + 1 : npairs;          // images per side
  const size_t ncs = CORR ? (size_t)nimg : 2 * (size_t)npairs;  // candidate counts per level
  auto match = [&](int l, const uint8_t* a, const uint8_t* b, void* rec, int rcap, int32_t* cnt) -> int {
    const gpc_settings sl = gpc::pyr_level_settings(*s, l);
    int32_t* nc = d_ncand ? d_ncand + (size_t)l * ncs : nullptr;
    LevelScope level(c, ws[l], hs[l]);
    if (CORR) return gpc_hip_match_sequence_device(c, a, ws[l], hs[l], nimg, &sl, (gpc_correspondence*)rec, rcap, cnt, nc);
    return gpc_hip_match_batch_device(c, a, b, ws[l], hs[l], npairs, &sl, (gpc_support*)rec, rcap, cnt, nc);
  };
  if (levels == 1) {  // the plain call, into the caller's arrays
    CHK(match(0, d_a, d_b, d_out, cap, d_counts));
    HIPCHK(c, hipMemcpyAsync(d_level_counts, d_counts, sizeof(int32_t) * (size_t)npairs, hipMemcpyDeviceToDevice, c->stream));
    return GPC_OK;
  }
  const size_t esz = sizeof(gpc::PyRec<CORR>);
  size_t img_at[GPC_MAX_PYRAMID_LEVELS] = {0}, rec_at[GPC_MAX_PYRAMID_LEVELS] = {0}, img_bytes = 0, rec_bytes = 0;
  int32_t caps[GPC_MAX_PYRAMID_LEVELS];
  for (int l = 0; l < levels; ++l) {
    caps[l] = (int32_t)gpc::pyr_level_cap(ws[l], hs[l]);
    rec_at[l] = rec_bytes;
    rec_bytes += pad16(esz * (size_t)caps[l] * npairs);
    if (!l) continue;
    img_at[l] = img_bytes;
    img_bytes += pad16((size_t)ws[l] * hs[l] * nimg) * (CORR ? 1 : 2);
  }
  CHK(ensure(c, c->py_img, img_bytes));
  CHK(ensure(c, c->py_rec, rec_bytes));
  CHK(ensure(c, c->py_cnt, sizeof(int32_t) * (size_t)levels * npairs));
  const void* d_rec[GPC_MAX_PYRAMID_LEVELS];
  const int32_t* d_cnt[GPC_MAX_PYRAMID_LEVELS];
  const uint8_t *a = d_a, *b = d_b;
  for (int l = 0; l < levels; ++l) {
    if (l) {
      uint8_t* na = (uint8_t*)c->py_img.p + img_at[l];
      uint8_t* nb = CORR ? nullptr : na + pad16((size_t)ws[l] * hs[l] * nimg);
      CHK(pyr_down(c, a, ws[l - 1], hs[l - 1], nimg, na));
      if (!CORR) CHK(pyr_down(c, b, ws[l - 1], hs[l - 1], nimg, nb));
      a = na;
      b = nb;
    }
    void* rec = (uint8_t*)c->py_rec.p + rec_at[l];
    int32_t* cnt = (int32_t*)c->py_cnt.p + (size_t)l * npairs;
    CHK(match(l, a, b, rec, caps[l], cnt));
    d_rec[l] = rec;
    d_cnt[l] = cnt;
  }
  return pyr_merge<CORR>(c, d_rec, caps, d_cnt, W, H, npairs, levels, d_out, cap, d_counts, d_level_counts);
}

// Host forms (Stage): chunks of at most 16 pairs, or of the pairs of GPC_HIP_SEQ_FRAMES frames (consecutive chunks share
// one).  b null: a holds npairs + 1 frames.  A chunk's counts, level counts and candidate counts land in h_cnt; its records
// go to the caller's array as far as the device form wrote them.
template <bool CORR>
int pyr_host(gpc_hip_ctx* c, const uint8_t* a, const uint8_t* b, int W, int H, int npairs, int levels, const gpc_settings* s,
             void* out, int cap, int32_t* counts, int32_t* level_counts, int32_t* ncand) {
  int32_t ws[GPC_MAX_PYRAMID_LEVELS], hs[GPC_MAX_PYRAMID_LEVELS];
  CHK(pyr_usable(c, s, W, H, levels, ws, hs));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H, esz = sizeof(gpc::PyRec<CORR>);
  const int seq = CORR ? 1 : 0;
  const int most = CORR ? (c->seq_frames > 1 && c->seq_frames < 16 ? c->seq_frames : 16) - 1 : 16;
  const int K = npairs < most ? npairs : most;
  const size_t ncs = CORR ? (size_t)K + 1 : 2 * (size_t)K;  // candidate counts of a full chunk, per level
  const size_t total_ncs = CORR ? (size_t)npairs + 1 : 2 * (size_t)npairs;
  Stage st(c);
  const size_t r_a = st.in(n * (K + seq)), r_b = st.in(CORR ? 0 : n * K), r_out = st.out(esz * (size_t)cap * K);
  const size_t r_cnt = st.out(sizeof(int32_t) * (size_t)K), r_lc = st.out(sizeof(int32_t) * (size_t)levels * K);
  const size_t r_nc = st.out(sizeof(int32_t) * levels * ncs);
  CHK(st.alloc(sizeof(int32_t) * ((size_t)K + (size_t)levels * K + levels * ncs)));
  int status = GPC_OK;
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    const size_t cs = CORR ? (size_t)pc + 1 : 2 * (size_t)pc;
    CHK(st.up(r_a, a + n * p0, n * (pc + seq)));
    if (!CORR) CHK(st.up(r_b, b + n * p0, n * pc));
    CHK(pyr_match<CORR>(c, st.p(r_a), CORR ? nullptr : st.p(r_b), W, H, pc, levels, s, st.p(r_out), cap, (int32_t*)st.p(r_cnt),
                        (int32_t*)st.p(r_lc), (int32_t*)st.p(r_nc)));
    int32_t *h_n = c->h_cnt.p, *h_lc = h_n + K, *h_nc = h_lc + (size_t)levels * K;
    CHK(st.down(h_n, r_cnt, sizeof(int32_t) * (size_t)pc));
    CHK(st.down(h_lc, r_lc, sizeof(int32_t) * (size_t)levels * pc));
    CHK(st.down(h_nc, r_nc, sizeof(int32_t) * levels * cs));
    CHK(st.wait());
    for (int t = 0; t < pc; ++t) {
      const size_t w = (size_t)valid_records(h_n[t], cap), q = (size_t)(p0 + t);
      if (h_n[t] > cap) status = GPC_E_CAPACITY;
      if (w) CHK(st.down((uint8_t*)out + esz * q * cap, r_out + esz * (size_t)t * cap, esz * w));
      counts[q] = h_n[t];
      for (int l = 0; l < levels; ++l) level_counts[(size_t)l * npairs + q] = h_lc[(size_t)l * pc + t];
    }
    if (ncand)
      for (int l = 0; l < levels; ++l)
        memcpy(ncand + l * total_ncs + (CORR ? (size_t)p0 : 2 * (size_t)p0), h_nc + l * cs, sizeof(int32_t) * cs);
    CHK(st.wait());
  }
  CHK(check_join_err(c));
  return status;
}

}  // namespace

extern "C" {

int gpc_hip_pyramid_levels(int W, int H, int levels, int32_t* widths, int32_t* heights) {
  return gpc::pyr_levels(W, H, levels, widths, heights);
}

int gpc_hip_pyramid_down_device(gpc_hip_ctx* c, const uint8_t* d_src, int W, int H, int nimages, uint8_t* d_dst) {
  if (!c) return GPC_E_INVALID;
  CHK(gpc::pyr_down_check(d_src, d_dst, W, H, nimages));
  HIPCHK(c, hipSetDevice(c->device));
  return pyr_down(c, d_src, W, H, nimages, d_dst);
}

int gpc_hip_pyramid_merge_supports_device(gpc_hip_ctx* c, const gpc_support* const* d_rec, const int32_t* caps,
                                          const int32_t* const* d_cnt, int W, int H, int npairs, int levels, gpc_support* d_out,
                                          int cap_per_pair, int32_t* d_counts, int32_t* d_level_counts) {
  return pyr_merge<false>(c, (const void* const*)d_rec, caps, d_cnt, W, H, npairs, levels, d_out, cap_per_pair, d_counts,
                          d_level_counts);
}

int gpc_hip_pyramid_merge_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* const* d_rec, const int32_t* caps,
                                                 const int32_t* const* d_cnt, int W, int H, int npairs, int levels,
                                                 gpc_correspondence* d_out, int cap_per_pair, int32_t* d_counts,
                                                 int32_t* d_level_counts) {
  return pyr_merge<true>(c, (const void* const*)d_rec, caps, d_cnt, W, H, npairs, levels, d_out, cap_per_pair, d_counts,
                         d_level_counts);
}

int gpc_hip_pyramid_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs, int levels,
                                 const gpc_settings* s, gpc_support* d_out, int cap_per_pair, int32_t* d_counts,
                                 int32_t* d_level_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_out || !d_counts || !d_level_counts || npairs <= 0 || cap_per_pair <= 0) return GPC_E_INVALID;
  return pyr_match<false>(c, d_rawL, d_rawR, W, H, npairs, levels, s, d_out, cap_per_pair, d_counts, d_level_counts, d_ncand);
}

int gpc_hip_pyramid_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, int levels,
                                    const gpc_settings* s, gpc_correspondence* d_out, int cap_per_pair, int32_t* d_counts,
                                    int32_t* d_level_counts, int32_t* d_ncand) {
  if (!c || !d_frames || !d_out || !d_counts || !d_level_counts || nframes < 2 || cap_per_pair <= 0) return GPC_E_INVALID;
  return pyr_match<true>(c, d_frames, nullptr, W, H, nframes - 1, levels, s, d_out, cap_per_pair, d_counts, d_level_counts,
                         d_ncand);
}

int gpc_hip_pyramid_batch(gpc_hip_ctx* c, const uint8_t* rawL, const uint8_t* rawR, int W, int H, int npairs, int levels,
                          const gpc_settings* s, gpc_support* out, int cap_per_pair, int32_t* counts, int32_t* level_counts,
                          int32_t* ncand) {
  if (!c || !rawL || !rawR || !out || !counts || !level_counts || npairs <= 0 || cap_per_pair <= 0) return GPC_E_INVALID;
  return pyr_host<false>(c, rawL, rawR, W, H, npairs, levels, s, out, cap_per_pair, counts, level_counts, ncand);
}

int gpc_hip_pyramid_sequence(gpc_hip_ctx* c, const uint8_t* frames, int W, int H, int nframes, int levels, const gpc_settings* s,
                             gpc_correspondence* out, int cap_per_pair, int32_t* counts, int32_t* level_counts, int32_t* ncand) {
  if (!c || !frames || !out || !counts || !level_counts || nframes < 2 || cap_per_pair <= 0) return GPC_E_INVALID;
  return pyr_host<true>(c, frames, nullptr, W, H, nframes - 1, levels, s, out, cap_per_pair, counts, level_counts, ncand);
}

}  // extern "C"
