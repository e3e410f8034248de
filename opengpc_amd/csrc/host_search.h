// host_search.h -- the local dense search around every pixel of a field: the launch, match-fill-search-and-clean, the host form.
// A piece of gpc_hip.hip, included where the section stands: it needs what that file defines above the include
// and, before it, host_staging.h, host_refine.h (refine_records), host_dense.h (dense_fill) and host_clean.h (flip_records,
// clean_fields_device).
#pragma once

namespace {

static_assert(sizeof(gpc_search) == 16 && GPC_DENSE_NONE == SR_NONE && SR_THREADS == 256 && SR_MAX_RADIUS <= RF_MAX_RADIUS,
              "the parameters and the kernel's view of none and of a tile");

int search_args(const gpc_hip_ctx* c, const void* field, const void* imgL, const void* imgR, int channels, int W, int H, int npairs,
                const gpc_search* prm, const void* out) {
  if (!c || !field || !imgL || !imgR || !out) return GPC_E_INVALID;
  CHK(gpc::sr_params(prm));
  CHK(gpc::sr_limits(channels, W, H, npairs));
  if (!gpc::sr_alias_ok((uintptr_t)out, (uintptr_t)field, gpc::cl_field_bytes(channels, W, H, npairs), (uintptr_t)imgL, (uintptr_t)imgR,
                        (int64_t)W * H * npairs))
    return GPC_E_INVALID;
  return GPC_OK;
}

// One launch over a field and its two images already on the device, behind a clear of the stats.
template <int C, int R>
int search_run(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
               const gpc_search* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 4 * (size_t)P, c->stream));
  const dim3 tiles((unsigned)gpc::sr_tiles_x(W), (unsigned)gpc::sr_tiles_y(H), (unsigned)P);
  {
    Timed t(c, KID_SEARCH);
#define GPC_SEARCH(G)                                                                                                              \
  hipLaunchKernelGGL((gpc::k_search<C, R, G>), tiles, dim3(SR_THREADS), 0, c->stream, d_field, d_imgL, d_imgR, W, H, prm->subpixel, \
                     prm->max_cost, d_out, d_cost, d_choice, d_stats)
    if (prm->range == 0) GPC_SEARCH(0);
    else if (prm->range == 1) GPC_SEARCH(1);
    else GPC_SEARCH(2);
#undef GPC_SEARCH
    snprintf(c->launch_name[KID_SEARCH], sizeof c->launch_name[0], "gpc::k_search<%d, %d, %d>", C, R, prm->range);
  }
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

template <int C>
int search_radius(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                  const gpc_search* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  switch (prm->radius) {
    case 1: return search_run<C, 1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    case 2: return search_run<C, 2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    case 3: return search_run<C, 3>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    default: return search_run<C, 4>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
  }
}

int search_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels, int W,
                         int H, int P, const gpc_search* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  return channels == 1 ? search_radius<1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats)
                       : search_radius<2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
}

// clean_match with the search behind each fill: match, refine (radius >= 1), fill, search in place; reverse the records
// where they lie, fill again and search with the two images exchanged (only for the check); clean
int search_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s, int radius,
                 const gpc_densify* fill, const gpc_search* search, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                 int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand,
                 uint16_t* d_cost) {
  if (radius < 0 || radius > RF_MAX_RADIUS) return GPC_E_INVALID;
  CHK(gpc::dn_params(fill, radius >= 1));
  CHK(gpc::sr_params(search));
  CHK(gpc::cl_params(prm, true));
  AllRecords r;
  CHK(all_records_cap(c, s, W, H, !d_b, &r.cap));
  CHK(gpc::dn_limits(W, H, npairs, r.cap));  // (before any workspace is made, too)
  const int C = d_b ? 1 : 2;
  const size_t field = (size_t)gpc::cl_field_bytes(C, W, H, npairs);
  if (gpc::cl_overlap((uintptr_t)d_out, (int64_t)field, (uintptr_t)d_fwd, (int64_t)field)) return GPC_E_INVALID;
  CHK(all_records(c, d_a, d_b, W, H, npairs, s, d_ncand, &r));
  if (d_counts) HIPCHK(c, hipMemcpyAsync(d_counts, r.counts, sizeof(int32_t) * (size_t)npairs, hipMemcpyDeviceToDevice, c->stream));
  const uint8_t* d_next = d_b ? d_b : d_a + (size_t)W * H;
  gpc_refinement* d_ref = nullptr;
  if (radius >= 1) {
    CHK(ensure(c, c->dn_ref, sizeof(gpc_refinement) * (size_t)r.cap * npairs));
    d_ref = (gpc_refinement*)c->dn_ref.p;
    CHK(d_b ? refine_records<false>(c, r.rec, r.cap, r.counts, d_a, d_next, W, H, npairs, radius, d_ref, nullptr)
            : refine_records<true>(c, r.rec, r.cap, r.counts, d_a, d_next, W, H, npairs, radius, d_ref, nullptr));
  }
  if (!d_fwd) {
    CHK(ensure(c, c->cl_fwd, field));
    d_fwd = (int32_t*)c->cl_fwd.p;
  }
  CHK(d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_fwd, d_level)
          : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_fwd, d_level));
  CHK(search_fields_device(c, d_fwd, d_a, d_next, C, W, H, npairs, search, d_fwd, d_cost, nullptr, nullptr));
  int32_t* d_bwd = nullptr;
  if (prm->check_tol_q8 >= 0) {
    CHK(ensure(c, c->cl_bwd, field));
    d_bwd = (int32_t*)c->cl_bwd.p;
    CHK(d_b ? flip_records<false>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref)
            : flip_records<true>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref));
    CHK(d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr)
            : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr));
    CHK(search_fields_device(c, d_bwd, d_next, d_a, C, W, H, npairs, search, d_bwd, nullptr, nullptr, nullptr));
  }
  return clean_fields_device(c, d_fwd, d_bwd, C, W, H, npairs, prm, d_out, d_state, d_label, d_stats);
}

}  // namespace

extern "C" {

int gpc_hip_search_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels,
                                 int W, int H, int npairs, const gpc_search* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice,
                                 int32_t* d_stats) {
  CHK(search_args(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return search_fields_device(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out, d_cost, d_choice, d_stats);
}

int gpc_hip_search_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                const gpc_settings* s, int refine_radius, const gpc_densify* fill, const gpc_search* search,
                                const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats,
                                int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost) {
  if (!c || !d_rawL || !d_rawR || !d_out || npairs <= 0) return GPC_E_INVALID;
  return search_match(c, d_rawL, d_rawR, W, H, npairs, s, refine_radius, fill, search, prm, d_out, d_state, d_label, d_stats, d_fwd,
                      d_level, d_counts, d_ncand, d_cost);
}

int gpc_hip_search_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                   int refine_radius, const gpc_densify* fill, const gpc_search* search, const gpc_clean* prm,
                                   int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                                   uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost) {
  if (!c || !d_frames || !d_out || nframes < 2) return GPC_E_INVALID;
  return search_match(c, d_frames, nullptr, W, H, nframes - 1, s, refine_radius, fill, search, prm, d_out, d_state, d_label, d_stats,
                      d_fwd, d_level, d_counts, d_ncand, d_cost);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields and images up, their outputs down.
int gpc_hip_search_fields(gpc_hip_ctx* c, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels, int W, int H,
                          int npairs, const gpc_search* prm, int32_t* out, uint16_t* cost, uint8_t* choice, int32_t* stats) {
  CHK(search_args(c, field, imgL, imgR, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_l = st.in(n * K), r_r = st.in(n * K);
  const size_t r_out = st.out(fb * K), r_cost = st.out(cost ? 2 * n * K : 0), r_ch = st.out(choice ? n * K : 0);
  const size_t r_sts = st.out(stats ? 16 * (size_t)K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    CHK(st.up(r_l, imgL + n * (size_t)p0, n * pc));
    CHK(st.up(r_r, imgR + n * (size_t)p0, n * pc));
    CHK(search_fields_device(c, (const int32_t*)st.p(r_field), st.p(r_l), st.p(r_r), channels, W, H, pc, prm, (int32_t*)st.p(r_out),
                             cost ? (uint16_t*)st.p(r_cost) : nullptr, choice ? st.p(r_ch) : nullptr,
                             stats ? (int32_t*)st.p(r_sts) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (cost) CHK(st.down((uint8_t*)cost + 2 * n * (size_t)p0, r_cost, 2 * n * pc));
    if (choice) CHK(st.down(choice + n * (size_t)p0, r_ch, n * pc));
    if (stats) CHK(st.down(stats + 4 * (size_t)p0, r_sts, 16 * (size_t)pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
