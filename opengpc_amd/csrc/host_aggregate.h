// host_aggregate.h -- the scanline aggregation of the search's costs: the launches, match-fill-aggregate-and-clean, the host form.
// A piece of gpc_hip.hip, included where the section stands: it needs what that file defines above the include
// and, before it, host_staging.h, host_refine.h (refine_records), host_dense.h (dense_fill), host_clean.h (flip_records,
// clean_fields_device) and host_search.h (search_args).
#pragma once

namespace {

static_assert(sizeof(gpc_aggregate) == 28 && AG_LANES == 64 && AG_MAX_COST + AG_MAX_PENALTY < (int)AG_NONE,
              "the parameters, a wave of chains, and a path value in 16 bits beside the mark");

int aggregate_args(const gpc_hip_ctx* c, const void* field, const void* imgL, const void* imgR, int channels, int W, int H, int npairs,
                   const gpc_aggregate* prm, const void* out) {
  CHK(gpc::ag_params(prm));
  const gpc_search s = {prm->radius, prm->range, prm->subpixel, prm->max_cost};
  return search_args(c, field, imgL, imgR, channels, W, H, npairs, &s, out);
}

// The launches of one group of pairs; every pointer is the group's.  None of them is timed: the slot table is closed.
template <int C, int R, int G>
int aggregate_group(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                    const gpc_aggregate* prm, uint16_t* d_vol, uint16_t* d_path, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice,
                    int32_t* d_stats, uint32_t* d_agg) {
  const dim3 tiles((unsigned)gpc::sr_tiles_x(W), (unsigned)gpc::sr_tiles_y(H), (unsigned)P);
  hipLaunchKernelGGL((gpc::k_agg_cost<C, R, G>), tiles, dim3(SR_THREADS), 0, c->stream, d_field, d_imgL, d_imgR, W, H, d_vol);
  const int h = (prm->paths & 1) + (prm->paths >> 1 & 1), v = (prm->paths >> 2 & 1) + (prm->paths >> 3 & 1);
  if (h)
    hipLaunchKernelGGL((gpc::k_agg_path_h<C, G>), dim3((unsigned)gpc::ag_blocks(H), (unsigned)h, (unsigned)P), dim3(AG_LANES), 0,
                       c->stream, d_field, (const uint16_t*)d_vol, W, H, prm->paths, (uint32_t)prm->p1, (uint32_t)prm->p2, d_path);
  if (v)
    hipLaunchKernelGGL((gpc::k_agg_path_v<C, G>), dim3((unsigned)gpc::ag_blocks(W), (unsigned)v, (unsigned)P), dim3(AG_LANES), 0,
                       c->stream, d_field, (const uint16_t*)d_vol, W, H, prm->paths, (uint32_t)prm->p1, (uint32_t)prm->p2, d_path);
  const unsigned blocks = (unsigned)(((size_t)W * H + AG_CHOOSE_THREADS - 1) / AG_CHOOSE_THREADS);
  hipLaunchKernelGGL((gpc::k_agg_choose<C, G>), dim3(blocks, 1, (unsigned)P), dim3(AG_CHOOSE_THREADS), 0, c->stream, d_field,
                     (const uint16_t*)d_vol, (const uint16_t*)d_path, W, H, prm->paths, prm->subpixel, prm->max_cost, d_out, d_cost,
                     d_choice, d_stats, d_agg);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// A clear of the stats, then the pairs in groups of what the budget holds (ag_group); the workspace is one block: the cost
// volume of a group, then its path volumes
template <int C, int R, int G>
int aggregate_run(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                  const gpc_aggregate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats, uint32_t* d_agg) {
  const size_t n = (size_t)W * H;
  const int g = gpc::ag_group(C, W, H, P, G, prm->paths, c->agg_group_bytes);
  const size_t vol = 2 * (size_t)gpc::ag_cells(C, G) * n * g;
  CHK(ensure(c, c->ag_ws, (size_t)gpc::ag_pixel_bytes(C, G, prm->paths) * n * g));
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 4 * (size_t)P, c->stream));
  uint16_t* d_vol = (uint16_t*)c->ag_ws.p;
  uint16_t* d_path = (uint16_t*)((uint8_t*)c->ag_ws.p + vol);
  for (int p0 = 0; p0 < P; p0 += g) {
    const int pc = P - p0 < g ? P - p0 : g;
    CHK((aggregate_group<C, R, G>(c, d_field + (size_t)p0 * C * n, d_imgL + (size_t)p0 * n, d_imgR + (size_t)p0 * n, W, H, pc, prm, d_vol,
                                  d_path, d_out + (size_t)p0 * C * n, d_cost ? d_cost + (size_t)p0 * n : nullptr,
                                  d_choice ? d_choice + (size_t)p0 * n : nullptr, d_stats ? d_stats + (size_t)p0 * 4 : nullptr,
                                  d_agg ? d_agg + (size_t)p0 * n : nullptr)));
  }
  return GPC_OK;
}

template <int C, int R>
int aggregate_range(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                    const gpc_aggregate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats, uint32_t* d_agg) {
  switch (prm->range) {
    case 0: return aggregate_run<C, R, 0>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
    case 1: return aggregate_run<C, R, 1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
    default: return aggregate_run<C, R, 2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
  }
}

template <int C>
int aggregate_radius(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                     const gpc_aggregate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats, uint32_t* d_agg) {
  switch (prm->radius) {
    case 1: return aggregate_range<C, 1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
    case 2: return aggregate_range<C, 2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
    case 3: return aggregate_range<C, 3>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
    default: return aggregate_range<C, 4>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
  }
}

int aggregate_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels, int W,
                            int H, int P, const gpc_aggregate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice,
                            int32_t* d_stats, uint32_t* d_agg) {
  return channels == 1 ? aggregate_radius<1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg)
                       : aggregate_radius<2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats, d_agg);
}

// search_match with the aggregation in the search's place
int aggregate_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s, int radius,
                    const gpc_densify* fill, const gpc_aggregate* agg, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                    int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand,
                    uint16_t* d_cost) {
  if (radius < 0 || radius > RF_MAX_RADIUS) return GPC_E_INVALID;
  CHK(gpc::dn_params(fill, radius >= 1));
  CHK(gpc::ag_params(agg));
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
  CHK(aggregate_fields_device(c, d_fwd, d_a, d_next, C, W, H, npairs, agg, d_fwd, d_cost, nullptr, nullptr, nullptr));
  int32_t* d_bwd = nullptr;
  if (prm->check_tol_q8 >= 0) {
    CHK(ensure(c, c->cl_bwd, field));
    d_bwd = (int32_t*)c->cl_bwd.p;
    CHK(d_b ? flip_records<false>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref)
            : flip_records<true>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref));
    CHK(d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr)
            : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr));
    CHK(aggregate_fields_device(c, d_bwd, d_next, d_a, C, W, H, npairs, agg, d_bwd, nullptr, nullptr, nullptr, nullptr));
  }
  return clean_fields_device(c, d_fwd, d_bwd, C, W, H, npairs, prm, d_out, d_state, d_label, d_stats);
}

}  // namespace

extern "C" {

int gpc_hip_aggregate_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels,
                                    int W, int H, int npairs, const gpc_aggregate* prm, int32_t* d_out, uint16_t* d_cost,
                                    uint8_t* d_choice, int32_t* d_stats, uint32_t* d_agg) {
  CHK(aggregate_args(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return aggregate_fields_device(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out, d_cost, d_choice, d_stats, d_agg);
}

int gpc_hip_aggregate_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                   const gpc_settings* s, int refine_radius, const gpc_densify* fill, const gpc_aggregate* aggregate,
                                   const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats,
                                   int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost) {
  if (!c || !d_rawL || !d_rawR || !d_out || npairs <= 0) return GPC_E_INVALID;
  return aggregate_match(c, d_rawL, d_rawR, W, H, npairs, s, refine_radius, fill, aggregate, prm, d_out, d_state, d_label, d_stats,
                         d_fwd, d_level, d_counts, d_ncand, d_cost);
}

int gpc_hip_aggregate_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                      int refine_radius, const gpc_densify* fill, const gpc_aggregate* aggregate, const gpc_clean* prm,
                                      int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                                      uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand, uint16_t* d_cost) {
  if (!c || !d_frames || !d_out || nframes < 2) return GPC_E_INVALID;
  return aggregate_match(c, d_frames, nullptr, W, H, nframes - 1, s, refine_radius, fill, aggregate, prm, d_out, d_state, d_label,
                         d_stats, d_fwd, d_level, d_counts, d_ncand, d_cost);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields and images up, their outputs down.
int gpc_hip_aggregate_fields(gpc_hip_ctx* c, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels, int W, int H,
                             int npairs, const gpc_aggregate* prm, int32_t* out, uint16_t* cost, uint8_t* choice, int32_t* stats,
                             uint32_t* agg) {
  CHK(aggregate_args(c, field, imgL, imgR, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_l = st.in(n * K), r_r = st.in(n * K);
  const size_t r_out = st.out(fb * K), r_cost = st.out(cost ? 2 * n * K : 0), r_ch = st.out(choice ? n * K : 0);
  const size_t r_sts = st.out(stats ? 16 * (size_t)K : 0), r_agg = st.out(agg ? 4 * n * K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    CHK(st.up(r_l, imgL + n * (size_t)p0, n * pc));
    CHK(st.up(r_r, imgR + n * (size_t)p0, n * pc));
    CHK(aggregate_fields_device(c, (const int32_t*)st.p(r_field), st.p(r_l), st.p(r_r), channels, W, H, pc, prm, (int32_t*)st.p(r_out),
                                cost ? (uint16_t*)st.p(r_cost) : nullptr, choice ? st.p(r_ch) : nullptr,
                                stats ? (int32_t*)st.p(r_sts) : nullptr, agg ? (uint32_t*)st.p(r_agg) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (cost) CHK(st.down((uint8_t*)cost + 2 * n * (size_t)p0, r_cost, 2 * n * pc));
    if (choice) CHK(st.down(choice + n * (size_t)p0, r_ch, n * pc));
    if (stats) CHK(st.down(stats + 4 * (size_t)p0, r_sts, 16 * (size_t)pc));
    if (agg) CHK(st.down((uint8_t*)agg + 4 * n * (size_t)p0, r_agg, 4 * n * pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
