// host_clean.h -- cleaning dense fields: the check, the labelling, the median; reversed records; match-fill-and-clean; the
// host form.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h, host_refine.h (refine_records) and host_dense.h (dense_fill).
#pragma once

namespace {

static_assert(sizeof(gpc_clean) == 16 && GPC_DENSE_NONE == CL_NONE && CL_TILE == 32 && CL_CHECK_W * CL_CHECK_H == CL_THREADS,
              "the parameters and the kernels' view of none, of a tile and of a strip");

int clean_args(const gpc_hip_ctx* c, const void* fwd, const void* bwd, int channels, int W, int H, int npairs, const gpc_clean* prm,
               const void* out) {
  if (!c || !fwd || !out) return GPC_E_INVALID;
  CHK(gpc::cl_params(prm, bwd != nullptr));
  CHK(gpc::cl_limits(channels, W, H, npairs));
  const int64_t n = gpc::cl_field_bytes(channels, W, H, npairs);
  if (gpc::cl_overlap((uintptr_t)out, n, (uintptr_t)fwd, n) || gpc::cl_overlap((uintptr_t)out, n, (uintptr_t)bwd, n)) return GPC_E_INVALID;
  return GPC_OK;
}

// The launches over fields already on the device.  The label plane is d_label where the caller wants the labels, else the
// fill's owner plane: a fill that fed this call is queued before it, and the next one clears the plane itself.
template <int C>
int clean_run(gpc_hip_ctx* c, const int32_t* d_fwd, const int32_t* d_bwd, int W, int H, int P, const gpc_clean* prm, int32_t* d_out,
              uint8_t* d_state, int32_t* d_label, int32_t* d_stats) {
  const bool labels = gpc::cl_labels_needed(*prm, d_label != nullptr), sizes = prm->speckle_min > 1;
  int32_t* lab = d_label;
  if (!lab) {
    CHK(ensure(c, c->dn_owner, (size_t)gpc::cl_label_bytes(W, H, P)));
    lab = (int32_t*)c->dn_owner.p;
  }
  int32_t* size = nullptr;
  if (sizes) {
    CHK(ensure(c, c->cl_size, (size_t)gpc::cl_size_bytes(W, H, P)));
    size = (int32_t*)c->cl_size.p;
  }
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 4 * (size_t)P, c->stream));
  const dim3 tiles((unsigned)gpc::cl_tiles(W), (unsigned)gpc::cl_tiles(H), (unsigned)P);
  const dim3 strips((unsigned)((W + CL_CHECK_W - 1) / CL_CHECK_W), (unsigned)((H + CL_CHECK_H - 1) / CL_CHECK_H), (unsigned)P);
  for (int k = KID_CLEAN_CHECK; k <= KID_CLEAN_APPLY; ++k) c->launch_name[k][0] = 0;
  {
    Timed t(c, KID_CLEAN_CHECK);
    hipLaunchKernelGGL((gpc::k_clean_check<C>), strips, dim3(CL_THREADS), 0, c->stream, d_fwd, d_bwd, W, H, prm->check_tol_q8, lab,
                       size);
    snprintf(c->launch_name[KID_CLEAN_CHECK], sizeof c->launch_name[0], "gpc::k_clean_check<%d>", C);
  }
  if (labels) {
    {
      Timed t(c, KID_CLEAN_TILE);
      hipLaunchKernelGGL((gpc::k_clean_tile<C>), tiles, dim3(CL_THREADS), 0, c->stream, d_fwd, W, H, prm->speckle_diff_q8, lab);
      snprintf(c->launch_name[KID_CLEAN_TILE], sizeof c->launch_name[0], "gpc::k_clean_tile<%d>", C);
    }
    const long lanes = (long)gpc::cl_border_pixels(W, H);
    if (lanes > 0) {  // (one tile: its roots are the components' already)
      {
        Timed t(c, KID_CLEAN_BORDER);
        hipLaunchKernelGGL((gpc::k_clean_border<C>), dim3((unsigned)((lanes + CL_THREADS - 1) / CL_THREADS), 1, (unsigned)P),
                           dim3(CL_THREADS), 0, c->stream, d_fwd, W, H, prm->speckle_diff_q8, (gpc::cl_tiles(W) - 1) * H, (int)lanes,
                           lab);
        snprintf(c->launch_name[KID_CLEAN_BORDER], sizeof c->launch_name[0], "gpc::k_clean_border<%d>", C);
      }
      Timed t(c, KID_CLEAN_FLATTEN);
      hipLaunchKernelGGL(gpc::k_clean_flatten, strips, dim3(CL_THREADS), 0, c->stream, W, H, lab);
      snprintf(c->launch_name[KID_CLEAN_FLATTEN], sizeof c->launch_name[0], "gpc::k_clean_flatten");
    }
    if (sizes) {
      Timed t(c, KID_CLEAN_SIZES);
      hipLaunchKernelGGL(gpc::k_clean_sizes, tiles, dim3(CL_THREADS), 0, c->stream, (const int32_t*)lab, W, H, size);
      snprintf(c->launch_name[KID_CLEAN_SIZES], sizeof c->launch_name[0], "gpc::k_clean_sizes");
    }
  }
  {
    Timed t(c, KID_CLEAN_APPLY);
    const int smin = prm->speckle_min;
#define GPC_CLEAN_APPLY(R)                                                                                                   \
  hipLaunchKernelGGL((gpc::k_clean_apply<C, R>), tiles, dim3(CL_THREADS), 0, c->stream, d_fwd, (const int32_t*)lab,           \
                     (const int32_t*)size, W, H, smin, d_out, d_state, d_stats)
    if (prm->median_radius == 0) GPC_CLEAN_APPLY(0);
    else if (prm->median_radius == 1) GPC_CLEAN_APPLY(1);
    else GPC_CLEAN_APPLY(2);
#undef GPC_CLEAN_APPLY
    snprintf(c->launch_name[KID_CLEAN_APPLY], sizeof c->launch_name[0], "gpc::k_clean_apply<%d, %d>", C, prm->median_radius);
  }
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int clean_fields_device(gpc_hip_ctx* c, const int32_t* d_fwd, const int32_t* d_bwd, int channels, int W, int H, int P,
                        const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats) {
  return channels == 1 ? clean_run<1>(c, d_fwd, d_bwd, W, H, P, prm, d_out, d_state, d_label, d_stats)
                       : clean_run<2>(c, d_fwd, d_bwd, W, H, P, prm, d_out, d_state, d_label, d_stats);
}

int flip_args(const gpc_hip_ctx* c, const void* rec, const void* ref, int cap, const void* counts, int npairs, const void* rec_out,
              const void* ref_out) {
  if (!c || !rec || !counts || !rec_out || (ref != nullptr) != (ref_out != nullptr)) return GPC_E_INVALID;
  if (npairs < 1 || cap < 1) return GPC_E_INVALID;
  if (npairs > 65535 || (int64_t)npairs * cap > 0x7FFFFFFFll) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

template <bool CORR>
int flip_records(gpc_hip_ctx* c, const void* d_rec, const gpc_refinement* d_ref, int cap, const int32_t* d_counts, int P,
                 void* d_rec_out, gpc_refinement* d_ref_out) {
  typedef gpc::ConsRec<CORR> Rec;
  const long nb = ((long)cap + CL_THREADS - 1) / CL_THREADS;
  Timed t(c, KID_CLEAN_FLIP);
  hipLaunchKernelGGL((gpc::k_clean_flip<CORR>), dim3((unsigned)(nb < 4096 ? nb : 4096), P), dim3(CL_THREADS), 0, c->stream,
                     (const Rec*)d_rec, (const uint2*)d_ref, cap, d_counts, (Rec*)d_rec_out, (uint2*)d_ref_out);
  snprintf(c->launch_name[KID_CLEAN_FLIP], sizeof c->launch_name[0], "gpc::k_clean_flip<%s>", CORR ? "true" : "false");
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// match, refine (radius >= 1), fill; reverse the records where they lie and fill again (only for the check); clean
int clean_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s, int radius,
                const gpc_densify* fill, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats,
                int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand) {
  if (radius < 0 || radius > RF_MAX_RADIUS) return GPC_E_INVALID;
  CHK(gpc::dn_params(fill, radius >= 1));
  CHK(gpc::cl_params(prm, true));
  AllRecords r;
  CHK(all_records_cap(c, s, W, H, !d_b, &r.cap));
  CHK(gpc::dn_limits(W, H, npairs, r.cap));  // (before any workspace is made, too)
  const int C = d_b ? 1 : 2;
  const size_t field = (size_t)gpc::cl_field_bytes(C, W, H, npairs);
  if (gpc::cl_overlap((uintptr_t)d_out, (int64_t)field, (uintptr_t)d_fwd, (int64_t)field)) return GPC_E_INVALID;
  CHK(all_records(c, d_a, d_b, W, H, npairs, s, d_ncand, &r));
  if (d_counts) HIPCHK(c, hipMemcpyAsync(d_counts, r.counts, sizeof(int32_t) * (size_t)npairs, hipMemcpyDeviceToDevice, c->stream));
  gpc_refinement* d_ref = nullptr;
  if (radius >= 1) {
    CHK(ensure(c, c->dn_ref, sizeof(gpc_refinement) * (size_t)r.cap * npairs));
    d_ref = (gpc_refinement*)c->dn_ref.p;
    const uint8_t* d_next = d_b ? d_b : d_a + (size_t)W * H;
    CHK(d_b ? refine_records<false>(c, r.rec, r.cap, r.counts, d_a, d_next, W, H, npairs, radius, d_ref, nullptr)
            : refine_records<true>(c, r.rec, r.cap, r.counts, d_a, d_next, W, H, npairs, radius, d_ref, nullptr));
  }
  if (!d_fwd) {
    CHK(ensure(c, c->cl_fwd, field));
    d_fwd = (int32_t*)c->cl_fwd.p;
  }
  CHK(d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_fwd, d_level)
          : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_fwd, d_level));
  int32_t* d_bwd = nullptr;
  if (prm->check_tol_q8 >= 0) {
    CHK(ensure(c, c->cl_bwd, field));
    d_bwd = (int32_t*)c->cl_bwd.p;
    CHK(d_b ? flip_records<false>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref)
            : flip_records<true>(c, r.rec, d_ref, r.cap, r.counts, npairs, r.rec, d_ref));
    CHK(d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr)
            : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, fill, d_bwd, nullptr));
  }
  return clean_fields_device(c, d_fwd, d_bwd, C, W, H, npairs, prm, d_out, d_state, d_label, d_stats);
}

}  // namespace

extern "C" {

int gpc_hip_clean_fields_device(gpc_hip_ctx* c, const int32_t* d_fwd, const int32_t* d_bwd, int channels, int W, int H, int npairs,
                                const gpc_clean* prm, int32_t* d_out, uint8_t* d_state, int32_t* d_label, int32_t* d_stats) {
  CHK(clean_args(c, d_fwd, d_bwd, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return clean_fields_device(c, d_fwd, d_bwd, channels, W, H, npairs, prm, d_out, d_state, d_label, d_stats);
}

int gpc_hip_flip_supports_device(gpc_hip_ctx* c, const gpc_support* d_rec, const gpc_refinement* d_ref, int cap_per_pair,
                                 const int32_t* d_counts, int npairs, gpc_support* d_rec_out, gpc_refinement* d_ref_out) {
  CHK(flip_args(c, d_rec, d_ref, cap_per_pair, d_counts, npairs, d_rec_out, d_ref_out));
  HIPCHK(c, hipSetDevice(c->device));
  return flip_records<false>(c, d_rec, d_ref, cap_per_pair, d_counts, npairs, d_rec_out, d_ref_out);
}

int gpc_hip_flip_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* d_rec, const gpc_refinement* d_ref, int cap_per_pair,
                                        const int32_t* d_counts, int npairs, gpc_correspondence* d_rec_out,
                                        gpc_refinement* d_ref_out) {
  CHK(flip_args(c, d_rec, d_ref, cap_per_pair, d_counts, npairs, d_rec_out, d_ref_out));
  HIPCHK(c, hipSetDevice(c->device));
  return flip_records<true>(c, d_rec, d_ref, cap_per_pair, d_counts, npairs, d_rec_out, d_ref_out);
}

int gpc_hip_clean_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                               const gpc_settings* s, int refine_radius, const gpc_densify* fill, const gpc_clean* prm, int32_t* d_out,
                               uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level,
                               int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_out || npairs <= 0) return GPC_E_INVALID;
  return clean_match(c, d_rawL, d_rawR, W, H, npairs, s, refine_radius, fill, prm, d_out, d_state, d_label, d_stats, d_fwd, d_level,
                     d_counts, d_ncand);
}

int gpc_hip_clean_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                  int refine_radius, const gpc_densify* fill, const gpc_clean* prm, int32_t* d_out, uint8_t* d_state,
                                  int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts,
                                  int32_t* d_ncand) {
  if (!c || !d_frames || !d_out || nframes < 2) return GPC_E_INVALID;
  return clean_match(c, d_frames, nullptr, W, H, nframes - 1, s, refine_radius, fill, prm, d_out, d_state, d_label, d_stats, d_fwd,
                     d_level, d_counts, d_ncand);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields up, their outputs down.
int gpc_hip_clean_fields(gpc_hip_ctx* c, const int32_t* fwd, const int32_t* bwd, int channels, int W, int H, int npairs,
                         const gpc_clean* prm, int32_t* out, uint8_t* state, int32_t* label, int32_t* stats) {
  CHK(clean_args(c, fwd, bwd, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n;
  Stage st(c);
  const size_t r_fwd = st.in(fb * K), r_bwd = st.in(bwd ? fb * K : 0);
  const size_t r_out = st.out(fb * K), r_st = st.out(state ? n * K : 0), r_lab = st.out(label ? 4 * n * K : 0);
  const size_t r_sts = st.out(stats ? 16 * (size_t)K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_fwd, (const uint8_t*)fwd + fb * (size_t)p0, fb * pc));
    if (bwd) CHK(st.up(r_bwd, (const uint8_t*)bwd + fb * (size_t)p0, fb * pc));
    CHK(clean_fields_device(c, (const int32_t*)st.p(r_fwd), bwd ? (const int32_t*)st.p(r_bwd) : nullptr, channels, W, H, pc, prm,
                            (int32_t*)st.p(r_out), state ? st.p(r_st) : nullptr, label ? (int32_t*)st.p(r_lab) : nullptr,
                            stats ? (int32_t*)st.p(r_sts) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (state) CHK(st.down(state + n * (size_t)p0, r_st, n * pc));
    if (label) CHK(st.down(label + n * (size_t)p0, r_lab, 4 * n * pc));
    if (stats) CHK(st.down(stats + 4 * (size_t)p0, r_sts, 16 * (size_t)pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
