// host_inpaint.h -- completing cleaned fields, guided by the image: the launches, match-fill-clean-and-complete, the host form.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h and host_clean.h (clean_match).
#pragma once

namespace {

static_assert(sizeof(gpc_inpaint) == 16 && GPC_DENSE_NONE == IP_NONE && IP_TILE == CL_TILE && IP_MAX_PASSES < 255,
              "the parameters and the kernels' view of none, of a tile and of a pass byte");

int inpaint_args(const gpc_hip_ctx* c, const void* field, const void* guide, int channels, int W, int H, int npairs,
                 const gpc_inpaint* prm, const void* out) {
  if (!c || !field || !guide || !out) return GPC_E_INVALID;
  CHK(gpc::ip_params(prm));
  CHK(gpc::ip_limits(channels, W, H, npairs));
  if (!gpc::ip_alias_ok((uintptr_t)out, (uintptr_t)field, gpc::cl_field_bytes(channels, W, H, npairs))) return GPC_E_INVALID;
  return GPC_OK;
}

// The launches over a field and a guide already on the device: begin, then one launch per pass, in place in d_out.  The pass
// plane is d_pass where the caller wants it, else a workspace; the stats likewise.  Nothing is read on the host: a pass
// that has nothing left to do finds that out on the device.
template <int C>
int inpaint_run(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int W, int H, int P, const gpc_inpaint* prm,
                int32_t* d_out, uint8_t* d_pass, int32_t* d_stats) {
  uint8_t* pz = d_pass;
  if (!pz) {
    CHK(ensure(c, c->ip_pass, (size_t)gpc::ip_pass_bytes(W, H, P)));
    pz = (uint8_t*)c->ip_pass.p;
  }
  CHK(ensure(c, c->ip_ctl, (size_t)gpc::ip_ctl_bytes(W, H, P)));
  int32_t* ctl = (int32_t*)c->ip_ctl.p;
  int32_t* stats = d_stats ? d_stats : ctl + gpc::ip_ctl_stats_at();
  int32_t* tile_holes = ctl + gpc::ip_ctl_tiles_at(P);
  HIPCHK(c, hipMemsetAsync(ctl, 0, sizeof(int32_t) * (size_t)(d_stats ? gpc::ip_ctl_stats_at() : gpc::ip_ctl_tiles_at(P)), c->stream));
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 2 * (size_t)P, c->stream));
  const dim3 tiles((unsigned)gpc::ip_tiles(W), (unsigned)gpc::ip_tiles(H), (unsigned)P);
  {
    Timed t(c, KID_INPAINT_BEGIN);
    hipLaunchKernelGGL((gpc::k_inpaint_begin<C>), tiles, dim3(IP_THREADS), 0, c->stream, d_field, W, H, d_out, pz, tile_holes, stats);
    snprintf(c->launch_name[KID_INPAINT_BEGIN], sizeof c->launch_name[0], "gpc::k_inpaint_begin<%d>", C);
  }
  for (int k = 1; k <= prm->passes; ++k) {
    Timed t(c, KID_INPAINT_PASS);
    hipLaunchKernelGGL((gpc::k_inpaint_pass<C>), tiles, dim3(IP_THREADS), 0, c->stream, d_out, pz, d_guide, W, H, prm->radius,
                       prm->range_shift, prm->min_weight, k, tile_holes, ctl, stats);
  }
  snprintf(c->launch_name[KID_INPAINT_PASS], sizeof c->launch_name[0], "gpc::k_inpaint_pass<%d>", C);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int inpaint_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int channels, int W, int H, int P,
                          const gpc_inpaint* prm, int32_t* d_out, uint8_t* d_pass, int32_t* d_stats) {
  return channels == 1 ? inpaint_run<1>(c, d_field, d_guide, W, H, P, prm, d_out, d_pass, d_stats)
                       : inpaint_run<2>(c, d_field, d_guide, W, H, P, prm, d_out, d_pass, d_stats);
}

// clean_match into d_cleaned (or straight into d_out, which is then completed in place), then the completion guided by d_a:
// the left images of a batch, or frames 0 .. nframes - 2 of a sequence
int inpaint_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s, int radius,
                  const gpc_densify* fill, const gpc_clean* prm, const gpc_inpaint* ip, int32_t* d_out, uint8_t* d_pass,
                  int32_t* d_fill_stats, int32_t* d_cleaned, uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd,
                  uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand) {
  CHK(gpc::ip_params(ip));
  const int C = d_b ? 1 : 2;
  const int64_t field = W > 0 && H > 0 ? gpc::cl_field_bytes(C, W, H, npairs) : 0;
  if (d_cleaned) {
    if (!gpc::ip_alias_ok((uintptr_t)d_out, (uintptr_t)d_cleaned, field)) return GPC_E_INVALID;
    if (gpc::cl_overlap((uintptr_t)d_out, field, (uintptr_t)d_fwd, field)) return GPC_E_INVALID;
  }
  int32_t* mid = d_cleaned ? d_cleaned : d_out;
  CHK(clean_match(c, d_a, d_b, W, H, npairs, s, radius, fill, prm, mid, d_state, d_label, d_stats, d_fwd, d_level, d_counts, d_ncand));
  return inpaint_fields_device(c, mid, d_a, C, W, H, npairs, ip, d_out, d_pass, d_fill_stats);
}

}  // namespace

extern "C" {

int gpc_hip_inpaint_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int channels, int W, int H,
                                  int npairs, const gpc_inpaint* prm, int32_t* d_out, uint8_t* d_pass, int32_t* d_stats) {
  CHK(inpaint_args(c, d_field, d_guide, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return inpaint_fields_device(c, d_field, d_guide, channels, W, H, npairs, prm, d_out, d_pass, d_stats);
}

int gpc_hip_inpaint_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                 const gpc_settings* s, int refine_radius, const gpc_densify* fill, const gpc_clean* prm,
                                 const gpc_inpaint* ip, int32_t* d_out, uint8_t* d_pass, int32_t* d_fill_stats, int32_t* d_cleaned,
                                 uint8_t* d_state, int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level,
                                 int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_out || npairs <= 0) return GPC_E_INVALID;
  return inpaint_match(c, d_rawL, d_rawR, W, H, npairs, s, refine_radius, fill, prm, ip, d_out, d_pass, d_fill_stats, d_cleaned,
                       d_state, d_label, d_stats, d_fwd, d_level, d_counts, d_ncand);
}

int gpc_hip_inpaint_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                    int refine_radius, const gpc_densify* fill, const gpc_clean* prm, const gpc_inpaint* ip,
                                    int32_t* d_out, uint8_t* d_pass, int32_t* d_fill_stats, int32_t* d_cleaned, uint8_t* d_state,
                                    int32_t* d_label, int32_t* d_stats, int32_t* d_fwd, uint8_t* d_level, int32_t* d_counts,
                                    int32_t* d_ncand) {
  if (!c || !d_frames || !d_out || nframes < 2) return GPC_E_INVALID;
  return inpaint_match(c, d_frames, nullptr, W, H, nframes - 1, s, refine_radius, fill, prm, ip, d_out, d_pass, d_fill_stats,
                       d_cleaned, d_state, d_label, d_stats, d_fwd, d_level, d_counts, d_ncand);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields and guides up, their outputs down.
int gpc_hip_inpaint_fields(gpc_hip_ctx* c, const int32_t* field, const uint8_t* guide, int channels, int W, int H, int npairs,
                           const gpc_inpaint* prm, int32_t* out, uint8_t* pass, int32_t* stats) {
  CHK(inpaint_args(c, field, guide, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_guide = st.in(n * K);
  const size_t r_out = st.out(fb * K), r_pass = st.out(pass ? n * K : 0), r_sts = st.out(stats ? 8 * (size_t)K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    CHK(st.up(r_guide, guide + n * (size_t)p0, n * pc));
    CHK(inpaint_fields_device(c, (const int32_t*)st.p(r_field), st.p(r_guide), channels, W, H, pc, prm, (int32_t*)st.p(r_out),
                              pass ? st.p(r_pass) : nullptr, stats ? (int32_t*)st.p(r_sts) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (pass) CHK(st.down(pass + n * (size_t)p0, r_pass, n * pc));
    if (stats) CHK(st.down(stats + 2 * (size_t)p0, r_sts, 8 * (size_t)pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
