// host_gapfill.h -- closing holes along scanlines from the background side: the three launches, the host form.
// A piece of gpc_hip.hip, included where the section stands: it needs what that file defines above the include
// and, before it, host_staging.h (Stage).
#pragma once

namespace {

static_assert(sizeof(gpc_gapfill) == 16 && GPC_DENSE_NONE == gpc::GF_NONE && GF_MAX_GAP < (int)GF_FAR && 32768 < (int)GF_FAR,
              "the parameters, the kernels' view of none, and a real distance below the codes");

int gapfill_args(const gpc_hip_ctx* c, const void* field, const void* guide, int channels, int W, int H, int npairs,
                 const gpc_gapfill* prm, const void* out) {
  if (!c || !field || !out) return GPC_E_INVALID;
  CHK(gpc::gf_params(prm, guide != nullptr));
  CHK(gpc::gf_limits(channels, W, H, npairs));
  if (!gpc::gf_alias_ok((uintptr_t)out, (uintptr_t)field, gpc::cl_field_bytes(channels, W, H, npairs), (uintptr_t)guide,
                        (int64_t)W * H * npairs))
    return GPC_E_INVALID;
  return GPC_OK;
}

// A clear of the stats, the row scan, the column scan, the choice.  No launch is timed: the slot table is closed.
template <int C, int SEL>
int gapfill_run(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int W, int H, int P, const gpc_gapfill* prm,
                int32_t* d_out, uint8_t* d_how, int32_t* d_stats) {
  CHK(ensure(c, c->gf_ws, (size_t)gpc::gf_ws_bytes(W, H, P)));
  const size_t plane = (size_t)gpc::gf_plane_pixels(W, H, P), n = (size_t)W * H;
  uint16_t* dist = (uint16_t*)c->gf_ws.p;
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 4 * (size_t)P, c->stream));
  const int band = gpc::gf_band(prm->max_gap);
  hipLaunchKernelGGL(gpc::k_gapfill_rows, dim3((unsigned)((H + GF_THREADS / 64 - 1) / (GF_THREADS / 64)), (unsigned)P), dim3(GF_THREADS), 0,
                     c->stream, d_field, (size_t)C * n, W, H, dist, dist + plane);
  hipLaunchKernelGGL(gpc::k_gapfill_cols, dim3((unsigned)((W + GF_THREADS - 1) / GF_THREADS), (unsigned)gpc::gf_bands(H, prm->max_gap), (unsigned)P),
                     dim3(GF_THREADS), 0, c->stream, d_field, (size_t)C * n, W, H, band, prm->max_gap, dist + 2 * plane, dist + 3 * plane);
  hipLaunchKernelGGL((gpc::k_gapfill_choose<C, SEL>), dim3((unsigned)((n + GF_THREADS - 1) / GF_THREADS), (unsigned)P), dim3(GF_THREADS), 0,
                     c->stream, d_field, d_guide, (const uint16_t*)dist, plane, W, H, prm->max_gap, prm->discon_q8, prm->border,
                     d_out != d_field ? 1 : 0, d_out, d_how, d_stats);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int gapfill_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int channels, int W, int H, int P,
                          const gpc_gapfill* prm, int32_t* d_out, uint8_t* d_how, int32_t* d_stats) {
  if (prm->select == 0)
    return channels == 1 ? gapfill_run<1, 0>(c, d_field, d_guide, W, H, P, prm, d_out, d_how, d_stats)
                         : gapfill_run<2, 0>(c, d_field, d_guide, W, H, P, prm, d_out, d_how, d_stats);
  return channels == 1 ? gapfill_run<1, 1>(c, d_field, d_guide, W, H, P, prm, d_out, d_how, d_stats)
                       : gapfill_run<2, 1>(c, d_field, d_guide, W, H, P, prm, d_out, d_how, d_stats);
}

}  // namespace

extern "C" {

int gpc_hip_gapfill_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_guide, int channels, int W, int H,
                                  int npairs, const gpc_gapfill* prm, int32_t* d_out, uint8_t* d_how, int32_t* d_stats) {
  CHK(gapfill_args(c, d_field, d_guide, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return gapfill_fields_device(c, d_field, d_guide, channels, W, H, npairs, prm, d_out, d_how, d_stats);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields and (where there are any) guides up, their outputs down.
int gpc_hip_gapfill_fields(gpc_hip_ctx* c, const int32_t* field, const uint8_t* guide, int channels, int W, int H, int npairs,
                           const gpc_gapfill* prm, int32_t* out, uint8_t* how, int32_t* stats) {
  CHK(gapfill_args(c, field, guide, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_guide = st.in(guide ? n * K : 0);
  const size_t r_out = st.out(fb * K), r_how = st.out(how ? n * K : 0), r_sts = st.out(stats ? 16 * (size_t)K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    if (guide) CHK(st.up(r_guide, guide + n * (size_t)p0, n * pc));
    CHK(gapfill_fields_device(c, (const int32_t*)st.p(r_field), guide ? st.p(r_guide) : nullptr, channels, W, H, pc, prm,
                              (int32_t*)st.p(r_out), how ? st.p(r_how) : nullptr, stats ? (int32_t*)st.p(r_sts) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (how) CHK(st.down(how + n * (size_t)p0, r_how, n * pc));
    if (stats) CHK(st.down((uint8_t*)stats + 16 * (size_t)p0, r_sts, 16 * (size_t)pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
