// host_field_score.h -- dense fields scored against ground truth: the argument checks, the launch, the host form.
// A piece of gpc_hip.hip, included where the section stands: it needs what that file defines above the include
// and, before it, host_staging.h (Stage).  The kernel has no timing slot: the slot table is closed.
#pragma once

namespace {

static_assert(GPC_DENSE_NONE == FS_NONE && GPC_SCORE_MAX_THR == 8, "the kernel's view of none and of the thresholds");

int field_score_args(const gpc_hip_ctx* c, const void* field, int channels, int W, int H, int npairs, const gpc_truth* truth,
                     const gpc_field_score_prm* prm, const void* scores) {
  if (!c || !field || !scores) return GPC_E_INVALID;
  CHK(gpc::fs_params(prm));
  CHK(gpc::fs_limits(channels, W, H, npairs));
  return gpc::fs_truth(truth, channels);
}

// a clear of the scores, then one launch over fields, truth and class plane already on the device
int field_score_device(gpc_hip_ctx* c, const int32_t* d_field, int channels, int W, int H, int P, const gpc_truth* truth,
                       const gpc_field_score_prm* prm, const uint8_t* d_cls, gpc_field_score* d_scores, uint16_t* d_err) {
  HIPCHK(c, hipMemsetAsync(d_scores, 0, sizeof(gpc_field_score) * (size_t)P, c->stream));
  const gpc::FsPrm q = gpc::fs_squares(*prm);
  const long n = (long)W * H, chunks = (long)gpc::fs_chunks(W, H);
  const dim3 grid((unsigned)gpc::fs_groups(W, H, P));
  const bool bins = d_cls || prm->n_speed > 0;
#define GPC_FIELD_SCORE(C, B)                                                                                                \
  hipLaunchKernelGGL((gpc::k_field_score<C, B>), grid, dim3(FS_THREADS), 0, c->stream, d_field, truth->u, truth->v, truth->ignore, \
                     d_cls, n, chunks, chunks * P, q, (unsigned long long*)d_scores, d_err)
  if (channels == 1) {
    if (bins) GPC_FIELD_SCORE(1, true); else GPC_FIELD_SCORE(1, false);
  } else {
    if (bins) GPC_FIELD_SCORE(2, true); else GPC_FIELD_SCORE(2, false);
  }
#undef GPC_FIELD_SCORE
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

}  // namespace

extern "C" {

int gpc_hip_score_fields_device(gpc_hip_ctx* c, const int32_t* d_field, int channels, int W, int H, int npairs,
                                const gpc_truth* truth, const gpc_field_score_prm* prm, const uint8_t* d_cls,
                                gpc_field_score* d_scores, uint16_t* d_err) {
  CHK(field_score_args(c, d_field, channels, W, H, npairs, truth, prm, d_scores));
  HIPCHK(c, hipSetDevice(c->device));
  return field_score_device(c, d_field, channels, W, H, npairs, truth, prm, d_cls, d_scores, d_err);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields, truth and class plane up, their scores and errors down.
int gpc_hip_score_fields(gpc_hip_ctx* c, const int32_t* field, int channels, int W, int H, int npairs, const gpc_truth* truth,
                         const gpc_field_score_prm* prm, const uint8_t* cls, gpc_field_score* scores, uint16_t* err) {
  CHK(field_score_args(c, field, channels, W, H, npairs, truth, prm, scores));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n, tb = sizeof(float) * n;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_u = st.in(tb * K), r_v = st.in(truth->v ? tb * K : 0);
  const size_t r_ign = st.in(truth->ignore ? n * K : 0), r_cls = st.in(cls ? n * K : 0);
  const size_t r_sc = st.out(sizeof(gpc_field_score) * (size_t)K), r_err = st.out(err ? 2 * n * K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    CHK(st.up(r_u, truth->u + n * (size_t)p0, tb * pc));
    if (truth->v) CHK(st.up(r_v, truth->v + n * (size_t)p0, tb * pc));
    if (truth->ignore) CHK(st.up(r_ign, truth->ignore + n * (size_t)p0, n * pc));
    if (cls) CHK(st.up(r_cls, cls + n * (size_t)p0, n * pc));
    const gpc_truth dt = {(const float*)st.p(r_u), truth->v ? (const float*)st.p(r_v) : nullptr,
                          truth->ignore ? st.p(r_ign) : nullptr};
    CHK(field_score_device(c, (const int32_t*)st.p(r_field), channels, W, H, pc, &dt, prm, cls ? st.p(r_cls) : nullptr,
                           (gpc_field_score*)st.p(r_sc), err ? (uint16_t*)st.p(r_err) : nullptr));
    CHK(st.down(scores + p0, r_sc, sizeof(gpc_field_score) * (size_t)pc));
    if (err) CHK(st.down((uint8_t*)err + 2 * n * (size_t)p0, r_err, 2 * n * pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
