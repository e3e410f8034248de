// host_propagate.h -- the propagation of field values between neighbours: the launches of the iterations, the host form.
// A piece of gpc_hip.hip, included where the section stands: it needs what that file defines above the include
// and, before it, host_staging.h (Stage).
#pragma once

namespace {

static_assert(sizeof(gpc_propagate) == 16 && PG_MAX_ITERATIONS * 4 * sizeof(int32_t) == 256, "the parameters, and a pair's rows of stats");

int propagate_args(const gpc_hip_ctx* c, const void* field, const void* imgL, const void* imgR, int channels, int W, int H, int npairs,
                   const gpc_propagate* prm, const void* out) {
  if (!c || !field || !imgL || !imgR || !out) return GPC_E_INVALID;
  CHK(gpc::pg_params(prm));
  CHK(gpc::pg_limits(channels, W, H, npairs));
  if (!gpc::pg_alias_ok((uintptr_t)out, (uintptr_t)field, gpc::cl_field_bytes(channels, W, H, npairs), (uintptr_t)imgL, (uintptr_t)imgR,
                        (int64_t)W * H * npairs))
    return GPC_E_INVALID;
  return GPC_OK;
}

// A clear of the stats, then one launch per iteration, each reading the block the one before it wrote (gpc::pg_src, pg_dst);
// the cost and the choice are those of the last one.  No launch is timed: the slot table is closed.
template <int C, int R, int NB>
int propagate_run(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                  const gpc_propagate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  const int N = prm->iterations;
  const bool in_place = d_out == d_field;
  const size_t bytes = (size_t)gpc::cl_field_bytes(C, W, H, P);
  if (gpc::pg_needs_ws(N, in_place)) CHK(ensure(c, c->pg_ws, bytes));
  int32_t* block[3] = {const_cast<int32_t*>(d_field), d_out, (int32_t*)c->pg_ws.p};
  if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 4 * (size_t)N * P, c->stream));
  if (gpc::pg_copy_first(N, in_place)) HIPCHK(c, hipMemcpyAsync(block[gpc::PG_WS], d_field, bytes, hipMemcpyDeviceToDevice, c->stream));
  const dim3 tiles((unsigned)gpc::sr_tiles_x(W), (unsigned)gpc::sr_tiles_y(H), (unsigned)P);
  for (int i = 0; i < N; ++i) {
    const bool last = i == N - 1;
    hipLaunchKernelGGL((gpc::k_propagate<C, R, NB>), tiles, dim3(SR_THREADS), 0, c->stream,
                       (const int32_t*)block[gpc::pg_src(i, N, in_place)], d_imgL, d_imgR, W, H, gpc::pg_stride(prm->span, i),
                       block[gpc::pg_dst(i, N)], last ? d_cost : nullptr, last ? d_choice : nullptr,
                       d_stats ? d_stats + 4 * (size_t)i : nullptr, 4 * N);
  }
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

template <int C, int R>
int propagate_neighbours(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                         const gpc_propagate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  return prm->neighbours == 4 ? propagate_run<C, R, 4>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats)
                              : propagate_run<C, R, 8>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
}

template <int C>
int propagate_radius(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int P,
                     const gpc_propagate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice, int32_t* d_stats) {
  switch (prm->radius) {
    case 1: return propagate_neighbours<C, 1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    case 2: return propagate_neighbours<C, 2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    case 3: return propagate_neighbours<C, 3>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
    default: return propagate_neighbours<C, 4>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
  }
}

int propagate_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels, int W,
                            int H, int P, const gpc_propagate* prm, int32_t* d_out, uint16_t* d_cost, uint8_t* d_choice,
                            int32_t* d_stats) {
  return channels == 1 ? propagate_radius<1>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats)
                       : propagate_radius<2>(c, d_field, d_imgL, d_imgR, W, H, P, prm, d_out, d_cost, d_choice, d_stats);
}

}  // namespace

extern "C" {

int gpc_hip_propagate_fields_device(gpc_hip_ctx* c, const int32_t* d_field, const uint8_t* d_imgL, const uint8_t* d_imgR, int channels,
                                    int W, int H, int npairs, const gpc_propagate* prm, int32_t* d_out, uint16_t* d_cost,
                                    uint8_t* d_choice, int32_t* d_stats) {
  CHK(propagate_args(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return propagate_fields_device(c, d_field, d_imgL, d_imgR, channels, W, H, npairs, prm, d_out, d_cost, d_choice, d_stats);
}

// Host form (Stage): chunks of at most 16 pairs -- their fields and images up, their outputs down.
int gpc_hip_propagate_fields(gpc_hip_ctx* c, const int32_t* field, const uint8_t* imgL, const uint8_t* imgR, int channels, int W, int H,
                             int npairs, const gpc_propagate* prm, int32_t* out, uint16_t* cost, uint8_t* choice, int32_t* stats) {
  CHK(propagate_args(c, field, imgL, imgR, channels, W, H, npairs, prm, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H, fb = sizeof(int32_t) * (size_t)channels * n, sb = 16 * (size_t)prm->iterations;
  Stage st(c);
  const size_t r_field = st.in(fb * K), r_l = st.in(n * K), r_r = st.in(n * K);
  const size_t r_out = st.out(fb * K), r_cost = st.out(cost ? 2 * n * K : 0), r_ch = st.out(choice ? n * K : 0);
  const size_t r_sts = st.out(stats ? sb * K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_field, (const uint8_t*)field + fb * (size_t)p0, fb * pc));
    CHK(st.up(r_l, imgL + n * (size_t)p0, n * pc));
    CHK(st.up(r_r, imgR + n * (size_t)p0, n * pc));
    CHK(propagate_fields_device(c, (const int32_t*)st.p(r_field), st.p(r_l), st.p(r_r), channels, W, H, pc, prm, (int32_t*)st.p(r_out),
                                cost ? (uint16_t*)st.p(r_cost) : nullptr, choice ? st.p(r_ch) : nullptr,
                                stats ? (int32_t*)st.p(r_sts) : nullptr));
    CHK(st.down((uint8_t*)out + fb * (size_t)p0, r_out, fb * pc));
    if (cost) CHK(st.down((uint8_t*)cost + 2 * n * (size_t)p0, r_cost, 2 * n * pc));
    if (choice) CHK(st.down(choice + n * (size_t)p0, r_ch, n * pc));
    if (stats) CHK(st.down((uint8_t*)stats + sb * (size_t)p0, r_sts, sb * pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // extern "C"
