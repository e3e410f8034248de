// host_dense.h -- dense maps from sparse matches: the hierarchical fill; records, match-and-fill, host forms.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h and host_refine.h (refine_records).
#pragma once

namespace {

static_assert(sizeof(gpc_densify) == 16 && GPC_DENSE_NONE == DN_NONE, "the parameters and the kernels' view of none");

int dense_args(const gpc_hip_ctx* c, const void* rec, int cap, const void* counts, const void* ref, int W, int H, int npairs,
               const gpc_densify* prm, const void* value) {
  if (!c || !rec || !counts || !value) return GPC_E_INVALID;
  CHK(gpc::dn_params(prm, ref != nullptr));
  return gpc::dn_limits(W, H, npairs, cap);
}

// The launches over records already on the device: clear and claim the owner plane, pull, the levels above the tile, push.
template <bool CORR>
int dense_fill(gpc_hip_ctx* c, const void* d_rec, int cap, const int32_t* d_counts, const gpc_refinement* d_ref, int W, int H,
               int P, const gpc_densify* prm, int32_t* d_value, uint8_t* d_level) {
  typedef gpc::ConsRec<CORR> Rec;
  constexpr int C = CORR ? 2 : 1;
  const gpc::DnGeom g = gpc::dn_geom(W, H, *prm);
  const long cells = (long)gpc::dn_cells(g);
  CHK(ensure(c, c->dn_owner, (size_t)gpc::dn_owner_bytes(W, H, P)));
  CHK(ensure(c, c->dn_n, (size_t)gpc::dn_count_bytes(g, P)));
  CHK(ensure(c, c->dn_s, (size_t)gpc::dn_sum_bytes(g, P, C)));
  uint32_t* owner = (uint32_t*)c->dn_owner.p;
  int32_t* pn = (int32_t*)c->dn_n.p;
  int64_t* ps = (int64_t*)c->dn_s.p;
  const uint2* ref = (const uint2*)d_ref;
  HIPCHK(c, hipMemsetAsync(owner, 0xFF, (size_t)gpc::dn_owner_bytes(W, H, P), c->stream));
  const long nb = ((long)cap + DN_THREADS - 1) / DN_THREADS;
  const dim3 tiles((unsigned)((W + DN_TILE - 1) / DN_TILE), (unsigned)((H + DN_TILE - 1) / DN_TILE), (unsigned)P);
  {
    Timed t(c, KID_DENSE_CLAIM);
    hipLaunchKernelGGL((gpc::k_dense_claim<CORR>), dim3((unsigned)(nb < 4096 ? nb : 4096), P), dim3(DN_THREADS), 0, c->stream,
                       (const Rec*)d_rec, cap, d_counts, ref, prm->max_cost, W, H, owner);
  }
  {
    Timed t(c, KID_DENSE_PULL);
    hipLaunchKernelGGL((gpc::k_dense_pull<CORR>), tiles, dim3(DN_THREADS), 0, c->stream, (const Rec*)d_rec, cap, ref,
                       (const uint32_t*)owner, g, cells, d_value, pn, ps);
  }
  if (g.top > DN_TILE_LEVELS) {
    Timed t(c, KID_DENSE_TOP);
    hipLaunchKernelGGL((gpc::k_dense_top<C>), dim3(P), dim3(DN_THREADS), 0, c->stream, g, cells, pn, ps);
  }
  {
    Timed t(c, KID_DENSE_PUSH);
    hipLaunchKernelGGL((gpc::k_dense_push<C>), tiles, dim3(DN_THREADS), 0, c->stream, g, cells, (const int32_t*)pn,
                       (const int64_t*)ps, d_value, d_level);
  }
  for (int k = KID_DENSE_CLAIM; k <= KID_DENSE_PUSH; ++k)  // (claim and pull are typed by the record, top and push by the channels)
    snprintf(c->launch_name[k], sizeof c->launch_name[0], "gpc::%s<%s>", kKernelNames[k],
             k <= KID_DENSE_PULL ? (CORR ? "true" : "false") : (CORR ? "2" : "1"));
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// match, refine (radius >= 1) and fill, images as all_records takes them
int dense_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s,
                int radius, const gpc_densify* prm, int32_t* d_value, uint8_t* d_level, int32_t* d_counts, int32_t* d_ncand) {
  if (radius < 0 || radius > RF_MAX_RADIUS) return GPC_E_INVALID;
  CHK(gpc::dn_params(prm, radius >= 1));
  AllRecords r;
  CHK(all_records_cap(c, s, W, H, !d_b, &r.cap));
  CHK(gpc::dn_limits(W, H, npairs, r.cap));  // (before any workspace is made, too)
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
  return d_b ? dense_fill<false>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, prm, d_value, d_level)
             : dense_fill<true>(c, r.rec, r.cap, r.counts, d_ref, W, H, npairs, prm, d_value, d_level);
}

// Host forms (Stage): chunks of at most 16 pairs -- their records as far as their counts go, their counts, their refinements.
template <bool CORR>
int dense_host(gpc_hip_ctx* c, const void* rec, int cap, const int32_t* counts, const gpc_refinement* ref, int W, int H,
               int npairs, const gpc_densify* prm, int32_t* value, uint8_t* level) {
  const size_t esz = sizeof(gpc::ConsRec<CORR>), C = CORR ? 2 : 1;
  CHK(dense_args(c, rec, cap, counts, ref, W, H, npairs, prm, value));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H;
  Stage st(c);
  const size_t r_rec = st.in(esz * (size_t)cap * K), r_cnt = st.in(sizeof(int32_t) * (size_t)K);
  const size_t r_ref = st.in(ref ? sizeof(gpc_refinement) * (size_t)cap * K : 0);
  const size_t r_val = st.out(sizeof(int32_t) * C * n * K), r_lev = st.out(level ? n * K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_cnt, counts + p0, sizeof(int32_t) * (size_t)pc));
    CHK(st.up_records(r_rec, rec, esz, cap, counts, p0, pc));
    if (ref) CHK(st.up_records(r_ref, ref, sizeof(gpc_refinement), cap, counts, p0, pc));
    CHK(dense_fill<CORR>(c, st.p(r_rec), cap, (const int32_t*)st.p(r_cnt), ref ? (const gpc_refinement*)st.p(r_ref) : nullptr, W, H, pc,
                         prm, (int32_t*)st.p(r_val), level ? st.p(r_lev) : nullptr));
    CHK(st.down(value + C * n * (size_t)p0, r_val, sizeof(int32_t) * C * n * pc));
    if (level) CHK(st.down(level + n * (size_t)p0, r_lev, n * pc));
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // namespace

extern "C" {

int gpc_hip_densify_supports_device(gpc_hip_ctx* c, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts,
                                    const gpc_refinement* d_ref, int W, int H, int npairs, const gpc_densify* prm, int32_t* d_value,
                                    uint8_t* d_level) {
  CHK(dense_args(c, d_rec, cap_per_pair, d_counts, d_ref, W, H, npairs, prm, d_value));
  HIPCHK(c, hipSetDevice(c->device));
  return dense_fill<false>(c, d_rec, cap_per_pair, d_counts, d_ref, W, H, npairs, prm, d_value, d_level);
}

int gpc_hip_densify_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* d_rec, int cap_per_pair, const int32_t* d_counts,
                                           const gpc_refinement* d_ref, int W, int H, int npairs, const gpc_densify* prm,
                                           int32_t* d_value, uint8_t* d_level) {
  CHK(dense_args(c, d_rec, cap_per_pair, d_counts, d_ref, W, H, npairs, prm, d_value));
  HIPCHK(c, hipSetDevice(c->device));
  return dense_fill<true>(c, d_rec, cap_per_pair, d_counts, d_ref, W, H, npairs, prm, d_value, d_level);
}

int gpc_hip_densify_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                 const gpc_settings* s, int refine_radius, const gpc_densify* prm, int32_t* d_value, uint8_t* d_level,
                                 int32_t* d_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_value || npairs <= 0) return GPC_E_INVALID;
  return dense_match(c, d_rawL, d_rawR, W, H, npairs, s, refine_radius, prm, d_value, d_level, d_counts, d_ncand);
}

int gpc_hip_densify_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                    int refine_radius, const gpc_densify* prm, int32_t* d_value, uint8_t* d_level, int32_t* d_counts,
                                    int32_t* d_ncand) {
  if (!c || !d_frames || !d_value || nframes < 2) return GPC_E_INVALID;
  return dense_match(c, d_frames, nullptr, W, H, nframes - 1, s, refine_radius, prm, d_value, d_level, d_counts, d_ncand);
}

int gpc_hip_densify_supports(gpc_hip_ctx* c, const gpc_support* rec, int cap_per_pair, const int32_t* counts, const gpc_refinement* ref,
                             int W, int H, int npairs, const gpc_densify* prm, int32_t* value, uint8_t* level) {
  return dense_host<false>(c, rec, cap_per_pair, counts, ref, W, H, npairs, prm, value, level);
}

int gpc_hip_densify_correspondences(gpc_hip_ctx* c, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts,
                                    const gpc_refinement* ref, int W, int H, int npairs, const gpc_densify* prm, int32_t* value,
                                    uint8_t* level) {
  return dense_host<true>(c, rec, cap_per_pair, counts, ref, W, H, npairs, prm, value, level);
}

}  // extern "C"
