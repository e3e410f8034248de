// host_refine.h -- match refinement: sub-pixel position and photometric cost; records, match-and-refine, host forms.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h.
#pragma once

namespace {

static_assert(sizeof(gpc_refinement) == sizeof(uint2), "the results and the kernel's view of them");

// rec / out: [npairs][cap] records of esz bytes
int refine_args(const gpc_hip_ctx* c, const void* rec, size_t esz, int cap, const void* counts, const void* imgL,
                const void* imgR, int W, int H, int npairs, int radius, const void* ref, const void* out) {
  if (!c || !rec || !counts || !imgL || !imgR || !ref || npairs < 1 || cap < 1 || W < 1 || H < 1) return GPC_E_INVALID;
  if (radius < 1 || radius > RF_MAX_RADIUS) return GPC_E_INVALID;
  // a launch has one grid row per pair, a record's number in the whole call and a pixel's in an image fit an int
  if (npairs > 65535 || (long)npairs * cap > 0x7FFFFFFFl || (long)W * H > (1l << 30)) return GPC_E_UNSUPPORTED;
  if (out) {
    const uintptr_t r0 = (uintptr_t)rec, r1 = r0 + esz * (size_t)npairs * (size_t)cap, o0 = (uintptr_t)out;
    if (r0 < o0 + esz * (size_t)npairs * (size_t)cap && o0 < r1) return GPC_E_INVALID;  // (the kernel reads and writes without order)
  }
  return GPC_OK;
}

// The launch over records and images already on the device.
template <bool CORR, int R>
void refine_launch(gpc_hip_ctx* c, dim3 grid, const void* d_rec, int cap, const int32_t* d_counts, const uint8_t* d_L,
                   const uint8_t* d_R, int W, int H, gpc_refinement* d_ref, gpc_support* d_out) {
  hipLaunchKernelGGL((gpc::k_refine<CORR, R>), grid, dim3(RF_THREADS), 0, c->stream, (const gpc::ConsRec<CORR>*)d_rec, cap, d_counts,
                     d_L, d_R, W, H, (uint2*)d_ref, (gpc::ConsRec<false>*)d_out);
}

template <bool CORR>
int refine_records(gpc_hip_ctx* c, const void* d_rec, int cap, const int32_t* d_counts, const uint8_t* d_L, const uint8_t* d_R,
                   int W, int H, int P, int radius, gpc_refinement* d_ref, gpc_support* d_out) {
  const long nb = ((long)cap + RF_THREADS - 1) / RF_THREADS;
  const dim3 grid((unsigned)(nb < 4096 ? nb : 4096), P);
  {
    Timed t(c, KID_REFINE);
    switch (radius) {
      case 1: refine_launch<CORR, 1>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
      case 2: refine_launch<CORR, 2>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
      case 3: refine_launch<CORR, 3>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
      case 4: refine_launch<CORR, 4>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
      case 5: refine_launch<CORR, 5>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
      default: refine_launch<CORR, 6>(c, grid, d_rec, cap, d_counts, d_L, d_R, W, H, d_ref, d_out); break;
    }
  }
  snprintf(c->launch_name[KID_REFINE], sizeof c->launch_name[0], "gpc::k_refine<%s, %d>", CORR ? "true" : "false", radius);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// Host forms (Stage): chunks of at most 16 pairs -- their records as far as their counts go, their counts, both images.
template <bool CORR>
int refine_host(gpc_hip_ctx* c, const void* rec, int cap, const int32_t* counts, const uint8_t* imgL, const uint8_t* imgR, int W,
                int H, int npairs, int radius, gpc_refinement* ref, gpc_support* out) {
  const size_t esz = sizeof(gpc::ConsRec<CORR>);
  CHK(refine_args(c, rec, esz, cap, counts, imgL, imgR, W, H, npairs, radius, ref, out));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  const size_t n = (size_t)W * H;
  Stage st(c);
  const size_t r_rec = st.in(esz * (size_t)cap * K), r_cnt = st.in(sizeof(int32_t) * (size_t)K), r_L = st.in(n * K), r_R = st.in(n * K);
  const size_t r_ref = st.out(sizeof(gpc_refinement) * (size_t)cap * K), r_out = st.out(out ? esz * (size_t)cap * K : 0);
  CHK(st.alloc(0));
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_cnt, counts + p0, sizeof(int32_t) * (size_t)pc));
    CHK(st.up_records(r_rec, rec, esz, cap, counts, p0, pc));
    CHK(st.up(r_L, imgL + n * p0, n * pc));
    CHK(st.up(r_R, imgR + n * p0, n * pc));
    CHK(refine_records<CORR>(c, st.p(r_rec), cap, (const int32_t*)st.p(r_cnt), st.p(r_L), st.p(r_R), W, H, pc, radius,
                             (gpc_refinement*)st.p(r_ref), out ? (gpc_support*)st.p(r_out) : nullptr));
    for (int t = 0; t < pc; ++t) {  // a pair's results as far as its records go
      const size_t m = (size_t)valid_records(counts[p0 + t], cap), q = (size_t)(p0 + t);
      if (!m) continue;
      CHK(st.down(ref + q * cap, r_ref + sizeof(gpc_refinement) * (size_t)t * cap, sizeof(gpc_refinement) * m));
      if (out) CHK(st.down(out + q * cap, r_out + esz * (size_t)t * cap, esz * m));
    }
    CHK(st.wait());
  }
  return check_join_err(c);
}

}  // namespace

extern "C" {

int gpc_hip_refine_supports_device(gpc_hip_ctx* c, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts,
                                   const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int npairs, int radius,
                                   gpc_refinement* d_ref, gpc_support* d_out) {
  CHK(refine_args(c, d_rec, sizeof(gpc_support), cap_per_pair, d_counts, d_imgL, d_imgR, W, H, npairs, radius, d_ref, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  return refine_records<false>(c, d_rec, cap_per_pair, d_counts, d_imgL, d_imgR, W, H, npairs, radius, d_ref, d_out);
}

int gpc_hip_refine_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* d_rec, int cap_per_pair, const int32_t* d_counts,
                                          const uint8_t* d_imgL, const uint8_t* d_imgR, int W, int H, int npairs, int radius,
                                          gpc_refinement* d_ref) {
  CHK(refine_args(c, d_rec, sizeof(gpc_correspondence), cap_per_pair, d_counts, d_imgL, d_imgR, W, H, npairs, radius, d_ref, nullptr));
  HIPCHK(c, hipSetDevice(c->device));
  return refine_records<true>(c, d_rec, cap_per_pair, d_counts, d_imgL, d_imgR, W, H, npairs, radius, d_ref, nullptr);
}

// Match, then refine over the raw images.  The match is the plain call on the context itself (lanes drained, as
// all_records has it): what it refuses is refused, its status is the call's.
int gpc_hip_refine_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                const gpc_settings* s, int radius, gpc_support* d_supports, int cap_per_pair, int32_t* d_counts,
                                int32_t* d_ncand, gpc_refinement* d_ref, gpc_support* d_out) {
  if (!c || !d_rawL || !d_rawR || !d_supports || !d_counts || npairs <= 0 || cap_per_pair <= 0) return GPC_E_INVALID;
  CHK(check_settings(s));
  CHK(check_dims(W, H));
  CHK(refine_args(c, d_supports, sizeof(gpc_support), cap_per_pair, d_counts, d_rawL, d_rawR, W, H, npairs, radius, d_ref, d_out));
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));
  CHK(match_batch_strict(c, d_rawL, d_rawR, W, H, npairs, s, d_supports, cap_per_pair, d_counts, d_ncand));
  return refine_records<false>(c, d_supports, cap_per_pair, d_counts, d_rawL, d_rawR, W, H, npairs, radius, d_ref, d_out);
}

int gpc_hip_refine_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                   int radius, gpc_correspondence* d_corr, int cap_per_pair, int32_t* d_counts, int32_t* d_ncand,
                                   gpc_refinement* d_ref) {
  if (!c || !d_frames || !d_corr || !d_counts || nframes < 2 || cap_per_pair <= 0) return GPC_E_INVALID;
  CHK(match_usable(c, s, W, H, true));
  const uint8_t* d_next = d_frames + (size_t)W * H;
  CHK(refine_args(c, d_corr, sizeof(gpc_correspondence), cap_per_pair, d_counts, d_frames, d_next, W, H, nframes - 1, radius, d_ref, nullptr));
  CHK(gpc_hip_match_sequence_device(c, d_frames, W, H, nframes, s, d_corr, cap_per_pair, d_counts, d_ncand));
  return refine_records<true>(c, d_corr, cap_per_pair, d_counts, d_frames, d_next, W, H, nframes - 1, radius, d_ref, nullptr);
}

int gpc_hip_refine_supports(gpc_hip_ctx* c, const gpc_support* rec, int cap_per_pair, const int32_t* counts, const uint8_t* imgL,
                            const uint8_t* imgR, int W, int H, int npairs, int radius, gpc_refinement* ref, gpc_support* out) {
  return refine_host<false>(c, rec, cap_per_pair, counts, imgL, imgR, W, H, npairs, radius, ref, out);
}

int gpc_hip_refine_correspondences(gpc_hip_ctx* c, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts,
                                   const uint8_t* imgL, const uint8_t* imgR, int W, int H, int npairs, int radius,
                                   gpc_refinement* ref) {
  return refine_host<true>(c, rec, cap_per_pair, counts, imgL, imgR, W, H, npairs, radius, ref, nullptr);
}

}  // extern "C"
