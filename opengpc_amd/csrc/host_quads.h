// host_quads.h -- stereo sequences: the three joins over one hashing (gpc_hip_match_stereo_sequence_device), the circular
// matches closed into quads (k_quad.h), host forms.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h (Stage).
#pragma once

#define QD_PLANE_BYTES ((size_t)1 << 30)  // what the planes and owner words of one group of steps may take (the candidate words,
                                          // 4 bytes per support slot more, are a block of their own and not counted)

namespace {

static_assert(sizeof(gpc_quad) == sizeof(gpc::QdQuad) && sizeof(gpc_quad) == 32, "gpc_quad and the kernels' view of it");
static_assert(sizeof(gpc_support) == sizeof(gpc::QdSup), "gpc_support and the kernels' view of it");

int quad_args(const gpc_hip_ctx* c, const void* sup, int cap_s, const void* nsup, const void* fl, const void* fr, int cap_f,
              const void* nfl, const void* nfr, int W, int H, int N, int tol, const void* quads, int quad_cap, const void* nquads) {
  if (!c || !sup || !nsup || !fl || !fr || !nfl || !nfr || !nquads || W <= 0 || H <= 0) return GPC_E_INVALID;
  if (tol < 0 || tol > 255 || N < 2 || cap_s <= 0 || cap_f <= 0 || quad_cap < 0 || (quad_cap > 0 && !quads)) return GPC_E_INVALID;
  // a pixel index takes 30 bits; a record slot's number in the whole call 31; a launch has one grid row per step and plane
  if ((long)W * H > (1l << 30) || N > 65535 || (long)N * cap_s > 0x7FFFFFFFl || (long)(N - 1) * cap_f > 0x7FFFFFFFl ||
      (long)(N - 1) * quad_cap > 0x7FFFFFFFl)
    return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// steps that go through the launches together: what QD_PLANE_BYTES holds (3 planes per step, one more for the group's last
// frame, and the owner words), at least one
int quad_group(const gpc_hip_ctx* c, size_t n, int cap_s, int P) {
  const size_t per_step = sizeof(int32_t) * (3 * n + (size_t)cap_s);
  size_t g = QD_PLANE_BYTES > sizeof(int32_t) * n ? (QD_PLANE_BYTES - sizeof(int32_t) * n) / per_step : 0;
  if (g > 21000) g = 21000;  // (k_quad_scatter: 3 g + 1 grid rows)
  if (c->quad_steps > 0 && (size_t)c->quad_steps < g) g = (size_t)c->quad_steps;
  if (g < 1) g = 1;
  return g < (size_t)P ? (int)g : P;
}

// The six launches per group of steps over records already on the device.  Planes and owner words are FILLED first, as for
// the tracks: a minimum needs a start value above every index.  A group's last frame is the next group's first: its plane
// is scattered again there.
int quad_close(gpc_hip_ctx* c, const gpc_support* d_sup, int cap_s, const int32_t* d_nsup, const gpc_correspondence* d_fl,
               const gpc_correspondence* d_fr, int cap_f, const int32_t* d_nfl, const int32_t* d_nfr, int W, int H, int N, int tol,
               gpc_quad* d_quads, int quad_cap, int32_t* d_nquads) {
  const size_t n = (size_t)W * H;
  const int P = N - 1, G = quad_group(c, n, cap_s, P);
  const long nchunk = ((long)cap_s + QD_CHUNK - 1) / QD_CHUNK;
  const size_t words = ((3 * (size_t)G + 1) * n + (size_t)G * cap_s + 3) / 4 * 4;  // (whole 16-byte groups: the fill's unit)
  CHK(ensure(c, c->qd_plane, sizeof(int32_t) * words));
  CHK(ensure(c, c->qd_sel, sizeof(int32_t) * (size_t)G * cap_s));
  CHK(ensure(c, c->qd_blk, sizeof(int32_t) * (size_t)G * nchunk));
  const long most = (long)(cap_s > cap_f ? cap_s : cap_f);
  const long sb = (most + QD_THREADS - 1) / QD_THREADS, cb = ((long)cap_s + QD_THREADS - 1) / QD_THREADS;
  for (int t0 = 0; t0 < P; t0 += G) {
    const int g = P - t0 < G ? P - t0 : G;
    gpc::QdArgs a;
    a.sup = (const gpc::QdSup*)d_sup + (size_t)t0 * cap_s;
    a.nsup = d_nsup + t0;
    a.fl = (const gpc::TrRec*)d_fl + (size_t)t0 * cap_f;
    a.fr = (const gpc::TrRec*)d_fr + (size_t)t0 * cap_f;
    a.nfl = d_nfl + t0;
    a.nfr = d_nfr + t0;
    a.first_s = (int32_t*)c->qd_plane.p;
    a.first_fl = a.first_s + (size_t)(g + 1) * n;
    a.first_fr = a.first_fl + (size_t)g * n;
    a.owner = a.first_fr + (size_t)g * n;
    a.cand = (int32_t*)c->qd_sel.p;
    a.blk = (int32_t*)c->qd_blk.p;
    a.cap_s = cap_s, a.cap_f = cap_f, a.W = W, a.H = H, a.steps = g, a.tol = tol, a.nchunk = (int)nchunk;
    const long n16 = (long)(((3 * (size_t)g + 1) * n + (size_t)g * cap_s + 3) / 4);  // (g <= G: within `words`)
    const long fb = (n16 + TR_THREADS - 1) / TR_THREADS;
    const dim3 cgrid((unsigned)nchunk, g);
    {
      Timed t(c, KID_QUAD_FILL);
      hipLaunchKernelGGL(gpc::k_track_fill, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(TR_THREADS), 0, c->stream, (int4*)a.first_s, n16);
    }
    {
      Timed t(c, KID_QUAD_SCATTER);
      hipLaunchKernelGGL(gpc::k_quad_scatter, dim3((unsigned)(sb < 256 ? sb : 256), 3 * g + 1), dim3(QD_THREADS), 0, c->stream, a);
    }
    {
      Timed t(c, KID_QUAD_CLOSE);
      hipLaunchKernelGGL(gpc::k_quad_close, dim3((unsigned)(cb < 1024 ? cb : 1024), g), dim3(QD_THREADS), 0, c->stream, a);
    }
    {
      Timed t(c, KID_QUAD_SETTLE);
      hipLaunchKernelGGL(gpc::k_quad_settle, cgrid, dim3(QD_THREADS), 0, c->stream, a);
    }
    {
      Timed t(c, KID_QUAD_SCAN);
      hipLaunchKernelGGL(gpc::k_quad_scan, dim3(g), dim3(1024), 0, c->stream, a.blk, (int)nchunk, d_nquads + t0);
    }
    if (quad_cap > 0) {
      Timed t(c, KID_QUAD_WRITE);
      hipLaunchKernelGGL(gpc::k_quad_write, cgrid, dim3(QD_THREADS), 0, c->stream, a, (gpc::QdQuad*)d_quads + (size_t)t0 * quad_cap, quad_cap);
    }
  }
  snprintf(c->launch_name[KID_QUAD_FILL], sizeof c->launch_name[0], "gpc::k_track_fill");
  for (int k = KID_QUAD_SCATTER; k <= KID_QUAD_WRITE; ++k) snprintf(c->launch_name[k], sizeof c->launch_name[0], "gpc::%s", kKernelNames[k]);
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

int stereo_sequence_usable(gpc_hip_ctx* c, const void* left, const void* right, int W, int H, int N, const gpc_settings* ss,
                           const gpc_settings* fs, const void* sup, int cap_s, const void* nsup, const void* fl, const void* fr, int cap_f,
                           const void* nfl, const void* nfr) {
  if (!c || !left || !right || !sup || !nsup || !fl || !fr || !nfl || !nfr || N < 2 || cap_s <= 0 || cap_f <= 0) return GPC_E_INVALID;
  CHK(check_settings(ss));
  CHK(check_settings(fs));
  if (ss->gradient_threshold != fs->gradient_threshold) return GPC_E_INVALID;  // (one k_preprocess serves both)
  if (c->ngroups > 1) return GPC_E_UNSUPPORTED;
  CHK(match_usable(c, ss, W, H, false));
  return match_usable(c, fs, W, H, true);
}

// the context's code images (and, for 32-bit codes, candidate bytes) stand aside for one side's image-major copies while a
// flow join runs
// (run_match and what it calls never ensure() c->codes or c->stats: their callers do, before the match, as here)
struct SideScope {
  gpc_hip_ctx* c;
  int side;
  SideScope(gpc_hip_ctx* ctx, int k) : c(ctx), side(k) { std::swap(c->codes, c->qd_codes[side]); }
  ~SideScope() { std::swap(c->codes, c->qd_codes[side]); }
};

}  // namespace

extern "C" {

int gpc_hip_quads_records_device(gpc_hip_ctx* c, const gpc_support* d_sup, int cap_s, const int32_t* d_nsup,
                                 const gpc_correspondence* d_flowL, const gpc_correspondence* d_flowR, int cap_f,
                                 const int32_t* d_nflowL, const int32_t* d_nflowR, int W, int H, int nframes, int tol,
                                 gpc_quad* d_quads, int quad_cap, int32_t* d_nquads) {
  CHK(quad_args(c, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, W, H, nframes, tol, d_quads, quad_cap, d_nquads));
  HIPCHK(c, hipSetDevice(c->device));
  return quad_close(c, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, W, H, nframes, tol, d_quads, quad_cap, d_nquads);
}

// One k_preprocess and one k_hash over the 2 N images, stored [t][side] as a batch stores them: the stereo join reads them
// where they lie.  A flow join reads consecutive images, so each side's code images (4 bytes per pixel; with 32-bit codes
// the candidate bytes too) and statistics words are copied once into an image-major block of their own (k_quad_sides), and
// the sequence matcher runs over that block as it runs over the frames of gpc_hip_match_sequence_device.
int gpc_hip_match_stereo_sequence_device(gpc_hip_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int W, int H, int nframes,
                                         const gpc_settings* ss, const gpc_settings* fs, gpc_support* d_sup, int cap_s,
                                         int32_t* d_nsup, gpc_correspondence* d_flowL, gpc_correspondence* d_flowR, int cap_f,
                                         int32_t* d_nflowL, int32_t* d_nflowR, int32_t* d_ncand) {
  CHK(stereo_sequence_usable(c, d_left, d_right, W, H, nframes, ss, fs, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR));
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pipeline > 1) CHK(drain_lanes(c));
  StrictScope strict(c);
  const size_t n = (size_t)W * H;
  const int N = nframes, P = N - 1;
  const size_t stat_bytes = sizeof(int32_t) * GPC_STAT_STRIDE;
  CHK(ensure(c, c->codes, sizeof(uint32_t) * n * 2 * N));
  CHK(ensure(c, c->sstats, stat_bytes * 2 * P));
  CHK(ensure(c, c->qd_stats, stat_bytes * 2 * N));
  const bool wide = wide_codes(c);
  for (int k = 0; k < 2; ++k) {
    CHK(ensure(c, c->qd_codes[k], sizeof(uint32_t) * n * N));
    if (wide) CHK(ensure(c, c->qd_gcand[k], n * N));
  }
  CHK(run_preprocess(c, d_left, d_right, W, H, N, 2, ss->gradient_threshold, true));
  CHK(run_hash(c, (const uint8_t*)c->smooth.p, (const uint8_t*)c->grad.p, nullptr, W, H, 2 * N, false, (uint32_t*)c->codes.p));
  {
    Timed t(c, KID_QUAD_SIDES);
    const long g_code = (long)(n / 4), g_cand = (long)(n / 16), gb = (g_code + QD_THREADS - 1) / QD_THREADS;  // (W % 16 == 0: check_dims)
    hipLaunchKernelGGL(gpc::k_quad_sides, dim3((unsigned)(gb < 64 ? gb : 64), N, 2), dim3(QD_THREADS), 0, c->stream,
                       (const uint4*)c->codes.p, (uint4*)c->qd_codes[0].p, (uint4*)c->qd_codes[1].p, g_code,
                       wide ? (const uint4*)c->grad.p : (const uint4*)nullptr, (uint4*)c->qd_gcand[0].p, (uint4*)c->qd_gcand[1].p,
                       g_cand, (const int32_t*)c->stats.p, (int32_t*)c->qd_stats.p);
    snprintf(c->launch_name[KID_QUAD_SIDES], sizeof c->launch_name[0], "gpc::k_quad_sides");
    HIPCHK(c, hipGetLastError());
  }
  CHK(run_match(c, W, H, N, ss, 0, (const uint8_t*)c->grad.p, d_sup, cap_s, d_nsup, nullptr));
  const int nthr = 2 * P * GPC_STAT_STRIDE;  // (>= N)
  for (int k = 0; k < 2; ++k) {
    hipLaunchKernelGGL(gpc::k_seq_stats, dim3((nthr + 255) / 256), dim3(256), 0, c->stream,
                       (const int32_t*)c->qd_stats.p + (size_t)k * GPC_STAT_STRIDE * N, (int32_t*)c->sstats.p,
                       d_ncand ? d_ncand + (size_t)k * N : nullptr, N);
    HIPCHK(c, hipGetLastError());
    SideScope side(c, k);
    std::swap(c->stats, c->sstats);
    const int st = run_match(c, W, H, P, fs, 1, wide ? (const uint8_t*)c->qd_gcand[k].p : (const uint8_t*)c->grad.p,
                             k ? d_flowR : d_flowL, cap_f, k ? d_nflowR : d_nflowL, nullptr, nullptr, true);
    std::swap(c->stats, c->sstats);
    CHK(st);
  }
  return GPC_OK;
}

int gpc_hip_quads_sequence_device(gpc_hip_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int W, int H, int nframes,
                                  const gpc_settings* ss, const gpc_settings* fs, int tol, gpc_support* d_sup, int cap_s,
                                  int32_t* d_nsup, gpc_correspondence* d_flowL, gpc_correspondence* d_flowR, int cap_f,
                                  int32_t* d_nflowL, int32_t* d_nflowR, int32_t* d_ncand, gpc_quad* d_quads, int quad_cap,
                                  int32_t* d_nquads) {
  CHK(quad_args(c, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, W, H, nframes, tol, d_quads, quad_cap, d_nquads));
  CHK(gpc_hip_match_stereo_sequence_device(c, d_left, d_right, W, H, nframes, ss, fs, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f,
                                           d_nflowL, d_nflowR, d_ncand));
  return quad_close(c, d_sup, cap_s, d_nsup, d_flowL, d_flowR, cap_f, d_nflowL, d_nflowR, W, H, nframes, tol, d_quads, quad_cap, d_nquads);
}

}  // extern "C"

// Host forms (Stage): the whole call in one block, the device form once over it (a quad joins records of two steps' frames,
// and the planes are per call: nothing is gained by chunks).
namespace {

struct QuadRegions {
  size_t left, right, sup, nsup, fl, fr, nfl, nfr, nc, quads, nq;
};

// frame_bytes: the frames of one side in the sequence form, whose records and counts come down; 0: the records form
int quad_layout(Stage& st, size_t frame_bytes, int N, int cap_s, int cap_f, int quad_cap, QuadRegions* r) {
  const size_t P = (size_t)N - 1, srec = sizeof(gpc_support) * (size_t)N * cap_s, frec = sizeof(gpc_correspondence) * P * cap_f;
  const bool up = frame_bytes == 0;
  r->left = st.in(frame_bytes), r->right = st.in(frame_bytes);
  r->sup = up ? st.in(srec) : st.out(srec);
  r->fl = up ? st.in(frec) : st.out(frec);
  r->fr = up ? st.in(frec) : st.out(frec);
  r->nsup = up ? st.in(sizeof(int32_t) * (size_t)N) : st.out(sizeof(int32_t) * (size_t)N);
  r->nfl = up ? st.in(sizeof(int32_t) * P) : st.out(sizeof(int32_t) * P);
  r->nfr = up ? st.in(sizeof(int32_t) * P) : st.out(sizeof(int32_t) * P);
  r->nc = st.out(sizeof(int32_t) * 2 * (size_t)N);
  r->quads = st.out(sizeof(gpc_quad) * P * quad_cap), r->nq = st.out(sizeof(int32_t) * P);
  return st.alloc(sizeof(int32_t) * (3 * (size_t)N + 3 * P));  // nsup [N], nfl, nfr, nq [P] each, candidates [2][N]
}

// the counts first, then what they say is valid.  sup .. ncand: null where the form does not hand them back
int quad_down(Stage& st, const QuadRegions& r, int N, int cap_s, int cap_f, int quad_cap, gpc_support* sup, int32_t* nsup,
              gpc_correspondence* fl, gpc_correspondence* fr, int32_t* nfl, int32_t* nfr, int32_t* ncand, gpc_quad* quads,
              int32_t* nquads, int status) {
  const int P = N - 1;
  int32_t* hs = st.c->h_cnt.p;
  int32_t *hl = hs + N, *hr = hl + P, *hq = hr + P, *hn = hq + P;
  if (sup) {
    CHK(st.down(hs, r.nsup, sizeof(int32_t) * (size_t)N));
    CHK(st.down(hl, r.nfl, sizeof(int32_t) * (size_t)P));
    CHK(st.down(hr, r.nfr, sizeof(int32_t) * (size_t)P));
    if (ncand) CHK(st.down(hn, r.nc, sizeof(int32_t) * 2 * (size_t)N));
  }
  CHK(st.down(hq, r.nq, sizeof(int32_t) * (size_t)P));
  CHK(st.wait());
  for (int t = 0; sup && t < N; ++t) {
    const size_t m = (size_t)valid_records(hs[t], cap_s), at = (size_t)t * cap_s;
    if (hs[t] > cap_s) status = GPC_E_CAPACITY;
    if (m) CHK(st.down(sup + at, r.sup + sizeof(gpc_support) * at, sizeof(gpc_support) * m));
  }
  for (int t = 0; t < P; ++t) {
    const size_t at = (size_t)t * cap_f, qat = (size_t)t * quad_cap;
    if (sup) {
      const size_t ml = (size_t)valid_records(hl[t], cap_f), mr = (size_t)valid_records(hr[t], cap_f);
      if (hl[t] > cap_f || hr[t] > cap_f) status = GPC_E_CAPACITY;
      if (ml) CHK(st.down(fl + at, r.fl + sizeof(gpc_correspondence) * at, sizeof(gpc_correspondence) * ml));
      if (mr) CHK(st.down(fr + at, r.fr + sizeof(gpc_correspondence) * at, sizeof(gpc_correspondence) * mr));
    }
    const size_t mq = (size_t)valid_records(hq[t], quad_cap);
    if (hq[t] > quad_cap) status = GPC_E_CAPACITY;
    if (mq) CHK(st.down(quads + qat, r.quads + sizeof(gpc_quad) * qat, sizeof(gpc_quad) * mq));
  }
  CHK(st.wait());
  if (sup) {
    memcpy(nsup, hs, sizeof(int32_t) * (size_t)N);
    memcpy(nfl, hl, sizeof(int32_t) * (size_t)P);
    memcpy(nfr, hr, sizeof(int32_t) * (size_t)P);
    if (ncand) memcpy(ncand, hn, sizeof(int32_t) * 2 * (size_t)N);
  }
  memcpy(nquads, hq, sizeof(int32_t) * (size_t)P);
  CHK(check_join_err(st.c));
  return status;
}

}  // namespace

extern "C" {

int gpc_hip_quads_records(gpc_hip_ctx* c, const gpc_support* sup, int cap_s, const int32_t* nsup, const gpc_correspondence* flowL,
                          const gpc_correspondence* flowR, int cap_f, const int32_t* nflowL, const int32_t* nflowR, int W, int H,
                          int nframes, int tol, gpc_quad* quads, int quad_cap, int32_t* nquads) {
  CHK(quad_args(c, sup, cap_s, nsup, flowL, flowR, cap_f, nflowL, nflowR, W, H, nframes, tol, quads, quad_cap, nquads));
  CHK(host_call_begin(c));
  const int N = nframes, P = N - 1;
  Stage st(c);
  QuadRegions r;
  CHK(quad_layout(st, 0, N, cap_s, cap_f, quad_cap, &r));
  CHK(st.up(r.nsup, nsup, sizeof(int32_t) * (size_t)N));
  CHK(st.up(r.nfl, nflowL, sizeof(int32_t) * (size_t)P));
  CHK(st.up(r.nfr, nflowR, sizeof(int32_t) * (size_t)P));
  CHK(st.up_records(r.sup, sup, sizeof(gpc_support), cap_s, nsup, 0, N));
  CHK(st.up_records(r.fl, flowL, sizeof(gpc_correspondence), cap_f, nflowL, 0, P));
  CHK(st.up_records(r.fr, flowR, sizeof(gpc_correspondence), cap_f, nflowR, 0, P));
  CHK(quad_close(c, (const gpc_support*)st.p(r.sup), cap_s, (const int32_t*)st.p(r.nsup), (const gpc_correspondence*)st.p(r.fl),
                 (const gpc_correspondence*)st.p(r.fr), cap_f, (const int32_t*)st.p(r.nfl), (const int32_t*)st.p(r.nfr), W, H, N, tol,
                 (gpc_quad*)st.p(r.quads), quad_cap, (int32_t*)st.p(r.nq)));
  int status = GPC_OK;
  for (int t = 0; t < N; ++t)
    if (nsup[t] > cap_s || (t < P && (nflowL[t] > cap_f || nflowR[t] > cap_f))) status = GPC_E_CAPACITY;
  return quad_down(st, r, N, cap_s, cap_f, quad_cap, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, quads, nquads, status);
}

int gpc_hip_quads_sequence(gpc_hip_ctx* c, const uint8_t* left, const uint8_t* right, int W, int H, int nframes,
                           const gpc_settings* ss, const gpc_settings* fs, int tol, gpc_support* sup, int cap_s, int32_t* nsup,
                           gpc_correspondence* flowL, gpc_correspondence* flowR, int cap_f, int32_t* nflowL, int32_t* nflowR,
                           int32_t* ncand, gpc_quad* quads, int quad_cap, int32_t* nquads) {
  CHK(quad_args(c, sup, cap_s, nsup, flowL, flowR, cap_f, nflowL, nflowR, W, H, nframes, tol, quads, quad_cap, nquads));
  CHK(stereo_sequence_usable(c, left, right, W, H, nframes, ss, fs, sup, cap_s, nsup, flowL, flowR, cap_f, nflowL, nflowR));
  CHK(host_call_begin(c));
  const size_t n = (size_t)W * H;
  const int N = nframes;
  Stage st(c);
  QuadRegions r;
  CHK(quad_layout(st, n * N, N, cap_s, cap_f, quad_cap, &r));
  CHK(st.up(r.left, left, n * N));
  CHK(st.up(r.right, right, n * N));
  CHK(gpc_hip_quads_sequence_device(c, st.p(r.left), st.p(r.right), W, H, N, ss, fs, tol, (gpc_support*)st.p(r.sup), cap_s,
                                    (int32_t*)st.p(r.nsup), (gpc_correspondence*)st.p(r.fl), (gpc_correspondence*)st.p(r.fr), cap_f,
                                    (int32_t*)st.p(r.nfl), (int32_t*)st.p(r.nfr), (int32_t*)st.p(r.nc), (gpc_quad*)st.p(r.quads),
                                    quad_cap, (int32_t*)st.p(r.nq)));
  return quad_down(st, r, N, cap_s, cap_f, quad_cap, sup, nsup, flowL, flowR, nflowL, nflowR, ncand, quads, nquads, GPC_OK);
}

}  // extern "C"
