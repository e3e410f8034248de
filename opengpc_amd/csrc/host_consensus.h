// host_consensus.h -- match filtering by grid motion consensus: records, match-and-filter, and their host forms.
// A piece of gpc_hip.hip, included where the section stood: it needs what that file defines above the include
// and, before it, host_staging.h.
#pragma once

namespace {

static_assert(sizeof(gpc_support) == sizeof(gpc::ConsRec<false>) && sizeof(gpc_correspondence) == sizeof(gpc::ConsRec<true>),
              "the records and the kernels' view of them");

int cons_params(const gpc_consensus* p) {
  if (!p) return GPC_E_INVALID;
  if (p->cell < 4 || p->cell > 256 || (p->cell & 1) || (p->shifts != 1 && p->shifts != 4)) return GPC_E_INVALID;
  if (p->alpha_num < 0 || p->alpha_num > 1024 || p->alpha_den < 1 || p->alpha_den > 64) return GPC_E_INVALID;
  return GPC_OK;
}

// S and T stay below 2^24 (the products of the test are exact, the kernels multiply 24-bit values), a cell index and a
// class below 2^26, a record's number in the whole call below 2^31, and a launch has one grid row per pair
int cons_limits(long cap, int W, int H, int npairs, int cell) {
  const long cw = ((long)W + cell - 1) / cell, ch = ((long)H + cell - 1) / cell;
  if (cap > (1l << 23) || cw * ch > (1l << 22) || npairs > 65535 || (long)npairs * cap > 0x7FFFFFFFl) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

int cons_args(const gpc_hip_ctx* c, const void* rec, size_t esz, int cap, const void* counts, int W, int H, int npairs,
              const gpc_consensus* prm, const void* out, int cap_out, const void* out_counts) {
  if (!c || !rec || !counts || !out || !out_counts || npairs < 1 || cap <= 0 || cap_out <= 0 || W <= 0 || H <= 0) return GPC_E_INVALID;
  CHK(cons_params(prm));
  CHK(cons_limits(cap, W, H, npairs, prm->cell));
  const uintptr_t r0 = (uintptr_t)rec, r1 = r0 + esz * (size_t)npairs * (size_t)cap;
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + esz * (size_t)npairs * (size_t)cap_out;
  if (r0 < o1 && o0 < r1) return GPC_E_INVALID;  // (kept records are written while later ones are still read)
  return GPC_OK;
}

gpc::ConsGrid cons_grid(int W, int H, const gpc_consensus* prm, int s) {
  gpc::ConsGrid g;
  const int cl = prm->cell;
  g.W = W, g.H = H;
  g.ox = (s & 1) ? cl / 2 : 0;
  g.oy = (s & 2) ? cl / 2 : 0;
  g.gx = (W - 1 + g.ox) / cl + 1;
  g.gy = (H - 1 + g.oy) / cl + 1;
  g.ncell = g.gx * g.gy;
  g.kw = 2u * (uint32_t)g.gx - 1u;
  g.dc = make_divw(cl);
  g.dgx = make_divw(g.gx > 1 ? g.gx : 2);
  g.bit = 1u << s;
  g.kq = (uint32_t)(prm->alpha_den * prm->alpha_den);
  g.an2 = (uint32_t)(prm->alpha_num * prm->alpha_num);
  return g;
}

// The launches over records already on the device: four per grid, then three that compact.
template <bool CORR>
int cons_filter(gpc_hip_ctx* c, const void* d_rec, int cap, const int32_t* d_counts, int W, int H, int P,
                const gpc_consensus* prm, uint8_t* d_keep, void* d_out, int cap_out, int32_t* d_index,
                int32_t* d_out_counts) {
  typedef gpc::ConsRec<CORR> Rec;
  size_t maxcell = 0;
  for (int s = 0; s < prm->shifts; ++s) maxcell = std::max(maxcell, (size_t)cons_grid(W, H, prm, s).ncell);
  const long nchunk = ((long)cap + CS_CHUNK - 1) / CS_CHUNK;
  CHK(ensure(c, c->cs_key, sizeof(uint32_t) * (size_t)cap * P));
  CHK(ensure(c, c->cs_idx, sizeof(int32_t) * (size_t)cap * P));
  CHK(ensure(c, c->cs_cur, sizeof(int32_t) * maxcell * P));
  CHK(ensure(c, c->cs_start, sizeof(int32_t) * (maxcell + 1) * P));
  CHK(ensure(c, c->cs_blk, sizeof(int32_t) * (size_t)nchunk * P));
  if (!d_keep) {
    CHK(ensure(c, c->cs_keep, (size_t)cap * P));
    d_keep = (uint8_t*)c->cs_keep.p;
  }
  const Rec* rec = (const Rec*)d_rec;
  uint32_t* skey = (uint32_t*)c->cs_key.p;
  int32_t* sidx = (int32_t*)c->cs_idx.p;
  int32_t* cur = (int32_t*)c->cs_cur.p;
  int32_t* start = (int32_t*)c->cs_start.p;
  int32_t* blk = (int32_t*)c->cs_blk.p;
  const long nb = ((long)cap + CS_THREADS - 1) / CS_THREADS;
  const dim3 sgrid((unsigned)(nb < 1024 ? nb : 1024), P), cgrid((unsigned)nchunk, P);
  for (int s = 0; s < prm->shifts; ++s) {
    const gpc::ConsGrid g = cons_grid(W, H, prm, s);
    HIPCHK(c, hipMemsetAsync(cur, 0, sizeof(int32_t) * (size_t)g.ncell * P, c->stream));
    {
      Timed t(c, KID_CONS_CELLS);
      hipLaunchKernelGGL((gpc::k_cons_cells<CORR>), sgrid, dim3(CS_THREADS), 0, c->stream, rec, cap, d_counts, g, cur, d_keep);
    }
    {
      Timed t(c, KID_CONS_SCAN);
      hipLaunchKernelGGL((gpc::k_cons_scan<true, true>), dim3(P), dim3(1024), 0, c->stream, cur, (long)g.ncell, g.ncell, start,
                         (long)g.ncell + 1, (int32_t*)nullptr);
    }
    {
      Timed t(c, KID_CONS_SCATTER);
      hipLaunchKernelGGL((gpc::k_cons_scatter<CORR>), sgrid, dim3(CS_THREADS), 0, c->stream, rec, cap, d_counts, g, cur, skey, sidx);
    }
    {
      Timed t(c, KID_CONS_COUNT);
      hipLaunchKernelGGL(gpc::k_cons_count, dim3((unsigned)g.ncell, P), dim3(CS_THREADS), 0, c->stream, cap, g,
                         (const int32_t*)start, (const uint32_t*)skey, (const int32_t*)sidx, d_keep);
    }
  }
  {
    Timed t(c, KID_CONS_BLOCKS);
    hipLaunchKernelGGL(gpc::k_cons_blocks, cgrid, dim3(CS_THREADS), 0, c->stream, cap, d_counts, (const uint8_t*)d_keep, blk, (int)nchunk);
  }
  {
    Timed t(c, KID_CONS_SCAN);
    hipLaunchKernelGGL((gpc::k_cons_scan<false, false>), dim3(P), dim3(1024), 0, c->stream, blk, nchunk, (int)nchunk, blk, nchunk,
                       d_out_counts);
  }
  {
    Timed t(c, KID_CONS_WRITE);
    hipLaunchKernelGGL((gpc::k_cons_write<CORR>), cgrid, dim3(CS_THREADS), 0, c->stream, rec, cap, d_counts, (const uint8_t*)d_keep,
                       (const int32_t*)blk, (int)nchunk, (Rec*)d_out, cap_out, d_index);
  }
  for (int k = KID_CONS_CELLS; k <= KID_CONS_WRITE; ++k) {
    const bool typed = k == KID_CONS_CELLS || k == KID_CONS_SCATTER || k == KID_CONS_WRITE;
    // (the scan's slot times both of its instantiations: <true, true> once per grid, <false, false> once for the compaction)
    snprintf(c->launch_name[k], sizeof c->launch_name[0], k == KID_CONS_SCAN ? "gpc::%s<true, true> + <false, false>" : (typed ? "gpc::%s<%s>" : "gpc::%s"),
             kKernelNames[k], CORR ? "true" : "false");
  }
  HIPCHK(c, hipGetLastError());
  return GPC_OK;
}

// match and filter, images as all_records takes them
int cons_match(gpc_hip_ctx* c, const uint8_t* d_a, const uint8_t* d_b, int W, int H, int npairs, const gpc_settings* s,
               const gpc_consensus* prm, void* d_out, int cap_out, int32_t* d_out_counts, int32_t* d_raw_counts,
               int32_t* d_ncand) {
  CHK(cons_params(prm));
  AllRecords r;
  CHK(all_records_cap(c, s, W, H, !d_b, &r.cap));
  CHK(cons_limits(r.cap, W, H, npairs, prm->cell));  // (before any workspace is made, too)
  CHK(all_records(c, d_a, d_b, W, H, npairs, s, d_ncand, &r));
  if (d_raw_counts)
    HIPCHK(c, hipMemcpyAsync(d_raw_counts, r.counts, sizeof(int32_t) * (size_t)npairs, hipMemcpyDeviceToDevice, c->stream));
  return d_b ? cons_filter<false>(c, r.rec, r.cap, r.counts, W, H, npairs, prm, nullptr, d_out, cap_out, nullptr, d_out_counts)
             : cons_filter<true>(c, r.rec, r.cap, r.counts, W, H, npairs, prm, nullptr, d_out, cap_out, nullptr, d_out_counts);
}

// Host forms (Stage): chunks of at most 16 pairs.
template <bool CORR>
int cons_host(gpc_hip_ctx* c, const void* rec, int cap, const int32_t* counts, int W, int H, int npairs,
              const gpc_consensus* prm, uint8_t* keep, void* out, int cap_out, int32_t* index, int32_t* out_counts) {
  const size_t esz = sizeof(gpc::ConsRec<CORR>);
  CHK(cons_args(c, rec, esz, cap, counts, W, H, npairs, prm, out, cap_out, out_counts));
  CHK(host_call_begin(c));
  const int K = npairs < 16 ? npairs : 16;
  Stage st(c);
  const size_t r_rec = st.in(esz * (size_t)cap * K), r_cnt = st.in(sizeof(int32_t) * (size_t)K), r_keep = st.out((size_t)cap * K);
  const size_t r_out = st.out(esz * (size_t)cap_out * K), r_idx = st.out(sizeof(int32_t) * (size_t)cap_out * K);
  const size_t r_n = st.out(sizeof(int32_t) * (size_t)K);
  CHK(st.alloc(sizeof(int32_t) * (size_t)K));
  int status = GPC_OK;
  for (int p0 = 0; p0 < npairs; p0 += K) {
    const int pc = npairs - p0 < K ? npairs - p0 : K;
    CHK(st.up(r_cnt, counts + p0, sizeof(int32_t) * (size_t)pc));
    CHK(st.up_records(r_rec, rec, esz, cap, counts, p0, pc));
    CHK(cons_filter<CORR>(c, st.p(r_rec), cap, (const int32_t*)st.p(r_cnt), W, H, pc, prm, keep ? st.p(r_keep) : nullptr, st.p(r_out),
                          cap_out, index ? (int32_t*)st.p(r_idx) : nullptr, (int32_t*)st.p(r_n)));
    CHK(st.down(c->h_cnt.p, r_n, sizeof(int32_t) * (size_t)pc));
    CHK(st.wait());
    for (int t = 0; t < pc; ++t) {  // a pair's keep bytes as far as its records go, its kept records and their indices as far as cap_out
      const size_t m = (size_t)valid_records(counts[p0 + t], cap), w = (size_t)valid_records(c->h_cnt.p[t], cap_out), q = (size_t)(p0 + t);
      if (c->h_cnt.p[t] > cap_out) status = GPC_E_CAPACITY;
      if (keep && m) CHK(st.down(keep + q * cap, r_keep + (size_t)t * cap, m));
      if (w) CHK(st.down((uint8_t*)out + esz * q * cap_out, r_out + esz * (size_t)t * cap_out, esz * w));
      if (w && index) CHK(st.down(index + q * cap_out, r_idx + sizeof(int32_t) * (size_t)t * cap_out, sizeof(int32_t) * w));
    }
    CHK(st.wait());
    memcpy(out_counts + p0, c->h_cnt.p, sizeof(int32_t) * (size_t)pc);
  }
  CHK(check_join_err(c));
  return status;
}

}  // namespace

extern "C" {

int gpc_hip_consensus_supports_device(gpc_hip_ctx* c, const gpc_support* d_rec, int cap_per_pair, const int32_t* d_counts, int W,
                                      int H, int npairs, const gpc_consensus* prm, uint8_t* d_keep, gpc_support* d_out, int cap_out,
                                      int32_t* d_index, int32_t* d_out_counts) {
  CHK(cons_args(c, d_rec, sizeof(gpc_support), cap_per_pair, d_counts, W, H, npairs, prm, d_out, cap_out, d_out_counts));
  HIPCHK(c, hipSetDevice(c->device));
  return cons_filter<false>(c, d_rec, cap_per_pair, d_counts, W, H, npairs, prm, d_keep, d_out, cap_out, d_index, d_out_counts);
}

int gpc_hip_consensus_correspondences_device(gpc_hip_ctx* c, const gpc_correspondence* d_rec, int cap_per_pair,
                                             const int32_t* d_counts, int W, int H, int npairs, const gpc_consensus* prm,
                                             uint8_t* d_keep, gpc_correspondence* d_out, int cap_out, int32_t* d_index,
                                             int32_t* d_out_counts) {
  CHK(cons_args(c, d_rec, sizeof(gpc_correspondence), cap_per_pair, d_counts, W, H, npairs, prm, d_out, cap_out, d_out_counts));
  HIPCHK(c, hipSetDevice(c->device));
  return cons_filter<true>(c, d_rec, cap_per_pair, d_counts, W, H, npairs, prm, d_keep, d_out, cap_out, d_index, d_out_counts);
}

int gpc_hip_consensus_batch_device(gpc_hip_ctx* c, const uint8_t* d_rawL, const uint8_t* d_rawR, int W, int H, int npairs,
                                   const gpc_settings* s, const gpc_consensus* prm, gpc_support* d_out, int cap_out,
                                   int32_t* d_out_counts, int32_t* d_raw_counts, int32_t* d_ncand) {
  if (!c || !d_rawL || !d_rawR || !d_out || !d_out_counts || npairs <= 0 || cap_out <= 0) return GPC_E_INVALID;
  return cons_match(c, d_rawL, d_rawR, W, H, npairs, s, prm, d_out, cap_out, d_out_counts, d_raw_counts, d_ncand);
}

int gpc_hip_consensus_sequence_device(gpc_hip_ctx* c, const uint8_t* d_frames, int W, int H, int nframes, const gpc_settings* s,
                                      const gpc_consensus* prm, gpc_correspondence* d_out, int cap_out, int32_t* d_out_counts,
                                      int32_t* d_raw_counts, int32_t* d_ncand) {
  if (!c || !d_frames || !d_out || !d_out_counts || nframes < 2 || cap_out <= 0) return GPC_E_INVALID;
  return cons_match(c, d_frames, nullptr, W, H, nframes - 1, s, prm, d_out, cap_out, d_out_counts, d_raw_counts, d_ncand);
}

int gpc_hip_consensus_supports(gpc_hip_ctx* c, const gpc_support* rec, int cap_per_pair, const int32_t* counts, int W, int H,
                               int npairs, const gpc_consensus* prm, uint8_t* keep, gpc_support* out, int cap_out, int32_t* index,
                               int32_t* out_counts) {
  return cons_host<false>(c, rec, cap_per_pair, counts, W, H, npairs, prm, keep, out, cap_out, index, out_counts);
}

int gpc_hip_consensus_correspondences(gpc_hip_ctx* c, const gpc_correspondence* rec, int cap_per_pair, const int32_t* counts, int W,
                                      int H, int npairs, const gpc_consensus* prm, uint8_t* keep, gpc_correspondence* out,
                                      int cap_out, int32_t* index, int32_t* out_counts) {
  return cons_host<true>(c, rec, cap_per_pair, counts, W, H, npairs, prm, keep, out, cap_out, index, out_counts);
}

}  // extern "C"
