// k_rowjoin_body.h -- the body of k_row_join (RJ_SEQ 0) and of k_row_join_seq (RJ_SEQ 1); k_rowjoin.h includes it twice.
// With RJ_SEQ 0 the text is k_row_join's as it stands, so its instantiations compile as before.  RJ_SEQ 1 reads the code
// images (and WIDE candidate bytes) of pair p at frames p and p + 1 of a sequence instead of images 2p and 2p + 1; the
// statistics stay in the pair layout (the host expands them: k_seq_stats).
// (no include guard: one inclusion per kernel)
#ifndef RJ_KEEP_RPW
  rpw = 1;  // (rows per workgroup with next-row prefetch measured within the noise of one row, docs/HISTORY.md 7, and its eight
            // prefetch registers put scratch into the 1024-thread instantiation: one row per workgroup it is)
#endif
  // flags of a table slot (one word per slot, x of a right record in the low half)
  constexpr uint32_t F_LSEEN = RJ_LSEEN, F_LDUP = RJ_LDUP, F_RSEEN = RJ_RSEEN, F_RDUP = RJ_RDUP, F_XMASK = 0xFFFFu;
  constexpr int NB = NT * SPT;
  extern __shared__ __attribute__((aligned(16))) uint32_t rj_lds[];
  __shared__ uint32_t s_max_key;
  __shared__ int s_tail_cnt;
  __shared__ unsigned s_tail_minx;
  __shared__ int s_sp_l, s_sp_r;   // WIDE: left / right candidates of this row whose code is 0xFFFFFFFF
  __shared__ unsigned s_sp_minx;   //       smallest x among the right ones
  __shared__ uint32_t s_w[NT / 64];
  __shared__ uint32_t s_cmin, s_cmax;      // smallest / largest matched code of the row: the rank buckets span that range
  __shared__ unsigned s_tail_xv, s_sp_xv;  // VIRT: position of the tail / key-less right record with the smallest pixel index
  const int S = 1 << log2s;
  uint32_t* t_key = rj_lds;               // [S]   stored key = code + 1, 0 = empty
  uint32_t* t_w = rj_lds + S + 1;         // [S]   per slot: seen / duplicate flags of either side, x of a right record in the low bits
  uint32_t* r_cnt = t_key;                // [NB+1] bucket counters -> starts   (reuses t_key, dead after step 2)
  uint32_t* r_key = t_w;                  // [NB]   matched codes, bucket-contiguous (reuses t_w, dead after step 3)
  // one returning OR on a slot's flag word; returns what the slot held
  auto mark = [&](uint32_t h, uint32_t val) -> uint32_t { return atomicOr(&t_w[h], val); };
  auto mark_noret = [&](uint32_t h, uint32_t val) { atomicOr(&t_w[h], val); };
  const uint32_t keys_lds = (uint32_t)(uintptr_t)t_key;  // low half of the flat address = LDS offset

  const int tid = threadIdx.x, lane = tid & 63;
  const int pair = (int)blockIdx.y;
  const int hshift = 32 - log2s;
  const uint32_t smask = (uint32_t)S - 1u;
  // VIRT: this workgroup's partition
  int32_t* vblk = nullptr;
  const uint2 *vrl = nullptr, *vrr = nullptr;  // the partition's records per side
  int v_nl = 0, v_nr = 0, v_offl = 0, v_p = 0;
  if (VIRT) {
    vblk = v.part + pair * v.ps;
    int p = blockIdx.x;
    if (v.use_list) {
      if (p >= vblk[v.o_misc + 3]) return;  // GP_NBIG
      p = vblk[v.o_misc + 8 + p];
    }
    v_p = p;
    if (p >= vblk[v.o_misc + 0]) return;  // GP_NPARTS
    v_offl = vblk[v.o_off + p];
    const int offr = vblk[v.o_off + v.pmax + 1 + p];
    v_nl = vblk[v.o_off + p + 1] - v_offl;
    v_nr = vblk[v.o_off + v.pmax + 1 + p + 1] - offr;
    if (v_nl > NB || v_nr > NB) return;  // another launch's partition (or k_gp_plan has raised the overflow flag: the host takes the radix path)
    if (max(v_nl, v_nr) <= v.min_recs) return;
    vrl = v.kv + pair * v.recs + v_offl;
    vrr = v.kv + pair * v.recs + v.recs / 2 + offr;
  }
  int last_r = 0;
  last_r = VIRT ? vblk[v.o_misc + 2] /* GP_LASTR */ : img_stats[(pair * 2 + 1) * GPC_STAT_STRIDE + GPC_STAT_LASTROW];
  // A workgroup handles `rpw` consecutive rows; the NEXT row's codes are fetched into registers
  // while the current row is joined, so only the first row's load latency is exposed.
  const int row0 = VIRT ? v_p : GPC_R + blockIdx.x * rpw;
  uint32_t ncl[SPT], ncr[SPT];
  uint32_t nspl = 0u, nspr = 0u;  // WIDE: bit j = pixel slot j is a candidate whose code is 0xFFFFFFFF
  auto fetch_row = [&](int yy) {
    nspl = nspr = 0u;
    if (VIRT) {
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int x = j * NT + tid;
        ncl[j] = (x < v_nl) ? vrl[x].x : RJ_EMPTY;
        ncr[j] = (x < v_nr) ? vrr[x].x : RJ_EMPTY;
        if (WIDE) {  // every record is a candidate: 0xFFFFFFFF is the key-less code
          if (x < v_nl && ncl[j] == RJ_EMPTY) nspl |= 1u << j;
          if (x < v_nr && ncr[j] == RJ_EMPTY) nspr |= 1u << j;
        }
      }
      return;
    }
#if RJ_SEQ
    const long ro = ((long)pair * H + yy) * W;  // frames [nframes][H][W]: pair p joins frames p and p + 1
#else
    const long ro = ((long)(pair * 2) * H + yy) * W;
#endif
    const uint32_t* rl = codes + ro;
    const uint32_t* rr_ = rl + (long)H * W;
    {
      // no branch around a load: with one the compiler sinks the key arithmetic into the branch and waits for every
      // pair of loads before it issues the next (four round trips per row instead of one)
      // (nor a clamp: pixel slots beyond W read into the next row -- the code image is allocated with that slack, the
      // host sees to it -- and are masked afterwards: one lane offset + an immediate per load)
      uint32_t tl[SPT], tr[SPT];
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
#ifdef RJ_DBG_NOLOAD     // (experiment, with RJ_DBG_EMPTY only: what the rows' loads cost)
        tl[j] = (uint32_t)(j * NT + tid) * 3u;
        tr[j] = (uint32_t)(j * NT + tid) * 5u;
#else
        tl[j] = rl[(uint32_t)(j * NT + tid)];
        tr[j] = rr_[(uint32_t)(j * NT + tid)];
#endif
      }
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        ncl[j] = (j * NT + tid < W) ? tl[j] : RJ_EMPTY;
        ncr[j] = (j * NT + tid < W) ? tr[j] : RJ_EMPTY;
      }
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int x = j * NT + tid;
      if (WIDE) {
        // the hash kernel's candidate rule (k_hash.h): candidate byte set, inside the margin (the row is)
        const bool inm = x >= GPC_R && x < W - GPC_R;
        if (inm && ncl[j] == RJ_EMPTY && cand[ro + x]) nspl |= 1u << j;
        if (inm && ncr[j] == RJ_EMPTY && cand[ro + (long)H * W + x]) nspr |= 1u << j;
      }
    }
  };
  fetch_row(row0);
#pragma unroll 1
  for (int ri = 0; ri < rpw && (VIRT ? ri == 0 : row0 + ri < H - GPC_R); ++ri) {
  const int y = row0 + ri;
  RJ_STAMP_INIT();
#ifdef RJ_DBG_PADVALU  // calibration: how much of a row's time is VALU issue?  RJ_DBG_PADVALU x 8 dependent-free adds per wave and row
  {
    uint32_t p0 = tid, p1 = tid + 1, p2 = tid + 2, p3 = tid + 3;
    for (int q = 0; q < RJ_DBG_PADVALU; ++q)
      asm volatile("v_add_u32 %0, %0, %1\n\tv_add_u32 %1, %1, %2\n\tv_add_u32 %2, %2, %3\n\tv_add_u32 %3, %3, %0\n\t"
                   "v_add_u32 %0, %0, %2\n\tv_add_u32 %1, %1, %3\n\tv_add_u32 %2, %2, %0\n\tv_add_u32 %3, %3, %1"
                   : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
    if ((p0 ^ p1 ^ p2 ^ p3) == 0x12345u && W < 0) rj_lds[0] = p0;  // (keeps the adds)
  }
#endif
#ifdef RJ_DBG_PADSALU
  {
    uint32_t q0 = (uint32_t)W, q1 = (uint32_t)H;
    for (int q = 0; q < RJ_DBG_PADSALU; ++q)
      asm volatile("s_add_u32 %0, %0, %1\n\ts_add_u32 %1, %1, %0\n\ts_add_u32 %0, %0, %1\n\ts_add_u32 %1, %1, %0\n\t"
                   "s_add_u32 %0, %0, %1\n\ts_add_u32 %1, %1, %0\n\ts_add_u32 %0, %0, %1\n\ts_add_u32 %1, %1, %0"
                   : "+s"(q0), "+s"(q1) : : "scc");
    if ((q0 ^ q1) == 0x12345u && W < 0) rj_lds[0] = q0;
  }
#endif
  // ---- 0. this row's codes (already in flight), table clear, next row's loads
  uint32_t kl[SPT], kr[SPT];  // (the code itself is kl - 1 wherever it is needed: one register per slot less)
  uint32_t spl = 0u, spr = 0u;
  {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {  // stored key = code + 1 (0 = no record in this pixel slot)
      kl[j] = ncl[j] + 1u;
      kr[j] = ncr[j] + 1u;
#ifdef RJ_DBG_EMPTY   // experiment: every pixel slot without a record -- what a row costs before it holds anything
      kl[j] = kr[j] = 0u * (ncl[j] + ncr[j]);
#endif
#ifdef RJ_DBG_LEFTONLY  // experiment: no right records (inserts and left lookups only)
      kr[j] = 0u * ncr[j];
#endif
    }
    if (WIDE) {
      spl = nspl;
      spr = nspr;
    }
    if (!VIRT && ri + 1 < rpw && y + 1 < H - GPC_R) fetch_row(y + 1);
    {  // 16-byte stores; the host rounds the allocation up to a multiple of 16 bytes
      uint4* z = reinterpret_cast<uint4*>(rj_lds);
      // the zeros are made HERE: as a plain constant the compiler keeps them in four registers across the whole row
      // and, at 64 VGPRs, spills them to scratch (one 16-byte store + load per thread and row)
      uint32_t z0;
      asm volatile("v_mov_b32 %0, 0" : "=v"(z0));
      const uint4 zero = make_uint4(z0, z0, z0, z0);
      const int nclear = (8 * (S + 1) + 15) / 16;
#ifndef RJ_DBG_NOCLEAR   // (experiment, with RJ_DBG_EMPTY only: what the table clear costs)
      for (int i = tid; i < nclear; i += NT) z[i] = zero;
#endif
    }
    if (tid == 0) {
      // (constants made here for the same reason as the zeros above: hoisted out of the row loop they are spilled to
      // scratch in the persistent instantiations, and the reload waits for every load in flight)
      uint32_t c0, c1;
      asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, -1" : "=v"(c0), "=v"(c1));
      s_cmin = c1;
      s_cmax = c0;
      s_max_key = c0;
      s_tail_cnt = (int)c0;
      s_tail_minx = c1;
      if (WIDE) {
        s_sp_l = (int)c0;
        s_sp_r = (int)c0;
        s_sp_minx = c1;
      }
    }
  }
  // Tail quirks of the reference's merge scan concern only the largest right
  // code of the last right row that has candidates: it matches iff it occurs exactly TWICE on
  // the right (then with the first of the two in mask order) and once on the left.
  const bool tail_row = (y == last_r);  // block-uniform
  __syncthreads();
  RJ_STAMP(0);

  // ---- 1. build the ordered table from the left codes (a slot without a record inserts key 0: a no-op)
  uint32_t h0l[SPT];
  {
    uint32_t old[SPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      // a pixel slot without a record inserts key 0 (a no-op) -- into a slot of its own: the atomics of
      // lanes that share an address are served one after the other
      h0l[j] = kl[j] ? rj_hash(kl[j], hshift) : ((uint32_t)(j * NT + tid) & smask);
      old[j] = atomicMax(&t_key[h0l[j]], kl[j]);
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) rj_insert_chain(keys_lds, kl[j], old[j], h0l[j], smask);
  }
  if (tail_row) {  // the largest right key of this row
    uint32_t max_k = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) max_k = max(max_k, kr[j]);
    for (int o = 32; o > 0; o >>= 1) max_k = max(max_k, (uint32_t)__shfl_xor((int)max_k, o));
    if (lane == 0 && max_k) atomicMax(&s_max_key, max_k);
  }
  if (WIDE) {  // the code without a key: count its records on either side
    if (__ballot(spl != 0u) | __ballot(spr != 0u)) {
      if (spl) atomicAdd(&s_sp_l, __popc(spl));
      if (spr) {
        atomicAdd(&s_sp_r, __popc(spr));
        if (VIRT) {  // positions carry no order here: the smallest PIXEL INDEX is the first in mask order
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if ((spr >> j) & 1u) atomicMin(&s_sp_minx, vrr[j * NT + tid].y);
        } else {
          atomicMin(&s_sp_minx, (unsigned)((__ffs((int)spr) - 1) * NT + tid));
        }
      }
    }
  }
  __syncthreads();
  RJ_STAMP(1);
  if (WIDE && VIRT && spr) {  // which position holds the key-less right record with the smallest pixel index (read after the next barrier)
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (((spr >> j) & 1u) && vrr[j * NT + tid].y == s_sp_minx) s_sp_xv = (unsigned)(j * NT + tid);
  }

  // ---- 2. every record finds its code's slot (read-only) and marks it.  The marks of a side go out
  //      together (one LDS round trip for SPT returning atomics): a record without a slot ORs 0 into
  //      wherever its walk stopped, which changes nothing.
  uint32_t hl[SPT];
  {
    uint32_t h0r[SPT], f0l[SPT], f0r[SPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {  // first probes of all records together
      h0r[j] = kr[j] ? rj_hash(kr[j], hshift) : ((uint32_t)(j * NT + tid) & smask);
      f0l[j] = t_key[h0l[j]];
      f0r[j] = t_key[h0r[j]];
    }
    uint32_t seen[SPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      uint32_t kk = kl[j] ? f0l[j] : 0u;
      hl[j] = rj_find_chain(keys_lds, kl[j], kk, h0l[j], smask);  // a left code is always found
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) seen[j] = mark(hl[j], kl[j] ? F_LSEEN : 0u);
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (kl[j] && (seen[j] & F_LSEEN)) mark_noret(hl[j], F_LDUP);  // a second left record of this code
    uint32_t hr[SPT], fr = 0u;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      uint32_t kk = kr[j] ? f0r[j] : 0u;
      hr[j] = rj_find_chain(keys_lds, kr[j], kk, h0r[j], smask);
      if (kr[j] && kk == kr[j]) fr |= 1u << j;
    }
    // x goes into the zeroed low half with the same atomic: several writers only when the code is
    // not unique on the right, and then x is not used
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      seen[j] = mark(hr[j], ((fr >> j) & 1u) ? (F_RSEEN | (uint32_t)(j * NT + tid)) : 0u);
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (((fr >> j) & 1u) && (seen[j] & F_RSEEN)) mark_noret(hr[j], F_RDUP);
  }
  // the key the tail rule applies to; none when the row's largest right code is the key-less 0xFFFFFFFF
  uint32_t tail_key = 0u;
  bool tail_sp = false;
  if (tail_row) {  // block-uniform
    tail_sp = WIDE && s_sp_r > 0;
    tail_key = tail_sp ? 0u : s_max_key;
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (kr[j] && kr[j] == tail_key) {
        atomicAdd(&s_tail_cnt, 1);
        atomicMin(&s_tail_minx, VIRT ? vrr[j * NT + tid].y : (unsigned)(j * NT + tid));
      }
    if (VIRT) {  // positions carry no order: find where the tail record with the smallest pixel index sits
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SPT; ++j)
        if (kr[j] && kr[j] == tail_key && vrr[j * NT + tid].y == s_tail_minx) s_tail_xv = (unsigned)(j * NT + tid);
    }
  }
  __syncthreads();
  RJ_STAMP(2);
  // ---- 3. decide every left candidate; the key table is dead already: it becomes the rank counters
  {  // NB + 1 counters: SPT consecutive ones per thread (16-byte stores where SPT is 4: one LDS instruction instead of five)
    uint32_t z0;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z0));
    if (SPT % 4 == 0) {
#pragma unroll
      for (int q = 0; q < SPT / 4; ++q) reinterpret_cast<uint4*>(r_cnt)[tid * (SPT / 4) + q] = make_uint4(z0, z0, z0, z0);
    } else {
#pragma unroll
      for (int q = 0; q < SPT; ++q) r_cnt[tid * SPT + q] = z0;
    }
    if (tid == 0) r_cnt[NB] = z0;
  }
  uint32_t okm = 0u;  // bit j = pixel slot j is a match
  uint32_t xr[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    xr[j] = 0u;
    bool good = false;
    if (kl[j]) {
      const uint32_t w = t_w[hl[j]];
      const bool tail = tail_row && kl[j] == tail_key;
      good = !(w & F_LDUP) && (tail ? (s_tail_cnt == 2) : ((w & (F_RSEEN | F_RDUP)) == F_RSEEN));
      xr[j] = tail ? (VIRT ? s_tail_xv : s_tail_minx) : (w & F_XMASK);
    } else if (WIDE && ((spl >> j) & 1u)) {
      good = (s_sp_l == 1) && (s_sp_r == (tail_sp ? 2 : 1));
      xr[j] = VIRT ? s_sp_xv : s_sp_minx;
    }
    if (good && apply_filter) {
      if (VIRT) {  // rectifiedMatch's filter on the two pixels (inference.hpp:384-391)
        const uint32_t pl = vrl[j * NT + tid].y, pr = vrr[xr[j]].y;
        const int yl = divw(pl, v.dw), yr = divw(pr, v.dw);
        good = abs(yl - yr) <= v.vtol && abs(((int)pl - yl * v.dw.W) - ((int)pr - yr * v.dw.W)) <= disp_high;
      } else {
        good = abs((int)(j * NT + tid) - (int)xr[j]) <= disp_high;
      }
    }
    if (good) okm |= 1u << j;
  }
  if (VIRT) {  // range of the partition's matched codes (one pair of LDS atomics per wave that has a match)
    uint32_t cmax = 0u, cmin = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if ((okm >> j) & 1u) {
        cmax = max(cmax, kl[j] - 1u);
        cmin = min(cmin, kl[j] - 1u);
      }
    if (__ballot(okm != 0u)) {  // wave-uniform
      cmax = wave_max_u32(cmax);
      cmin = ~wave_max_u32(~cmin);
      if (lane == 0) {
        atomicMax(&s_cmax, cmax);
        atomicMin(&s_cmin, cmin);
      }
    }
  }
  __syncthreads();  // the flag words are dead from here on: their LDS is reused
  RJ_STAMP(3);
  // ---- 4. output position = rank of the code among the row's matches (counting rank)
  // Measured on one box and NOT adopted (546 / 514 us per 256 pairs as it stands):
  //   * matches alone in their bucket written straight from the scan, only shared buckets walked: 553 us;
  //   * matches first appended to a dense list (a wave reserving its stretch with one atomic) and ranked from
  //     there, one match per thread, with 16-bit counters beside the table: 522 us.
  // The NB buckets divide the range the codes really span, so that bits the forest leaves constant cost no resolution:
  // rows: [0, 2^bits) with bits from the OR of every code k_hash computed for the left image (a scalar load; tests
  // that never hold leave their bit clear there); partitions (VIRT): [smallest, largest matched code] of this
  // partition, reduced above (all its codes share a prefix).  The reduction costs a row kernel 18 us per 256 pairs.
  uint32_t cbase = 0u;
  int csh = 0;
  {
    uint32_t span;
    if (VIRT) {
      cbase = s_cmin;
      span = s_cmax >= cbase ? s_cmax - cbase : 0u;
    } else {
      span = (uint32_t)img_stats[(pair * 2) * GPC_STAT_STRIDE + GPC_STAT_CODEOR];
    }
    int lnb = 0;
    while ((1 << lnb) < NB) ++lnb;
    csh = (span ? 32 - __builtin_clz(span) : 0) - lnb;  // bits of the span beyond the log2(NB) a bucket index has
    if (csh < 0) csh = 0;
  }
  uint32_t rb[SPT], rs[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    rb[j] = (kl[j] - 1u - cbase) >> csh;
    rs[j] = 0u;
    if ((okm >> j) & 1u) rs[j] = atomicAdd(&r_cnt[rb[j]], 1u);
  }
  __syncthreads();
  RJ_STAMP(4);
#ifndef RJ_OLD_RANK
  // How many matches share the bucket, read BEFORE the scan turns the counters into starts (every such read is done
  // before block_exscan's first barrier, the scan's stores come after it): four matches in five are alone in theirs and
  // need neither a place in r_key nor the two reads of neighbouring starts -- their rank is their bucket's start.
  // rs[j] becomes (arrival order | bucket count << 16): both are at most NB <= 4096... 16384 (VIRT) < 2^16.
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if ((okm >> j) & 1u) rs[j] |= r_cnt[rb[j]] << 16;
#endif
#ifndef RJ_DBG_NOSCAN    // (experiment, with RJ_DBG_EMPTY only)
  block_exscan<SPT, NT>(r_cnt, s_w, tid);  // r_cnt[b] = first rank of bucket b, r_cnt[NB] = number of matches
#endif
#ifdef RJ_OLD_RANK
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if ((okm >> j) & 1u) r_key[r_cnt[rb[j]] + rs[j]] = kl[j] - 1u;  // the code (WIDE: the key-less 0xFFFFFFFF ranks last)
#else
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if ((okm >> j) & 1u) {
      rb[j] = r_cnt[rb[j]];  // the bucket's first rank (the bucket index is not needed again)
      if ((rs[j] >> 16) > 1u) r_key[rb[j] + (rs[j] & 0xFFFFu)] = kl[j] - 1u;  // the code (WIDE: the key-less 0xFFFFFFFF ranks last)
    }
#endif
  __syncthreads();
  RJ_STAMP(5);
  const long rowbase = (long)pair * H + y;
  uint32_t* dst = (VIRT ? v.staged + pair * (v.recs / 2) + v_offl : staged + rowbase * W);
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if ((okm >> j) & 1u) {
      // (two plain ds_read_b32: for neighbouring words the compiler emits ds_read2_b32, which issues 3.6 times slower than
      // one ds_read_b32 on gfx950 -- profiles/r03_ubench2_issue_rates.txt -- and it unrolls the walk 16-fold with them)
#ifdef RJ_OLD_RANK
      uint32_t bidx = rb[j];
      const uint32_t s0 = r_cnt[bidx];
      asm volatile("" : "+v"(bidx));
      const uint32_t e0 = r_cnt[bidx + 1];
#else
      const uint32_t s0 = rb[j], e0 = s0 + (rs[j] >> 16);
#endif
      uint32_t rank = s0;
      const uint32_t cj = kl[j] - 1u;
#ifdef RJ_WALK_ALWAYS
      if (true) {
#else
      if (e0 - s0 > 1u) {  // a match alone in its bucket (four of five) has its rank already
#endif
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (uint32_t i = s0; i < e0; ++i) rank += (r_key[i] < cj);
      }
      if (VIRT) {
        // the two PIXEL INDICES, not the positions inside the partition: the partition's records were read by this
        // workgroup a moment ago (L2), where k_gp_gather fetched the same two words per match at random from memory
        // (83 -> 4x us per 8 pairs of 1920x1080 for that kernel)
        uint2* d2 = reinterpret_cast<uint2*>(v.staged) + pair * (v.recs / 2) + v_offl;
        d2[rank] = make_uint2(vrl[j * NT + tid].y, vrr[xr[j]].y);
      } else {
        dst[rank] = (uint32_t)(j * NT + tid) | (xr[j] << 16);
      }
    }
  if (tid == 0) {
    if (VIRT) vblk[v.o_rowcnt + y] = (int32_t)r_cnt[NB];
    else rowcnt[rowbase] = (int32_t)r_cnt[NB];
  }
#ifdef GPC_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  RJ_STAMP(6);
  RJ_STAMP_FLUSH();
  if (ri + 1 < rpw && y + 1 < H - GPC_R) __syncthreads();  // the table is cleared again for the next row
  }  // rows of this workgroup
