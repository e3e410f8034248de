// k_hash_body.h -- the body of k_hash (HT_GROUPS 0) and of k_hash_groups (HT_GROUPS 1); k_hash.h includes it twice.
// With HT_GROUPS 0 the text is k_hash's as it stands, so its instantiations compile as before.
// (no include guard: one inclusion per kernel)
  static_assert(TY % (HT_THREADS / 64) == 0, "a wave owns TY / 8 rows of the tile");
  constexpr int RPW = TY / (HT_THREADS / 64);
  constexpr int T_ROWS = TY + 2 * GPC_R, T_COPY = T_ROWS * HT_STRIDE;  // window rows; bytes of one (shifted) copy of the window
  __shared__ __attribute__((aligned(16))) uint8_t tile[4 * T_COPY];
  __shared__ int s_cnt, s_last, s_or;
#if HT_GROUPS
  __shared__ int s_gor[GPC_MAX_GROUPS];  // the OR of each group's codes
  const GpcForestDev* __restrict__ fp = fp_groups;
#endif

  // XCD-aware tile order: workgroups go round-robin to the 8 XCDs (each with its own L2) in launch
  // order, so launch-order neighbours never share an L2.  Remapped, XCD k works through its own
  // contiguous eighth of the (x, y, image) tile list: the tiles that share a window apron (left /
  // right, above / below) meet in one L2.
  unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
#ifndef HT_NO_XCD_REMAP
  {
    const unsigned nwg = gridDim.x * gridDim.y * gridDim.z;
    if ((nwg & 7u) == 0u) {
      const unsigned flat = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
      const unsigned logical = (flat & 7u) * (nwg >> 3) + (flat >> 3);
      bx = logical % gridDim.x;
      by = (logical / gridDim.x) % gridDim.y;
      bz = logical / (gridDim.x * gridDim.y);
    }
  }
#endif
  const int img = bz;
  const long n = (long)W * H;
  const uint8_t* sm = smooth + (long)img * n;
  static_assert(!GBITS || (!DENSE && !NAIVE), "the bit image exists in the batched SSE pipelines only");
  const uint8_t* gr = grad + (long)img * (GBITS ? n / 8 : n);
  // (the bit image's launches never bring a candidate map -- run_hash: gbits requires d_cand == nullptr)
  const uint8_t* cm = (!GBITS && candmap) ? candmap + (long)img * n : nullptr;
#if !HT_GROUPS
  uint32_t* out = codes + (long)img * n;
#endif
  const int tx0 = bx * HT_X;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int x0 = tx0 + 4 * lane;

  if (tid == 0) { s_cnt = 0; s_last = -1; s_or = 0; }
#if HT_GROUPS
  if (tid < GPC_MAX_GROUPS) s_gor[tid] = 0;  // (the tile loop's first barrier comes before any use)
#endif

  // bit 7 of byte j: pixel x0 + j lies inside the image and the 13-pixel margin (constant per lane)
  uint32_t xmask = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x0 + j >= GPC_R && x0 + j < W - GPC_R) xmask |= 0x80u << (8 * j);

  // A workgroup walks `tpw` vertically adjacent tiles.  The window of the NEXT tile is fetched
  // into registers (16-byte coalesced loads) before the current tile's tests run, so the global
  // latency hides behind ~7 us of VALU/LDS work; it is written to LDS (as 4 byte-shifted copies)
  // once the current tile is done.
  constexpr int QPR = HT_STRIDE / 16;                          // 16-byte chunks per window row
  constexpr int NCHUNK = T_ROWS * QPR;
  constexpr int CPT = (NCHUNK + HT_THREADS - 1) / HT_THREADS;  // chunks per thread
  // chunk -> (window row, chunk in row), byte offset inside a copy: the same for every tile
  int crow[CPT], cnxt[CPT], cdst[CPT];
  uint32_t cflag[CPT];  // bit 0: chunk exists, bit 1: it has a right neighbour inside the window
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + i * HT_THREADS;
    const int r = c / QPR, q = c - r * QPR;
    // offset of the chunk from the window's first row; a chunk this thread does not have lies 2^30 bytes out: beyond any image
    crow[i] = c < NCHUNK ? r * W + q * 16 - HT_APRON + tx0 : HT_FAR;
    cnxt[i] = (c < NCHUNK && q + 1 < QPR) ? crow[i] + 16 : HT_FAR;  // the dword behind the chunk -- the row's last chunk has none inside the window
    cdst[i] = r * HT_STRIDE + q * 16;
    cflag[i] = (c < NCHUNK ? 1u : 0u) | (q + 1 < QPR ? 2u : 0u);
  }
  uint4 pv[CPT];
  uint32_t pn[CPT];
  uint32_t pg[RPW];  // gradient bytes of this thread's 4 pixels in its RPW rows of the fetched tile
  // The image's bytes and its gradient image as BUFFER resources (base, size, no stride): a buffer load outside [0, size)
  // returns 0 by itself -- the reference's "bytes outside the image read as 0" (its unaligned loads reach above row 0 and
  // below row H - 1) is the hardware's range check.  Chunks are 16-byte aligned and so is the size: none straddles the end.
  // (As flat loads behind compares the fetch of a tile was ~150 instructions of EXEC regions and zero moves; it is 25.)
  const uint32_t nbytes = (uint32_t)n;  // an image has at most 2^30 pixels (check_dims): 32-bit offsets
  const __amdgpu_buffer_rsrc_t rs_sm = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(sm), 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_gr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(gr), 0, (int)(GBITS ? nbytes / 8u : nbytes), 0x00020000);
  // a lane beyond the image's width asks for a gradient word 2^30 bytes out
  const uint32_t gcol = x0 < W ? (GBITS ? (uint32_t)(x0 & ~15) >> 3 : (uint32_t)x0) : (uint32_t)HT_FAR;
  auto fetch = [&](int ty0) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int y = ty0 + wave * RPW + r;  // (a row below the image: beyond the gradient image's size)
      if (GBITS)  // the group's 16 bits (2-byte aligned: W is a multiple of 16)
        pg[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs_gr, ((uint32_t)(y * W) >> 3) + gcol, 0, 0);
      else
        pg[r] = __builtin_amdgcn_raw_buffer_load_b32(rs_gr, (uint32_t)(y * W) + gcol, 0, 0);
    }
    const int base = (ty0 - GPC_R) * W;  // linear addressing like the reference's unaligned loads
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const uint32_t k = (uint32_t)(base + crow[i]);  // (negative above the image's first byte: wraps beyond its size)
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_sm, k, 0, 0);
      // (nothing here may touch what the loads return: the wait for them belongs in front of the staging, a tile later)
      pn[i] = __builtin_amdgcn_raw_buffer_load_b32(rs_sm, (uint32_t)(base + cnxt[i]), 0, 0);
      pv[i] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  auto stage = [&]() {  // copy s holds the window shifted left by s bytes (v_alignbyte of neighbouring dwords)
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      if (cflag[i] & 1u) {
        uint8_t* dst = tile + cdst[i];
        const uint4 v = pv[i];
        *reinterpret_cast<uint4*>(dst) = v;
#pragma unroll
        for (int sft = 1; sft < 4; ++sft) {
          uint4 w;
          w.x = __builtin_amdgcn_alignbyte(v.y, v.x, sft);
          w.y = __builtin_amdgcn_alignbyte(v.z, v.y, sft);
          w.z = __builtin_amdgcn_alignbyte(v.w, v.z, sft);
          w.w = __builtin_amdgcn_alignbyte(pn[i], v.w, sft);
          *reinterpret_cast<uint4*>(dst + sft * T_COPY) = w;
        }
      }
    }
  };

  constexpr bool INV = !DENSE && !NAIVE;
  constexpr int CBIT = GBITS ? 0 : 7;   // where cand8 keeps a pixel's candidate flag inside its byte
  const int tile0 = by * tpw;
  const int ntiles = (H - 2 * GPC_R + TY - 1) / TY;
  // workgroups are dispatched in the order of their flat index: those from `last_round_from` on are the last the places take
  const bool last_round = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) >= last_round_from;
  HT_STAMP_INIT();
  fetch(GPC_R + tile0 * TY);
  int cnt = 0, last = -1;
  uint32_t cor = 0u;  // OR of the codes computed here (candidates or not: a superset costs the join nothing)
  uint32_t cor3 = 0u; // INV: OR of the last plane's complemented bytes (the codes' bits 24 .. 30), folded into cor at the end
  const int T = fp->num_tests;
  const bool m128 = TAU && !NAIVE && fp->tau_m128 != 0;  // the forest holds a tau of -128 (wave-uniform, read once)
  int lanebase = (wave * RPW + GPC_R) * HT_STRIDE + 4 * lane + HT_APRON;
  // keep the constant part (13 rows + apron = 3760 bytes) inside the register: left to the compiler it
  // becomes an immediate that no longer fits the 8-bit dword offsets of ds_read2_b32, and every pair of
  // row reads then needs its own address add (6 adds per test instead of 2)
  asm volatile("" : "+v"(lanebase));
  const int n3 = max(1, min(T, 32) - 25);                     // tests that went into the last plane (T <= 25: plane empty, ~p3 = 0)
  const uint32_t m3 = 0x01010101u * ((1u << n3) - 1u);       // n3 = 7: 0x7F7F7F7F
  // test 8 is OR-ed into bit 0 unless x % 8 == 0 (64-bit-lane carry of bitMask += bitMask)
  const uint32_t m8 = (x0 & 4) ? 0x01010101u : 0x01010100u;
#pragma unroll 1
  for (int tt = 0; tt < tpw && tile0 + tt < ntiles; ++tt) {
  const int ty0 = GPC_R + (tile0 + tt) * TY;
#ifndef HT_NO_SETPRIO
  // Wave priorities (s_setprio, 0 .. 3; a CU's arbiter serves the higher one first, then the older wave).
  //  * Inside a tile the priority steps down with the test groups (3 until test 8, then 2, 1, and 0 from test 25 through the
  //    stores): a wave that is behind its workgroup is served before one that is ahead, and the eight waves reach the tile's
  //    barrier together (they waited there for 24 % of the kernel): 318-321 -> 310-315 us per 256 pairs (two levels, 3 then
  //    0: 315-317; the steps ascending: 321-327).
  //  * The two workgroups of a CU share its issue slots oldest wave first: the older one runs ahead, ends early, and the
  //    younger works its last tiles alone at half the CU's occupancy (a 32-pair launch: a CU's 13 tiles in 50 us where 41
  //    would do, tools/exp/hash_wg_lives.py).  In the launch's LAST round of workgroups the steps are capped by the tiles a
  //    workgroup has left -- 6 and more: 3, 4-5: 2, 2-3: 1, the last: 0 -- so whoever is behind is served first and both
  //    reach their last tile together: k_hash 51.5 -> 49.0 us at 32 pairs, 89.6 -> 83.5 at 64, 324.5 -> 318.7 at 256
  //    (caps 3 / 2 / 1 over the last three tiles, by quarters of the workgroup's tiles, 8 / 5 / 3: 0-3 us behind, and
  //    within 1 % of each other over the BASELINE configurations, tools/exp/ab_configs.sh; a cap in every round, where a
  //    place is refilled when a workgroup ends, cost 324 -> 328 us per 256 pairs).
  int prio_cap = 3;
  if (last_round) {
    const int left = min(tpw - tt, ntiles - tile0 - tt);
    prio_cap = left >= 6 ? 3 : left >= 4 ? 2 : left >= 2 ? 1 : 0;
  }
  ht_set_prio(prio_cap);
#endif
  if (tt) __syncthreads();  // every wave has finished reading the previous window
  HT_STAMP(0);   // wait for the other waves' tests
  stage();
  uint32_t gq[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) gq[r] = pg[r];
  __syncthreads();
  HT_STAMP(1);   // window arrives (vmcnt), shifted copies written, barrier
  if (tt + 1 < tpw && tile0 + tt + 1 < ntiles) fetch(ty0 + TY);
  HT_STAMP(2);   // next window's loads issued

  const int yw = ty0 + wave * RPW;  // first row of this wave (>= 13)

  // ---- per row: candidate flags (bit 7 of byte j = pixel x0+j), group-of-16 activity
  uint32_t cand8[RPW];
  bool rowdo[RPW];
  bool any = false;
  if (GBITS) {
    // straight-line for the bit image: the fetched word is 0 for a row below the image and for a lane beyond its width
    // (buffer loads), so what is left of the row conditions is "above the last 13 rows" for the candidates and "above
    // the last 15" for the rows that are hashed -- two compares per row, no EXEC region
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int y = yw + r;
      const uint32_t g4 = gq[r];
      // own nibble -> BIT 0 of byte j (CBIT): nib * 0x204081 puts bit k of the nibble at 7j + k for j = 0 .. 3, i.e. bit j at
      // bit 0 of byte j (the other products fall on bits 1 .. 3 and are masked with the margin mask) -- a 24-bit multiply at
      // full rate where nib * 0x10204080 (bit 7 of byte j) was a v_mul_lo_u32 at a quarter of it
      const uint32_t nib = __builtin_amdgcn_ubfe(g4, (uint32_t)(x0 & 15), 4u);
      const uint32_t cb = __umul24(nib, 0x204081u) & (xmask >> 7) & (y < H - GPC_R ? ~0u : 0u);
      cand8[r] = cb;
      rowdo[r] = (y < H - 15) & (g4 != 0u);  // gpcFilterSegment(13, height-15) :602; groups without a gradient byte are skipped :566
      any = any | ((cb != 0u) & rowdo[r]);
    }
  } else
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int y = yw + r;
    const uint32_t g4 = gq[r];  // 0 outside the image
    uint32_t c4 = g4;
    if (cm) c4 = (x0 < W && y < H) ? *reinterpret_cast<const uint32_t*>(cm + (uint32_t)(y * W + x0)) : 0u;
    uint32_t cb;
    if (GBITS && !cm) {  // own nibble -> bit 7 of byte j (n * 0x10204080: bit j lands on 7, 15, 23, 31; the other products fall elsewhere)
      const uint32_t nib = (g4 >> (x0 & 15)) & 0xFu;
      cb = (y < H - GPC_R) ? ((nib * 0x10204080u) & SW_H & xmask) : 0u;
    } else {
      cb = (y < H - GPC_R) ? (swar_nonzero(c4) & xmask) : 0u;
    }
    // the reference skips 16-pixel groups (4 lanes here) without any gradient byte (filter.hpp:566):
    // OR over the quad of lanes with two DPP quad permutes (GBITS: the fetched word is the group's)
    uint32_t gany = g4;
    if (!NAIVE && !GBITS) {
      gany |= (uint32_t)__builtin_amdgcn_mov_dpp((int)gany, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
      gany |= (uint32_t)__builtin_amdgcn_mov_dpp((int)gany, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    }
    const bool rows_ok = y < (NAIVE ? H - GPC_R : H - 15);  // gpcFilterSegment(13, height-15) :602
    cand8[r] = cb;
    rowdo[r] = (x0 < W) && rows_ok && (NAIVE || gany != 0u);
    any = any || ((DENSE && !NAIVE) ? rowdo[r] : (cb != 0u && rowdo[r]));
  }

#if HT_GROUPS
  // every group on the staged window and the flags above: its tests, transposes and code plane, then its OR of the codes
#pragma unroll 1
  for (int g = 0; g < ngroups; ++g) {
  const GpcForestDev* __restrict__ fp = fp_groups + g;
  const int T = fp->num_tests;
  const bool m128 = TAU && !NAIVE && fp->tau_m128 != 0;
  const int n3 = max(1, min(T, 32) - 25);
  const uint32_t m3 = 0x01010101u * ((1u << n3) - 1u);
  uint32_t* out = codes + (long)((img >> 1) * 2 * ngroups + (img & 1) + g * gstep) * n;
  uint32_t cor = 0u, cor3 = 0u;
#ifndef HT_NO_SETPRIO
  if (g) ht_set_prio(prio_cap);
#endif
#endif
  // ---- the tests, in the reference's byte planes: P0 = tests 0..7, (test 8), P1 = 9..16,
  //      P2 = 17..24, P3 = 25..31.  Tests >= T are padded with equal taps (compare false).
  // The planes hold NOT(code bit).  The batched SSE instantiations (INV) keep the codes complemented through the transposes
  // and take the complement inside the store phase's v_bitop3 (a truth table costs nothing): four v_not per row less.
  uint32_t code[RPW][4];   // INV: the complemented codes
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) code[r][j] = INV ? ~0u : 0u;
  HT_STAMP(3);   // candidate flags, group activity

#ifdef HT_EXP_NOCOMPUTE
  if (W < 0) {
#else
  if (__ballot(any)) {  // wave-uniform: skip segments with nothing to hash
#endif
    uint32_t p0[RPW], p1[RPW], p2[RPW], p3[RPW], p8[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) p0[r] = p1[r] = p2[r] = p3[r] = p8[r] = ~0u;  // "ge" planes: all-ones = no bit
    if (NAIVE) {
      // slot u -> bit u: four full byte planes, no special test 8 (slots >= T are padded with equal taps)
      if (T > 0) fern_group<TAU, true, RPW, 8>(tile, lanebase, fp, 0, 8, p0);
      HT_PRIO_STEP(2);
      if (T > 8) fern_group<TAU, true, RPW, 8>(tile, lanebase, fp, 8, 8, p1);
      HT_PRIO_STEP(1);
      if (T > 16) fern_group<TAU, true, RPW, 8>(tile, lanebase, fp, 16, 8, p2);
      HT_PRIO_STEP(0);
      if (T > 24) fern_group<TAU, true, RPW, 8>(tile, lanebase, fp, 24, 8, p3);
    } else if (TAU && m128) {
      // (a forest with a tau of -128: the complemented subtract that holds for every tau, two operations more per test and row)
      if (T > 0) fern_group<TAU, false, RPW, 8, true>(tile, lanebase, fp, 0, 8, p0);
      if (T > 8) fern_group<TAU, false, RPW, 1, true>(tile, lanebase, fp, 8, 1, p8);
      HT_PRIO_STEP(2);
      if (T > 9) fern_group<TAU, false, RPW, 8, true>(tile, lanebase, fp, 9, 8, p1);
      HT_PRIO_STEP(1);
      if (T > 17) fern_group<TAU, false, RPW, 8, true>(tile, lanebase, fp, 17, 8, p2);
      HT_PRIO_STEP(0);
      if (T > 25) fern_group<TAU, false, RPW, 7, true>(tile, lanebase, fp, 25, min(T, 32) - 25, p3);
    } else {
      if (T > 0) fern_group<TAU, false, RPW, 8, false>(tile, lanebase, fp, 0, 8, p0);
      if (T > 8) fern_group<TAU, false, RPW, 1, false>(tile, lanebase, fp, 8, 1, p8);
      HT_PRIO_STEP(2);
      if (T > 9) fern_group<TAU, false, RPW, 8, false>(tile, lanebase, fp, 9, 8, p1);
      HT_PRIO_STEP(1);
      if (T > 17) fern_group<TAU, false, RPW, 8, false>(tile, lanebase, fp, 17, 8, p2);
      HT_PRIO_STEP(0);
      // the last plane holds tests 25 .. min(T, 32) - 1: no padded tests here (T = 30: 5, not 7)
      if (T > 25) fern_group<TAU, false, RPW, 7, false>(tile, lanebase, fp, 25, min(T, 32) - 25, p3);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      // planes hold "b >= a"; the code bit is its complement.  P3 saw 7 tests: one more shift.
      // (INV: the same with every term complemented -- ~(~p0 | ((~p8 >> 7) & m8)) = p0 & ((p8 >> 7) | ~m8) on the bits m8
      //  selects, ~((~p3 >> s) & m3) = (p3 >> s) | ~m3 on the bits m3 selects: neither shift crosses into a selected bit)
      const uint32_t q0 = INV ? (p0[r] & ((p8[r] >> 7) | ~m8)) : (NAIVE ? ~p0[r] : (~p0[r] | ((~p8[r] >> 7) & m8)));
      const uint32_t q1 = INV ? p1[r] : ~p1[r];
      const uint32_t q2 = INV ? p2[r] : ~p2[r];
      // P3 saw n3 tests (first one now n3 - 1 places below bit 7): bring the first down to bit 0
      const uint32_t q3 = INV ? ((p3[r] >> (8 - n3)) | ~m3) : (NAIVE ? ~p3[r] : ((~p3[r] >> (8 - n3)) & m3));
      // INV: the joins want the highest bit any code of the image has set (GPC_STAT_CODEOR: its leading zeros size their rank
      // buckets).  Bits 24 .. 30 of a code are its pixel's byte of the last plane, so the OR of that plane's bytes over the
      // rows that are hashed says which of them occur; below bit 24 the statistic is "every bit the forest can set" (a
      // superset is all the joins need).  One operation per row: cor3 | (~q3 & do).
      if (INV) cor3 = __builtin_amdgcn_bitop3_b32(q3, rowdo[r] ? ~0u : 0u, cor3, 0xAE);
      // transpose 4 planes x 4 pixels -> 4 codes (byte k of code j = plane k, byte j)
      const uint32_t lo01 = __builtin_amdgcn_perm(q1, q0, 0x05010400u);
      const uint32_t hi01 = __builtin_amdgcn_perm(q1, q0, 0x07030602u);
      const uint32_t lo23 = __builtin_amdgcn_perm(q3, q2, 0x05010400u);
      const uint32_t hi23 = __builtin_amdgcn_perm(q3, q2, 0x07030602u);
      code[r][0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
      code[r][1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
      code[r][2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
      code[r][3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    }
  }

  HT_STAMP(4);   // tests + plane transposes
  // ---- store (16 bytes per lane and row, 1 KiB per wave and row) + statistics
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int y = yw + r;
    if ((x0 < W) && (y < H)) {
      uint4 o;
      uint32_t* op = reinterpret_cast<uint32_t*>(&o);
      if (DENSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t c = rowdo[r] ? code[r][j] : 0u;
          cor |= c;
          const bool is_cand = (cand8[r] >> (8 * j + 7)) & 1u;
          op[j] = (NAIVE && !is_cand) ? 0u : c;
        }
      } else {
        // a candidate gets its code (0 where the row's 16-pixel group was skipped), anything else GPC_NOCAND (all ones):
        // (code & do & cand) | ~cand with the candidate bit spread over the word by a signed bit-field extract -- one
        // v_bfe_i32 + one v_bitop3 per pixel (select by select it was two v_cndmask, an and and a compare)
        const uint32_t dom = rowdo[r] ? ~0u : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t cm4 = (uint32_t)__builtin_amdgcn_sbfe((int)cand8[r], 8 * j + CBIT, 1);  // all ones for a candidate
          if (INV) {
            // (the OR of the codes is kept on the planes: cor3 below -- one operation per row instead of one per pixel)
            op[j] = __builtin_amdgcn_bitop3_b32(code[r][j], dom, cm4, 0x5D);  // cand ? (~ncode & do) : all ones
          } else {
            cor |= code[r][j] & dom;
            op[j] = __builtin_amdgcn_bitop3_b32(code[r][j], dom, cm4, 0xD5);  // cand ? (code & do) : all ones
          }
        }
      }
#if defined(HT_EXP_NOSTORE)   // experiment: how much of the kernel is the code image's write stream?
      if (o.x == 0x12345678u && W < 0) *reinterpret_cast<uint4*>(out + (uint32_t)(y * W + x0)) = o;
#elif defined(HT_EXP_HALFSTORE)
      if ((lane & 1) == 0) *reinterpret_cast<uint4*>(out + (uint32_t)(y * W + x0)) = o;
#else
      *reinterpret_cast<uint4*>(out + (uint32_t)(y * W + x0)) = o;
#endif
    }
#if HT_GROUPS
    if (g == 0 && cand8[r]) { cnt += __popc(cand8[r]); last = y; }
#else
    if (cand8[r]) { cnt += __popc(cand8[r]); last = y; }
#endif
  }
#if HT_GROUPS
  if (!DENSE) {  // this group's OR over the tile, into the workgroup's word of the group
    uint32_t t = INV ? ht_inv_cor(cor3, m3, T) : cor;
    for (int o = 32; o > 0; o >>= 1) t |= (uint32_t)__shfl_xor((int)t, o);
    if (lane == 0 && t) atomicOr(&s_gor[g], (int)t);
  }
  }  // groups
#endif
  HT_STAMP(5);   // code stores issued
  }  // tiles of this workgroup
  HT_STAMP_FLUSH();
#if !HT_GROUPS
  if (INV) {
    // bits 24 .. 30 from the last plane's bytes (only the n3 bits m3 selects are code bits); every lower bit the forest
    // has: tests 0 .. 7 -> bits 0 .. 7, test 8 -> bit 0, tests 9 .. 24 -> bits 8 .. 23
    uint32_t t = cor3 & m3;
    t |= t >> 16;
    t |= t >> 8;
    const int lowbits = T <= 8 ? T : (T - 1 < 24 ? T - 1 : 24);
    cor = ((t & 0x7Fu) << 24) | ((1u << lowbits) - 1u);
  }
#endif
  if (!DENSE) {
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o);
      last = max(last, __shfl_xor(last, o));
      cor |= (uint32_t)__shfl_xor((int)cor, o);
    }
    if (lane == 0 && cnt) { atomicAdd(&s_cnt, cnt); atomicMax(&s_last, last); atomicOr(&s_or, (int)cor); }
    __syncthreads();
#if HT_GROUPS
    if (tid < ngroups && s_cnt) {  // every virtual image of the image: the same candidates, its group's codes
      const int v = (img >> 1) * 2 * ngroups + (img & 1) + tid * gstep;
      atomicAdd(&img_stats[v * GPC_STAT_STRIDE + GPC_STAT_NCAND], s_cnt);
      atomicMax(&img_stats[v * GPC_STAT_STRIDE + GPC_STAT_LASTROW], s_last);
      atomicOr(&img_stats[v * GPC_STAT_STRIDE + GPC_STAT_CODEOR], s_gor[tid]);
    }
#else
    if (tid == 0 && s_cnt) {
      atomicAdd(&img_stats[img * GPC_STAT_STRIDE + GPC_STAT_NCAND], s_cnt);
      atomicMax(&img_stats[img * GPC_STAT_STRIDE + GPC_STAT_LASTROW], s_last);
      atomicOr(&img_stats[img * GPC_STAT_STRIDE + GPC_STAT_CODEOR], s_or);
    }
#endif
  }
