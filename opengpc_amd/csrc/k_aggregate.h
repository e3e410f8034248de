// k_aggregate.h -- the scanline aggregation of the search's costs (gpc_hip_aggregate_*).  include/gpc_hip.h has the rule in
// full; it is made of integers only.  Three stages, each a launch per group of pairs (two for the paths, one per orientation):
//   k_agg_cost<C, R, G>    k_search's cost evaluation -- the same tile of 32 x 8 pixels, the staged left tile, the one-check
//                          fast path through sr_load_row / sr_row (v_qsad_pk_u16_u8) and the clamped byte-wise path -- but
//                          instead of choosing it writes the costs: vol[pair][cell][y][x] uint16, cell = (dy+G+1)(2G+3) +
//                          (dx+G+1) over the shifts -(G+1) .. G+1 (C = 1: one row of 2G+3).  The inner cells are the labels;
//                          an inadmissible one holds AG_NONE, and so do all of a hole.  The ring around them keeps the raw
//                          costs the parabola needs (its corners are never read and never written).  Label-major, so that
//                          both path orientations and the choice read along x.
//   k_agg_path_v<C, G>     one lane per column, the K <= 25 running values of the chain in registers, rows read and written
//                          coalesced; the next row's costs are loaded before this row's step.  grid.y = the vertical
//                          directions in `paths`.
//   k_agg_path_h<C, G>     one lane per row.  A chunk of TX columns of 64 rows goes through LDS both ways: the wave loads
//                          it along x, every lane walks its own row in it (the pitch is an odd number of dwords: no bank
//                          conflicts), writes L over the costs, and the wave stores it along x.
//   Both run ag_step: the shift form.  The predecessor's values go through a 3 x 3 minimum in ITS label frame, extended by
//   one (F[j] = min(L[j], p1 + min of the 3 x 3 around j)), all indices constants; F goes to a lane-private LDS slot, and the
//   pixel gathers F[k + d], d the difference of the two bases: the only dynamic index of the step is an LDS address.
//   k_agg_choose<C, G>     one lane per pixel: S = the sum of the path values (or the cost, without paths), the search's
//                          tie-break chain over S, the parabola from the ring, stats by ballot as in k_search.
#pragma once
#include "aggregate_host.h"
#include "gpc_device.h"
#include "k_search.h"  // sr_whole, sr_clamp, sr_load_row, sr_row, the tile

#define AG_INF 0x3FFFFFFFu

namespace gpc {

template <int C, int G>
struct AgGeom {
  static constexpr int N1 = 2 * G + 1, NE = 2 * G + 3, NEY = C == 2 ? NE : 1;
  static constexpr int K = C == 2 ? N1 * N1 : N1, CELLS = C == 2 ? NE * NE : NE;
  static constexpr int TX = K > 9 ? 8 : K > 5 ? 16 : 32;  // ag_chunk
  static constexpr int PITCH = TX + 2;                     // halfwords a staged row of a label takes: an odd number of dwords
  static constexpr int RPITCH = TX + 1;                    // dwords a staged row of bases takes
  // label k = (ky + G) N1 + kx + G -> its cell
  static constexpr int cell(int k) { return C == 2 ? (k / N1 + 1) * NE + k % N1 + 1 : k + 1; }
  static constexpr bool corner(int c) { return C == 2 && (c / NE == 0 || c / NE == NE - 1) && (c % NE == 0 || c % NE == NE - 1); }
};

// grid (tiles x, tiles y, pairs of the group); field, imgL, imgR and vol are the group's.  n = W * H.
template <int C, int R, int G>
__global__ __launch_bounds__(SR_THREADS) void k_agg_cost(const int32_t* __restrict__ field, const uint8_t* __restrict__ imgL,
                                                         const uint8_t* __restrict__ imgR, int W, int H, uint16_t* __restrict__ vol) {
  static_assert((C == 1 || C == 2) && R >= 1 && R <= SR_MAX_RADIUS && G >= 0 && G <= SR_MAX_RANGE, "a target row with its shifts fits one 16-byte load");
  using Ge = AgGeom<C, G>;
  constexpr int NL = 2 * R + 1, NS = 2 * G + 3, NT = NL + NS - 1, ND = C == 2 ? NS : 1;
  constexpr int NLW = (NL + 3) / 4, NLD = (NL + 3 + 3) / 4;
  constexpr int TWA = SR_TILE_W + 2 * R, THA = SR_TILE_H + 2 * R;
  __shared__ uint32_t s_tile[SR_ROWS * SR_PITCH / 4];
  const int tid = threadIdx.x, lx = tid & (SR_TILE_W - 1), ly = tid / SR_TILE_W;
  const int p = blockIdx.z, x0 = blockIdx.x * SR_TILE_W, y0 = blockIdx.y * SR_TILE_H;
  const uint32_t n = (uint32_t)W * (uint32_t)H;
  const uint8_t* pl = imgL + (size_t)p * n;
  const uint8_t* pr = imgR + (size_t)p * n;
  uint8_t* tb = (uint8_t*)s_tile;
  for (int i = tid; i < TWA * THA; i += SR_THREADS) {
    const int row = i / TWA, col = i - row * TWA;
    tb[row * SR_PITCH + col] = pl[(size_t)sr_clamp(y0 - R + row, H - 1) * W + sr_clamp(x0 - R + col, W - 1)];
  }
  __syncthreads();

  const int x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  const size_t at = (size_t)p * C * n + (size_t)y * W + x;
  const int32_t f0 = field[at], f1 = C == 2 ? field[at + n] : 0;
  uint16_t* v = vol + (size_t)p * Ge::CELLS * n + (size_t)y * W + x;  // cell c is v[c * n]
  if (f0 == SR_NONE) {
#pragma unroll
    for (int c = 0; c < Ge::CELLS; ++c)
      if (!Ge::corner(c)) v[(size_t)c * n] = (uint16_t)AG_NONE;
    return;
  }
  const int r0 = sr_whole(f0), r1 = C == 2 ? sr_whole(f1) : 0;
  const int bx = C == 1 ? x - r0 : x + r0, by = y + r1;
  uint32_t cst[ND][4];  // the cost at y shift d - (G + 1) and x shift s - (G + 1): half s & 1 of cst[d][s >> 1]
#pragma unroll
  for (int d = 0; d < ND; ++d) cst[d][0] = cst[d][1] = cst[d][2] = cst[d][3] = 0u;
  // (k_search's check, its last condition included: the 16 bytes of the last row's load end inside the image)
  const bool fast = bx - R - (G + 1) >= 0 && bx + R + (G + 1) <= W - 1 &&
                    (C == 2 ? by - R - (G + 1) >= 0 && by + R + (G + 1) <= H - 1 : y - R >= 0 && y + R <= H - 1) &&
                    (uint32_t)(C == 2 ? by + R + (G + 1) : y + R) * (uint32_t)W + (uint32_t)(bx - R - (G + 1)) + 16u <= n;
  if (fast) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pr), 0, (int)n, 0x00020000);
    uint32_t l[NL][3];
    const uint32_t sh = (uint32_t)lx & 3u;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int base = ((ly + j) * SR_PITCH + (lx & ~3)) >> 2;
      uint32_t dw[NLD + 1];
#pragma unroll
      for (int k = 0; k < NLD; ++k) dw[k] = s_tile[base + k];
      dw[NLD] = 0u;
      l[j][0] = l[j][1] = l[j][2] = 0u;
#pragma unroll
      for (int k = 0; k < NLW; ++k) l[j][k] = __builtin_amdgcn_alignbyte(dw[k + 1], dw[k], sh);
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int dy = C == 2 ? d - (G + 1) : 0;
      uint64_t qlo = 0, qhi = 0;
      uint32_t tl[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) tl[s] = 0u;
      const uint32_t off0 = (uint32_t)(by + dy - R) * (uint32_t)W + (uint32_t)(bx - R - (G + 1));
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        uint32_t g[4];
        sr_load_row<NT>(rs, off0 + (uint32_t)j * (uint32_t)W, g);
        sr_row<R, G>(l[j], g, qlo, qhi, tl);
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t c = ((uint32_t)((s < 4 ? qlo : qhi) >> (16 * (s & 3))) & 0xFFFFu) + tl[s];
        cst[d][s >> 1] |= c << (16 * (s & 1));
      }
      __builtin_amdgcn_sched_barrier(0);  // one y shift's loads in flight at a time, as in k_search
    }
  } else {
    const uint8_t* lw = tb + ly * SR_PITCH + lx;  // the window's pixel (i, j), 0 .. 2R each way, is lw[j * SR_PITCH + i]
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int ty = by + (C == 2 ? d - (G + 1) : 0);
      uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
#pragma nounroll
      for (int s = 0; s < NS; ++s) {
        const int tx = bx + s - (G + 1);
        uint32_t sum = 0u;
#pragma nounroll
        for (int j = 0; j < NL; ++j) {
          const uint8_t* row = pr + (size_t)sr_clamp(ty + j - R, H - 1) * W;
#pragma nounroll
          for (int i = 0; i < NL; ++i) {
            const int a = lw[j * SR_PITCH + i], b = row[sr_clamp(tx + i - R, W - 1)];
            sum += (uint32_t)(a > b ? a - b : b - a);
          }
        }
        const uint32_t val = sum << (16 * (s & 1));
        const int k = s >> 1;
        w0 |= k == 0 ? val : 0u, w1 |= k == 1 ? val : 0u, w2 |= k == 2 ? val : 0u, w3 |= k == 3 ? val : 0u;
      }
      cst[d][0] = w0, cst[d][1] = w1, cst[d][2] = w2, cst[d][3] = w3;
    }
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (Ge::corner(d * NS + s)) continue;
      uint32_t c = (cst[d][s >> 1] >> (16 * (s & 1))) & 0xFFFFu;
      const bool label = s >= 1 && s <= NS - 2 && (C == 1 || (d >= 1 && d <= ND - 2));
      if (label) {
        const int tx = bx + s - (G + 1), ty = by + (C == 2 ? d - (G + 1) : 0);
        if (tx < 0 || tx >= W || ty < 0 || ty >= H) c = AG_NONE;
      }
      v[(size_t)(d * NS + s) * n] = (uint16_t)c;
    }
  }
}

template <int C, int G>
using AgVals = uint32_t[AgGeom<C, G>::K];  // one value per label

// the predecessor's value at (ex, ey) of its label frame extended by one; every index a constant once unrolled
template <int C, int G>
__device__ __forceinline__ uint32_t ag_ext(const AgVals<C, G>& L, int ex, int ey) {
  using Ge = AgGeom<C, G>;
  if (ex < 1 || ex > Ge::NE - 2) return AG_INF;
  if (C == 2 && (ey < 1 || ey > Ge::NE - 2)) return AG_INF;
  return L[C == 2 ? (ey - 1) * Ge::N1 + ex - 1 : ex - 1];
}

__device__ __forceinline__ uint32_t ag_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t ag_min3(uint32_t a, uint32_t b, uint32_t c) { return ag_min(ag_min(a, b), c); }

// One step of a chain.  In: the predecessor's L (AG_INF where inadmissible), their minimum mn (AG_INF: not live, or none --
// the path starts anew) and its bases q0, q1; the pixel's costs c (AG_NONE where inadmissible; all of them for a pixel that
// is not live) and bases r0, r1.  Out: the same of this pixel.  f: the lane's slot, cell e at f[e * AG_LANES].
template <int C, int G>
__device__ __forceinline__ void ag_step(AgVals<C, G>& L, uint32_t& mn, int& q0, int& q1, const AgVals<C, G>& c, int r0, int r1, uint32_t p1, uint32_t p2, uint32_t* f) {
  using Ge = AgGeom<C, G>;
  constexpr int N1 = Ge::N1, NE = Ge::NE, NEY = Ge::NEY, K = Ge::K;
  // F[e] = min(L[e], p1 + the minimum over the 3 x 3 (C = 1: the 3) around e), by rows then columns
#pragma unroll
  for (int ey = 0; ey < NEY; ++ey) {
#pragma unroll
    for (int ex = 0; ex < NE; ++ex) {
      uint32_t m = AG_INF;
#pragma unroll
      for (int dy = (C == 2 ? -1 : 0); dy <= (C == 2 ? 1 : 0); ++dy)
        m = ag_min(m, ag_min3(ag_ext<C, G>(L, ex - 1, ey + dy), ag_ext<C, G>(L, ex, ey + dy), ag_ext<C, G>(L, ex + 1, ey + dy)));
      f[(ey * NE + ex) * AG_LANES] = ag_min(ag_ext<C, G>(L, ex, ey), m + p1);
    }
  }
  // label k of this pixel has the displacement of the predecessor's label k + d
  const int lim = 2 * G + 2;
  int d0 = C == 1 ? q0 - r0 : r0 - q0, d1 = C == 2 ? r1 - q1 : 0;
  d0 = d0 < -lim ? -lim : (d0 > lim ? lim : d0), d1 = d1 < -lim ? -lim : (d1 > lim ? lim : d1);
  const bool live = mn != AG_INF;
  const uint32_t far = mn + p2;
  int ix[N1], iy[N1];
  bool vx[N1], vy[N1];
#pragma unroll
  for (int k = 0; k < N1; ++k) {
    const int ex = k + 1 + d0, ey = k + 1 + d1;
    vx[k] = ex >= 0 && ex < NE, vy[k] = ey >= 0 && ey < NE;
    ix[k] = sr_clamp(ex, NE - 1) * AG_LANES, iy[k] = sr_clamp(ey, NE - 1) * (NE * AG_LANES);
  }
  uint32_t m2 = AG_INF;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int kx = C == 2 ? k % N1 : k, ky = C == 2 ? k / N1 : 0;
    uint32_t t = f[ix[kx] + (C == 2 ? iy[ky] : 0)];
    t = vx[kx] && (C == 1 || vy[ky]) ? t : AG_INF;
    t = live ? ag_min(t, far) - mn : 0u;
    L[k] = c[k] == AG_NONE ? AG_INF : c[k] + t;
    m2 = ag_min(m2, L[k]);
  }
  mn = m2, q0 = r0, q1 = r1;
}

// which of the two directions of an orientation a workgroup runs (lo, hi: the orientation's bits), and its path volume
__device__ __forceinline__ int ag_bit(int paths, int lo, int hi, int which) { return which == 0 && (paths & lo) ? lo : hi; }
__device__ __forceinline__ int ag_slot(int paths, int bit) { return __popc((unsigned)(paths & (bit - 1))); }

// grid (columns / 64, the vertical directions in paths, pairs of the group).  path[slot][pair][label][y][x].
template <int C, int G>
__global__ __launch_bounds__(AG_LANES) void k_agg_path_v(const int32_t* __restrict__ field, const uint16_t* __restrict__ vol, int W,
                                                         int H, int paths, uint32_t p1, uint32_t p2, uint16_t* __restrict__ path) {
  using Ge = AgGeom<C, G>;
  constexpr int K = Ge::K;
  __shared__ uint32_t s_f[Ge::CELLS * AG_LANES];
  const int lane = threadIdx.x, x = blockIdx.x * AG_LANES + lane, p = blockIdx.z;
  if (x >= W) return;  // (no barrier below: the slots are the lanes' own)
  const int bit = ag_bit(paths, 4, 8, blockIdx.y);
  const bool down = bit == 4;
  const size_t n = (size_t)W * H;
  const int32_t* fp = field + (size_t)p * C * n + x;
  const uint16_t* vp = vol + (size_t)p * Ge::CELLS * n + x;
  uint16_t* lp = path + ((size_t)ag_slot(paths, bit) * gridDim.z + p) * K * n + x;
  uint32_t L[K], c[K], cn[K], mn = AG_INF;
  int q0 = 0, q1 = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = AG_INF;
  int32_t f0, f1 = 0;
  {
    const size_t row = (size_t)(down ? 0 : H - 1) * W;
#pragma unroll
    for (int k = 0; k < K; ++k) cn[k] = vp[(size_t)Ge::cell(k) * n + row];
    f0 = fp[row];
    if (C == 2) f1 = fp[n + row];
  }
#pragma nounroll
  for (int i = 0; i < H; ++i) {
    const size_t row = (size_t)(down ? i : H - 1 - i) * W;
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = cn[k];
    const int r0 = sr_whole(f0), r1 = C == 2 ? sr_whole(f1) : 0;
    if (i + 1 < H) {
      const size_t next = down ? row + W : row - W;
#pragma unroll
      for (int k = 0; k < K; ++k) cn[k] = vp[(size_t)Ge::cell(k) * n + next];
      f0 = fp[next];
      if (C == 2) f1 = fp[n + next];
    }
    ag_step<C, G>(L, mn, q0, q1, c, r0, r1, p1, p2, s_f + lane);
#pragma unroll
    for (int k = 0; k < K; ++k) lp[(size_t)k * n + row] = (uint16_t)ag_min(L[k], AG_NONE);
  }
}

// grid (rows / 64, the horizontal directions in paths, pairs of the group)
template <int C, int G>
__global__ __launch_bounds__(AG_LANES) void k_agg_path_h(const int32_t* __restrict__ field, const uint16_t* __restrict__ vol, int W,
                                                         int H, int paths, uint32_t p1, uint32_t p2, uint16_t* __restrict__ path) {
  using Ge = AgGeom<C, G>;
  constexpr int K = Ge::K, TX = Ge::TX, PITCH = Ge::PITCH, RPITCH = Ge::RPITCH;
  __shared__ uint16_t s_t[K * AG_LANES * PITCH];
  __shared__ int32_t s_r[C * AG_LANES * RPITCH];
  __shared__ uint32_t s_f[Ge::CELLS * AG_LANES];
  const int lane = threadIdx.x, y0 = blockIdx.x * AG_LANES, p = blockIdx.z;
  const int bit = ag_bit(paths, 1, 2, blockIdx.y);
  const bool right = bit == 1;
  const size_t n = (size_t)W * H;
  const int32_t* fp = field + (size_t)p * C * n;
  const uint16_t* vp = vol + (size_t)p * Ge::CELLS * n;
  uint16_t* lp = path + ((size_t)ag_slot(paths, bit) * gridDim.z + p) * K * n;
  uint32_t L[K], mn = AG_INF;
  int q0 = 0, q1 = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = AG_INF;
  const int chunks = (W + TX - 1) / TX;
#pragma nounroll
  for (int ci = 0; ci < chunks; ++ci) {
    const int xa = right ? ci * TX : W - (ci + 1) * TX;  // the chunk is columns xa .. xa + TX - 1, those inside the image
    // in: element it * 64 + lane of the chunk is column (it * 64 + lane) % TX of row (it * 64 + lane) / TX
#pragma nounroll
    for (int it = 0; it < TX; ++it) {
      const int e = it * AG_LANES + lane, col = e & (TX - 1), row = e / TX, x = xa + col, y = y0 + row;
      if (x < 0 || x >= W || y >= H) continue;
      const size_t at = (size_t)y * W + x;
#pragma unroll
      for (int k = 0; k < K; ++k) s_t[(k * AG_LANES + row) * PITCH + col] = vp[(size_t)Ge::cell(k) * n + at];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) s_r[(ch * AG_LANES + row) * RPITCH + col] = sr_whole(fp[(size_t)ch * n + at]);
    }
    __syncthreads();
    if (y0 + lane < H) {
#pragma nounroll
      for (int st = 0; st < TX; ++st) {
        const int col = right ? st : TX - 1 - st, x = xa + col;
        if (x < 0 || x >= W) continue;
        uint32_t c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] = s_t[(k * AG_LANES + lane) * PITCH + col];
        const int r0 = s_r[lane * RPITCH + col], r1 = C == 2 ? s_r[(AG_LANES + lane) * RPITCH + col] : 0;
        ag_step<C, G>(L, mn, q0, q1, c, r0, r1, p1, p2, s_f + lane);
#pragma unroll
        for (int k = 0; k < K; ++k) s_t[(k * AG_LANES + lane) * PITCH + col] = (uint16_t)ag_min(L[k], AG_NONE);
      }
    }
    __syncthreads();
#pragma nounroll
    for (int it = 0; it < TX; ++it) {
      const int e = it * AG_LANES + lane, col = e & (TX - 1), row = e / TX, x = xa + col, y = y0 + row;
      if (x < 0 || x >= W || y >= H) continue;
      const size_t at = (size_t)y * W + x;
#pragma unroll
      for (int k = 0; k < K; ++k) lp[(size_t)k * n + at] = s_t[(k * AG_LANES + row) * PITCH + col];
    }
    __syncthreads();
  }
}

// grid (pixels / 256, 1, pairs of the group); every pointer is the group's.  out may be field.
template <int C, int G>
__global__ __launch_bounds__(AG_CHOOSE_THREADS) void k_agg_choose(const int32_t* field, const uint16_t* __restrict__ vol,
                                                                  const uint16_t* __restrict__ path, int W, int H, int paths,
                                                                  int subpixel, int max_cost, int32_t* out,
                                                                  uint16_t* __restrict__ cost, uint8_t* __restrict__ choice,
                                                                  int32_t* __restrict__ stats, uint32_t* __restrict__ agg) {
  using Ge = AgGeom<C, G>;
  constexpr int K = Ge::K, N1 = Ge::N1, NE = Ge::NE;
  __shared__ int s_stats[4];
  const int tid = threadIdx.x, p = blockIdx.z;
  const uint32_t n = (uint32_t)W * (uint32_t)H, pix = blockIdx.x * AG_CHOOSE_THREADS + tid;
  if (tid < 4) s_stats[tid] = 0;
  __syncthreads();
  int cat = -1;  // 0 kept, 1 hole, 2 unmatched, 3 rejected
  if (pix < n) {
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint32_t)y * (uint32_t)W);
    const size_t at = (size_t)p * C * n + pix;
    const int32_t f0 = field[at], f1 = C == 2 ? field[at + n] : 0;
    int32_t o0 = SR_NONE, o1 = SR_NONE;
    uint32_t oc = 0xFFFFu, och = 255u, os = 0xFFFFFFFFu;
    cat = 1;
    if (f0 != SR_NONE) {
      const int r0 = sr_whole(f0), r1 = C == 2 ? sr_whole(f1) : 0;
      const int bx = C == 1 ? x - r0 : x + r0, by = y + r1;
      const uint16_t* v = vol + (size_t)p * Ge::CELLS * n + pix;
      uint32_t cv[Ge::CELLS], S[K];
#pragma unroll
      for (int c = 0; c < Ge::CELLS; ++c) cv[c] = Ge::corner(c) ? 0u : v[(size_t)c * n];
      const int dirs = __popc((unsigned)paths);
#pragma unroll
      for (int k = 0; k < K; ++k) S[k] = dirs ? 0u : cv[Ge::cell(k)];
#pragma nounroll
      for (int s = 0; s < dirs; ++s) {
        const uint16_t* l = path + ((size_t)s * gridDim.z + p) * K * n + pix;
#pragma unroll
        for (int k = 0; k < K; ++k) S[k] += l[(size_t)k * n];
      }
      // the candidates in the order (|kx| + |ky|, ky, kx): a later one wins only with a strictly smaller sum
      uint32_t bs = 0xFFFFFFFFu, bc = 0u, cxm = 0u, cxp = 0u, cym = 0u, cyp = 0u;
      int bkx = 0, bky = 0;
#pragma unroll
      for (int dist = 0; dist <= 2 * G; ++dist) {
#pragma unroll
        for (int ky = -G; ky <= G; ++ky) {
#pragma unroll
          for (int kx = -G; kx <= G; ++kx) {
            if ((C == 1 && ky != 0) || (kx < 0 ? -kx : kx) + (ky < 0 ? -ky : ky) != dist) continue;
            const int k = C == 2 ? (ky + G) * N1 + kx + G : kx + G, e = Ge::cell(k);
            if (cv[e] != AG_NONE && S[k] < bs) {
              bs = S[k], bc = cv[e], bkx = kx, bky = ky;
              cxm = cv[e - 1], cxp = cv[e + 1];
              if (C == 2) cym = cv[e - NE], cyp = cv[e + NE];
            }
          }
        }
      }
      cat = 2;
      if (bs != 0xFFFFFFFFu) {
        const int tx = bx + bkx, ty = by + bky;
        int qx = 0, qy = 0;
        if (subpixel) {
          if (tx >= 1 && tx <= W - 2) rf_axis(cxm, bc, cxp, qx);
          if (C == 2 && ty >= 1 && ty <= H - 2) rf_axis(cym, bc, cyp, qy);
        }
        oc = bc, os = bs;
        och = (uint32_t)(C == 1 ? bkx + G : (bky + G) * N1 + bkx + G);
        cat = 3;
        if ((int)bc <= max_cost) {
          cat = 0;
          o0 = C == 1 ? 256 * (r0 - bkx) - qx : 256 * (r0 + bkx) + qx;
          o1 = 256 * (r1 + bky) + qy;
        }
      }
    }
    out[at] = o0;
    if (C == 2) out[at + n] = cat == 0 ? o1 : SR_NONE;
    const size_t px = (size_t)p * n + pix;
    if (cost) cost[px] = (uint16_t)oc;
    if (choice) choice[px] = (uint8_t)och;
    if (agg) agg[px] = os;
  }
  if (stats) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long m = __ballot(cat == k);
      if ((tid & 63) == 0 && m) atomicAdd(&s_stats[k], __popcll(m));
    }
    __syncthreads();
    if (tid < 4 && s_stats[tid]) atomicAdd(stats + (size_t)p * 4 + tid, s_stats[tid]);
  }
}

}  // namespace gpc
