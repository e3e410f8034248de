// k_propagate.h -- one iteration of the propagation of field values between neighbours (gpc_hip_propagate_*).  include/gpc_hip.h
// has the rule in full; it is made of integers only.  A pixel tries the whole-pixel displacements of its 4 or 8 neighbours at
// the iteration's stride beside its own and keeps whichever gives the smallest (2r+1)^2 SAD against the other image; the
// iteration reads only the previous field and writes a whole new one.
//   k_propagate<C, R, NB>  C channels, radius R, NB neighbours.  The tile, its staging and a lane's window rows are those of
//                       k_search: a workgroup is 32 x 8 pixels, one lane each; the left tile lies in LDS with its apron,
//                       addresses already clamped, and a lane takes its 2R+1 window rows out once, into registers.
//                       First every candidate is GATHERED (all indices constants): the neighbour's value straight from the
//                       previous field -- the stride is uniform, so a row of lanes reads a row of the field --, its
//                       displacement, whether its target lies inside the image, and whether the displacement differs from
//                       the pixel's own and from every earlier candidate's.  A candidate that does not exist takes the
//                       pixel's own displacement and so drops out as a duplicate.  What is left is a bit mask per lane.
//                       Then ONE loop over j = 0 .. NB evaluates the candidates whose bit is set; a wave none of whose lanes
//                       has bit j skips j.  The displacement of j comes out of the registers by a chain of selects on the
//                       (uniform) j: nothing indexes a register array dynamically, and the cost code exists once.
//                       A candidate's cost is a full window against ONE target: a target row is 2R+1 <= 9 bytes, one buffer
//                       load of 4, 8 or 12 bytes at a byte address (sr_load_row), v_sad_u8 per dword, the last one masked.
//                       A candidate any of whose loads would leave the image takes the byte-wise path with clamped
//                       addresses.  Both feed the same compare: a later candidate wins only with a strictly smaller cost.
//                       The pixel's own candidate is evaluated only when something can be compared with it or the cost is
//                       asked for: in a filled field most lanes have no second displacement and evaluate nothing.
#pragma once
#include "gpc_device.h"
#include "k_search.h"  // the tile (SR_*), sr_whole, sr_clamp, sr_load_row
#include "propagate_host.h"

namespace gpc {

// the (2R+1)^2 SAD of the lane's window -- l: its rows in registers, lw: its first byte in the staged tile -- against the
// window around (tx, ty) of the right image pr (rs: the same image as a buffer of n bytes)
template <int R>
__device__ __forceinline__ uint32_t pg_cost(const uint32_t (&l)[2 * R + 1][3], const uint8_t* lw, const uint8_t* __restrict__ pr,
                                            const __amdgpu_buffer_rsrc_t rs, int tx, int ty, int W, int H, uint32_t n) {
  constexpr int NL = 2 * R + 1, CH = NL / 4, TAIL = NL % 4, ND = (NL + 3) / 4;  // TAIL is 1 or 3
  constexpr uint32_t TM = TAIL == 1 ? 0xFFu : 0xFFFFFFu;
  uint32_t sum = 0u;
  // (the last condition: the dwords of the last row's load end inside the image -- a load that reaches past the buffer's end
  // comes back as zeros; the few targets it excludes at the image's end take the byte-wise path)
  const bool fast = tx - R >= 0 && tx + R <= W - 1 && ty - R >= 0 && ty + R <= H - 1 &&
                    (uint32_t)(ty + R) * (uint32_t)W + (uint32_t)(tx - R) + 4u * ND <= n;
  if (fast) {
    const uint32_t off0 = (uint32_t)(ty - R) * (uint32_t)W + (uint32_t)(tx - R);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      uint32_t g[4];
      sr_load_row<NL>(rs, off0 + (uint32_t)j * (uint32_t)W, g);
#pragma unroll
      for (int c = 0; c < CH; ++c) sum = __builtin_amdgcn_sad_u8(g[c], l[j][c], sum);
      sum = __builtin_amdgcn_sad_u8(g[CH] & TM, l[j][CH] & TM, sum);
    }
  } else {
#pragma nounroll
    for (int j = 0; j < NL; ++j) {
      const uint8_t* row = pr + (size_t)sr_clamp(ty + j - R, H - 1) * W;
#pragma nounroll
      for (int i = 0; i < NL; ++i) {
        const int a = lw[j * SR_PITCH + i], b = row[sr_clamp(tx + i - R, W - 1)];
        sum += (uint32_t)(a > b ? a - b : b - a);
      }
    }
  }
  return sum;
}

// grid (tiles x, tiles y, P).  n = W * H: the images of pair t are imgL + t * n and imgR + t * n.  prev and out are different
// blocks (the host's plan sees to it).  s: the stride.  stats: this iteration's row of pair 0; stats_pitch words between pairs.
template <int C, int R, int NB>
__global__ __launch_bounds__(SR_THREADS) void k_propagate(const int32_t* __restrict__ prev, const uint8_t* __restrict__ imgL,
                                                          const uint8_t* __restrict__ imgR, int W, int H, int s,
                                                          int32_t* __restrict__ out, uint16_t* __restrict__ cost,
                                                          uint8_t* __restrict__ choice, int32_t* __restrict__ stats, int stats_pitch) {
  static_assert((C == 1 || C == 2) && R >= 1 && R <= SR_MAX_RADIUS && (NB == 4 || NB == 8), "a target row fits one 12-byte load");
  constexpr int NL = 2 * R + 1;
  constexpr int NLW = (NL + 3) / 4, NLD = (NL + 3 + 3) / 4;  // dwords of a left row, and of the aligned read that holds it
  constexpr int TWA = SR_TILE_W + 2 * R, THA = SR_TILE_H + 2 * R;
  __shared__ uint32_t s_tile[SR_ROWS * SR_PITCH / 4];
  __shared__ int s_stats[4];
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
  if (tid < 4) s_stats[tid] = 0;
  __syncthreads();

  const int x = x0 + lx, y = y0 + ly;
  int cat = -1;  // 0 kept its own value, 1 hole, 2 unmatched, 3 moved to a neighbour's value
  if (x < W && y < H) {
    const int32_t* pf = prev + (size_t)p * C * n;
    const size_t at = (size_t)y * W + x;
    const int32_t f0 = pf[at], f1 = C == 2 ? pf[at + n] : 0;
    int32_t o0 = f0, o1 = f1;
    uint32_t oc = 0xFFFFu, och = 255u;
    cat = 1;
    if (f0 != SR_NONE) {
      // the displacement of candidate j, target less pixel: (-r_0, 0) with C = 1, (r_0, r_1) with C = 2
      int cx[NB + 1], cy[NB + 1];
      cx[0] = C == 1 ? -sr_whole(f0) : sr_whole(f0), cy[0] = C == 2 ? sr_whole(f1) : 0;
      const bool own = x + cx[0] >= 0 && x + cx[0] < W && y + cy[0] >= 0 && y + cy[0] < H;
      uint32_t ev = 0u;  // bit j: candidate j >= 1 is admissible and no duplicate
#pragma unroll
      for (int j = 1; j <= NB; ++j) {
        // the sources in the rule's order: left, right, up, down, then the four diagonals row by row
        const int ox = j <= 2 ? 2 * j - 3 : (j <= 4 ? 0 : 2 * ((j - 5) & 1) - 1);
        const int oy = j <= 2 ? 0 : (j <= 4 ? 2 * j - 7 : 2 * ((j - 5) >> 1) - 1);
        const int qx = x + ox * s, qy = y + oy * s;
        cx[j] = cx[0], cy[j] = cy[0];
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
          const size_t aq = (size_t)qy * W + qx;
          const int32_t g0 = pf[aq];
          if (g0 != SR_NONE) {
            cx[j] = C == 1 ? -sr_whole(g0) : sr_whole(g0);
            if (C == 2) cy[j] = sr_whole(pf[aq + n]);
          }
        }
        bool fresh = x + cx[j] >= 0 && x + cx[j] < W && y + cy[j] >= 0 && y + cy[j] < H;
#pragma unroll
        for (int k = 0; k < j; ++k) fresh = fresh && (cx[k] != cx[j] || cy[k] != cy[j]);
        ev |= fresh ? 1u << j : 0u;
      }
      if (own && (ev != 0u || cost != nullptr)) ev |= 1u;
      uint32_t bc = 0xFFFFFFFFu;
      int bj = own ? 0 : -1, bx = cx[0], by = cy[0];
      if (ev != 0u) {
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
        const uint8_t* lw = tb + ly * SR_PITCH + lx;  // the window's pixel (i, j), 0 .. 2R each way, is lw[j * SR_PITCH + i]
        bj = -1;
#pragma nounroll
        for (int j = 0; j <= NB; ++j) {
          if ((ev >> j) & 1u) {
            int dx = cx[0], dy = cy[0];
#pragma unroll
            for (int k = 1; k <= NB; ++k) dx = j == k ? cx[k] : dx, dy = j == k ? cy[k] : dy;
            const uint32_t c = pg_cost<R>(l, lw, pr, rs, x + dx, y + dy, W, H, n);
            if (c < bc) bc = c, bj = j, bx = dx, by = dy;
          }
        }
      }
      cat = 2;
      if (bj >= 0) {
        cat = bj == 0 ? 0 : 3;
        oc = bc & 0xFFFFu;  // (read only where the cost is asked for, and then every admissible own candidate was evaluated)
        och = (uint32_t)bj;
        if (bj > 0) o0 = C == 1 ? -256 * bx : 256 * bx, o1 = 256 * by;
      }
    }
    int32_t* po = out + (size_t)p * C * n;
    po[at] = o0;
    if (C == 2) po[at + n] = o1;
    const size_t px = (size_t)p * n + at;
    if (cost) cost[px] = (uint16_t)oc;
    if (choice) choice[px] = (uint8_t)och;
  }
  if (stats) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long m = __ballot(cat == k);
      if ((tid & 63) == 0 && m) atomicAdd(&s_stats[k], __popcll(m));
    }
    __syncthreads();
    if (tid < 4 && s_stats[tid]) atomicAdd(stats + (size_t)p * stats_pitch + tid, s_stats[tid]);
  }
}

}  // namespace gpc
