// k_search.h -- the local dense search around every pixel of a filled field (gpc_hip_search_*).  include/gpc_hip.h has the
// rule in full; it is made of integers only.  A valued pixel's field value, rounded to whole pixels, names a base target in
// the other image; the (2r+1)^2 SAD of the pixel's window against the windows at the targets within R pixels of the base
// picks the best one, and the costs one pixel either side of it give the parabola of k_refine per axis.
//   k_search<C, R, G>   C channels, radius R, range G.  A workgroup is a tile of 32 x 8 pixels, one lane each.  The tile of
//                       the left image is staged in LDS with its apron of R, addresses already clamped, so the left side
//                       has no border case; a lane takes its 2R+1 window rows out of it once, as aligned dwords shifted
//                       into place (v_alignbyte), and keeps them in registers.  The right image is read from global memory
//                       through buffer loads, the whole image of the pair being the buffer as in k_refine: the targets of
//                       the lanes of a wave lie side by side in a filled field, so their rows share cache lines.  A target
//                       row with ALL its x shifts, -(G+1) .. G+1, is 2R+1 + 2(G+1) <= 15 bytes: ONE load (sr_load_row).
//                       v_qsad_pk_u16_u8 sums a 4-byte chunk of the left row against the target row at four byte shifts
//                       per instruction (two instructions cover up to eight shifts); the row's last 1 or 3 bytes go through
//                       v_sad_u8 on words masked after the shift, as in k_refine.  With C = 2 the same row step runs for
//                       every y shift -(G+1) .. G+1, one after the other, so that one set of accumulators is live; the
//                       (2G+3)^2 costs are kept as 16-bit halves (the largest cost is 81 * 255).  The choice among the
//                       candidates is a chain of compares in the order of the rule's tie-break, all indices constants.
//                       A pixel of which some target window (shifts included) leaves the image takes the byte-wise path:
//                       the same costs by clamped single-byte reads.  Both paths feed the same choice.
#pragma once
#include "gpc_device.h"
#include "k_refine.h"  // rf_axis, the rf_u32x* vectors
#include "search_host.h"

#define SR_THREADS (SR_TILE_W * SR_TILE_H)
#define SR_NONE (-2147483647 - 1)
#define SR_PITCH 44                               // bytes per staged row: 32 + 2 * 4, and the aligned dwords a lane reads end at byte 28 + 12
#define SR_ROWS (SR_TILE_H + 2 * SR_MAX_RADIUS)   // staged rows
#define SR_LDS_BYTES (SR_ROWS * SR_PITCH + 16)    // the tile and the four counts of the workgroup

namespace gpc {

// sgn(f) * ((|f| + 128) >> 8); |f| <= 2^31 fits 32 unsigned bits with the 128 on top
__device__ __forceinline__ int sr_whole(int32_t f) {
  const uint32_t a = f < 0 ? 0u - (uint32_t)f : (uint32_t)f;
  const int r = (int)((a + 128u) >> 8);
  return f < 0 ? -r : r;
}

__device__ __forceinline__ int sr_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// NB bytes of the image from byte `off` on, in v[0 .. (NB + 3) / 4) (the rest 0): rf_load_row without its byte-wise second
// try -- the caller has checked that the dwords lie inside the buffer, so the loads of a pixel are one straight line
template <int NB>
__device__ __forceinline__ void sr_load_row(const __amdgpu_buffer_rsrc_t img, uint32_t off, uint32_t (&v)[4]) {
  constexpr int ND = (NB + 3) / 4;
  v[0] = v[1] = v[2] = v[3] = 0u;
  if constexpr (ND == 1) {
    v[0] = __builtin_amdgcn_raw_buffer_load_b32(img, off, 0, 0);
  } else if constexpr (ND == 2) {
    const rf_u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y;
  } else if constexpr (ND == 3) {
    const rf_u32x3 q = __builtin_amdgcn_raw_buffer_load_b96(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z;
  } else {
    const rf_u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(img, off, 0, 0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
}

// One window row against one target row: l = the left row from x - R, g = the target row from tx - R - (G + 1).  The 16-bit
// fields of qlo gather the full chunks' sums at the byte shifts 0 .. 3, those of qhi at 4 .. 7; tl[s] the tail's at shift s.
template <int R, int G>
__device__ __forceinline__ void sr_row(const uint32_t (&l)[3], const uint32_t (&g)[4], uint64_t& qlo, uint64_t& qhi,
                                       uint32_t (&tl)[2 * G + 3]) {
  constexpr int NL = 2 * R + 1, NS = 2 * G + 3, CH = NL / 4, TAIL = NL % 4;  // TAIL is 1 or 3
  constexpr uint32_t TM = TAIL == 1 ? 0xFFu : 0xFFFFFFu;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    qlo = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)g[c + 1] << 32) | g[c], l[c], qlo);
    if (NS > 4) qhi = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)g[(c + 2) & 3] << 32) | g[c + 1], l[c], qhi);
  }
  const uint32_t lt = l[CH] & TM;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int b = 4 * CH + s, w = b / 4, sh = b % 4;  // (b + TAIL - 1 <= 14: inside the four dwords)
    const uint32_t hi = w + 1 < 4 ? g[(w + 1) & 3] : 0u;
    const uint32_t word = sh ? __builtin_amdgcn_alignbyte(hi, g[w], (uint32_t)sh) : g[w];
    tl[s] = __builtin_amdgcn_sad_u8(word & TM, lt, tl[s]);
  }
}

// grid (tiles x, tiles y, P).  n = W * H: the images of pair t are imgL + t * n and imgR + t * n.  out may be field.
template <int C, int R, int G>
__global__ __launch_bounds__(SR_THREADS) void k_search(const int32_t* field, const uint8_t* __restrict__ imgL,
                                                       const uint8_t* __restrict__ imgR, int W, int H, int subpixel, int max_cost,
                                                       int32_t* out, uint16_t* __restrict__ cost, uint8_t* __restrict__ choice,
                                                       int32_t* __restrict__ stats) {
  static_assert((C == 1 || C == 2) && R >= 1 && R <= SR_MAX_RADIUS && G >= 0 && G <= SR_MAX_RANGE, "a target row with its shifts fits one 16-byte load");
  constexpr int NL = 2 * R + 1, NS = 2 * G + 3, NT = NL + NS - 1, ND = C == 2 ? NS : 1;
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
  int cat = -1;  // 0 kept, 1 hole, 2 unmatched, 3 rejected
  if (x < W && y < H) {
    const size_t at = (size_t)p * C * n + (size_t)y * W + x;
    const int32_t f0 = field[at], f1 = C == 2 ? field[at + n] : 0;
    int32_t o0 = SR_NONE, o1 = SR_NONE;
    uint32_t oc = 0xFFFFu, och = 255u;
    cat = 1;
    if (f0 != SR_NONE) {
      const int r0 = sr_whole(f0), r1 = C == 2 ? sr_whole(f1) : 0;
      const int bx = C == 1 ? x - r0 : x + r0, by = y + r1;
      uint32_t cst[ND][4];  // the cost at y shift d - (G + 1) and x shift s - (G + 1): half s & 1 of cst[d][s >> 1]
#pragma unroll
      for (int d = 0; d < ND; ++d) cst[d][0] = cst[d][1] = cst[d][2] = cst[d][3] = 0u;
      // (the last condition: the 16 bytes of the last row's load end inside the image -- a load that reaches past the
      // buffer's end comes back as zeros; the few pixels it excludes at the image's end take the byte-wise path)
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
          __builtin_amdgcn_sched_barrier(0);  // one y shift's loads in flight at a time: hoisting them all costs the registers of seven
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
            const uint32_t v = sum << (16 * (s & 1));
            const int k = s >> 1;
            w0 |= k == 0 ? v : 0u, w1 |= k == 1 ? v : 0u, w2 |= k == 2 ? v : 0u, w3 |= k == 3 ? v : 0u;
          }
          cst[d][0] = w0, cst[d][1] = w1, cst[d][2] = w2, cst[d][3] = w3;
        }
      }
#define SR_COST(d, s) ((cst[d][(s) >> 1] >> (16 * ((s) & 1))) & 0xFFFFu)
      // the candidates in the order (|kx| + |ky|, ky, kx): a later one wins only with a strictly smaller cost
      uint32_t bc = 0xFFFFFFFFu, cxm = 0u, cxp = 0u, cym = 0u, cyp = 0u;
      int bkx = 0, bky = 0;
#pragma unroll
      for (int dist = 0; dist <= 2 * G; ++dist) {
#pragma unroll
        for (int ky = -G; ky <= G; ++ky) {
#pragma unroll
          for (int kx = -G; kx <= G; ++kx) {
            if ((C == 1 && ky != 0) || (kx < 0 ? -kx : kx) + (ky < 0 ? -ky : ky) != dist) continue;
            const int d = C == 2 ? ky + G + 1 : 0, s = kx + G + 1;
            const int tx = bx + kx, ty = by + ky;
            const uint32_t c = SR_COST(d, s);
            if (tx >= 0 && tx < W && ty >= 0 && ty < H && c < bc) {
              bc = c, bkx = kx, bky = ky;
              cxm = SR_COST(d, s - 1), cxp = SR_COST(d, s + 1);
              if (C == 2) cym = SR_COST(d > 0 ? d - 1 : 0, s), cyp = SR_COST(d + 1 < ND ? d + 1 : 0, s);
            }
          }
        }
      }
#undef SR_COST
      cat = 2;
      if (bc != 0xFFFFFFFFu) {
        const int tx = bx + bkx, ty = by + bky;
        int qx = 0, qy = 0;
        if (subpixel) {
          if (tx >= 1 && tx <= W - 2) rf_axis(cxm, bc, cxp, qx);
          if (C == 2 && ty >= 1 && ty <= H - 2) rf_axis(cym, bc, cyp, qy);
        }
        oc = bc;
        och = (uint32_t)(C == 1 ? bkx + G : (bky + G) * (2 * G + 1) + bkx + G);
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
    const size_t px = (size_t)p * n + (size_t)y * W + x;
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
    if (tid < 4 && s_stats[tid]) atomicAdd(stats + (size_t)p * 4 + tid, s_stats[tid]);
  }
}

}  // namespace gpc
