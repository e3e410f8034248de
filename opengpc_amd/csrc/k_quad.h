// k_quad.h -- circular matches over a stereo sequence closed into quads (gpc_hip_quads_*): L_t -> R_t -> R_t+1 -> L_t+1
// -> L_t, joined on the device by pixel position (include/gpc_hip.h has the rule in full).  The shape is k_track.h's:
// per-pixel planes that hold the lowest record index of a pixel, integer minima as the only atomics, a launch per phase,
// nothing that waits across workgroups inside a launch.  Every launch covers all the steps of a group (blockIdx.y).
//   k_track_fill    (k_track.h) the planes and the owner words to TR_NONE;
//   k_quad_scatter  first_S[f][left pixel], first_FL[t][source pixel], first_FR[t][source pixel] = min record index;
//   k_quad_close    support i of step t: a start?  then the five dependent lookups; where the circle closes on i',
//                   cand[t][i] = i' and i into owner[t][i'] with a minimum, else cand[t][i] = -1;
//   k_quad_settle   cand[t][i] stays only where owner[t][i'] == i; the quads of every chunk counted;
//   k_quad_scan     exclusive scan of a step's chunk counts (one workgroup per step), the total into nquads[t];
//   k_quad_write    every kept start numbers itself (chunk offset + rank) and writes its quad below quad_cap.
// And for the matching call in front of them (gpc_hip_match_stereo_sequence_device):
//   k_quad_sides    the code images, candidate bytes and statistics words of 2 N images stored [t][side] copied into one
//                   image-major block per side, which a flow join reads as the frames of a sequence.
// Random 4-byte reads and minima over 12 bytes of planes per pixel and step: latency, not bandwidth, is what this costs.
#pragma once
#include "k_track.h"

#define QD_THREADS TR_THREADS
#define QD_CHUNK TR_CHUNK    // support slots per workgroup of the settle and write kernels
#define QD_MAX_DISP 16384.f  // |d| above this takes no part (no image is wider: check_dims)

namespace gpc {

struct QdSup {  // gpc_support
  int32_t x, y;
  float d;
};
struct QdQuad {  // gpc_quad
  int32_t x, y, d0, u, v, d1, support0, support1;
};

// The records and planes of one group of steps: frames [0, steps], steps [0, steps) (the host has moved every pointer to
// the group's first frame / step).
struct QdArgs {
  const QdSup* sup;     // [steps + 1][cap_s]
  const int32_t* nsup;  // [steps + 1]
  const TrRec* fl;      // [steps][cap_f]
  const TrRec* fr;      // [steps][cap_f]
  const int32_t* nfl;   // [steps]
  const int32_t* nfr;   // [steps]
  int32_t* first_s;     // [steps + 1][H][W]
  int32_t* first_fl;    // [steps][H][W]
  int32_t* first_fr;    // [steps][H][W]
  int32_t* owner;       // [steps][cap_s]: the lowest start of step t that closes on support i' of frame t + 1
  int32_t* cand;        // [steps][cap_s]: i' of start i, -1 where i is no start or its circle does not close
  int32_t* blk;         // [steps][nchunk]
  int cap_s, cap_f, W, H, steps, tol, nchunk;
};

// Takes part: inside the image, d finite and integral with |d| <= 16384 (tested BEFORE the conversion, so that the
// conversion is always defined), and the right pixel x - d inside the row.  *di = (int)d then.
__device__ __forceinline__ bool qd_support(const QdSup& s, int W, int H, int* di) {
  if (!((uint32_t)s.x < (uint32_t)W && (uint32_t)s.y < (uint32_t)H)) return false;
  if (!(fabsf(s.d) <= QD_MAX_DISP) || truncf(s.d) != s.d) return false;  // (NaN and infinities fail the first test)
  const int d = (int)s.d;
  *di = d;
  return (uint32_t)(s.x - d) < (uint32_t)W;
}

// grid (x, 3 * steps + 1): rows 0 .. steps are the supports of the frames, then the left flow of every step, then the right
__global__ __launch_bounds__(QD_THREADS) void k_quad_scatter(const QdArgs a) {
  const int r = blockIdx.y;
  const long n = (long)a.W * a.H;
  if (r <= a.steps) {
    const int m = tr_count(a.nsup, r, a.cap_s);
    const QdSup* rec = a.sup + (long)r * a.cap_s;
    int32_t* pl = a.first_s + (long)r * n;
    for (long il = (long)blockIdx.x * QD_THREADS + threadIdx.x; il < m; il += (long)gridDim.x * QD_THREADS) {
      const int i = (int)il;  // (stepped in long: m may be within a grid's width of INT_MAX)
      const QdSup s = rec[i];
      int d;
      if (qd_support(s, a.W, a.H, &d)) atomicMin(&pl[s.y * a.W + s.x], i);
    }
    return;
  }
  const bool right = r > 2 * a.steps;
  const int t = r - a.steps - 1 - (right ? a.steps : 0);
  const int m = tr_count(right ? a.nfr : a.nfl, t, a.cap_f);
  const TrRec* rec = (right ? a.fr : a.fl) + (long)t * a.cap_f;
  int32_t* pl = (right ? a.first_fr : a.first_fl) + (long)t * n;
  for (long il = (long)blockIdx.x * QD_THREADS + threadIdx.x; il < m; il += (long)gridDim.x * QD_THREADS) {
    const int i = (int)il;
    const TrRec c = rec[i];
    if (tr_inside(c, a.W, a.H)) atomicMin(&pl[c.sy * a.W + c.sx], i);
  }
}

// The circle of support i of step t: false where i is no start or the circle does not close.  A plane holds only indices
// of records that take part and lie below their count, so what it names may be read without a further test.
__device__ __forceinline__ bool qd_circle(const QdArgs& a, int t, int i, QdQuad* q) {
  const long n = (long)a.W * a.H;
  const QdSup s = a.sup[(long)t * a.cap_s + i];
  int d;
  if (!qd_support(s, a.W, a.H, &d)) return false;
  const int pa = s.y * a.W + s.x;
  if (a.first_s[(long)t * n + pa] != i) return false;  // (another support of this left pixel is the start)
  const int j = a.first_fl[(long)t * n + pa];
  const int k = a.first_fr[(long)t * n + pa - d];
  if (j == TR_NONE || k == TR_NONE) return false;
  const TrRec fl = a.fl[(long)t * a.cap_f + j];
  const TrRec fr = a.fr[(long)t * a.cap_f + k];
  const int i1 = a.first_s[(long)(t + 1) * n + fl.ty * a.W + fl.tx];
  if (i1 == TR_NONE) return false;
  const int d1 = (int)a.sup[(long)(t + 1) * a.cap_s + i1].d;  // (takes part: the conversion is defined)
  const int ex = fl.tx - d1 - fr.tx, ey = fl.ty - fr.ty;
  if (ex > a.tol || -ex > a.tol || ey > a.tol || -ey > a.tol) return false;
  q->x = s.x;
  q->y = s.y;
  q->d0 = d;
  q->u = fl.tx - s.x;
  q->v = fl.ty - s.y;
  q->d1 = d1;
  q->support0 = i;
  q->support1 = i1;
  return true;
}

// grid (x, steps): one thread per support slot of step t
__global__ __launch_bounds__(QD_THREADS) void k_quad_close(const QdArgs a) {
  const int t = blockIdx.y;
  const int m = tr_count(a.nsup, t, a.cap_s);
  int32_t* cd = a.cand + (long)t * a.cap_s;
  int32_t* ow = a.owner + (long)t * a.cap_s;
  for (long il = (long)blockIdx.x * QD_THREADS + threadIdx.x; il < m; il += (long)gridDim.x * QD_THREADS) {
    const int i = (int)il;
    QdQuad q;
    int i1 = -1;
    if (qd_circle(a, t, i, &q)) {
      i1 = q.support1;
      atomicMin(&ow[i1], i);
    }
    cd[i] = i1;
  }
}

// grid (nchunk, steps): a start that another start of the step beat to its i' gives way; blk[t][b] = quads of the chunk
__global__ __launch_bounds__(QD_THREADS) void k_quad_settle(const QdArgs a) {
  const int t = blockIdx.y;
  const int m = tr_count(a.nsup, t, a.cap_s);
  const int i0 = blockIdx.x * QD_CHUNK;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int kept = 0;
  if (i0 < m) {
    int32_t* cd = a.cand + (long)t * a.cap_s;
    const int32_t* ow = a.owner + (long)t * a.cap_s;
#pragma unroll 1
    for (int k = 0; k < QD_CHUNK / QD_THREADS; ++k) {
      const int i = i0 + k * QD_THREADS + threadIdx.x;
      if (i < m) {
        const int i1 = cd[i];
        if (i1 >= 0) {
          if (ow[i1] == i) ++kept;
          else cd[i] = -1;
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&s_n, kept);
  __syncthreads();
  if (threadIdx.x == 0) a.blk[(long)t * a.nchunk + blockIdx.x] = s_n;
}

// grid (steps): workgroup t scans the chunk counts of step t in place, the step's total into nquads[t]
__global__ __launch_bounds__(1024) void k_quad_scan(int32_t* __restrict__ blk, int nchunk, int32_t* __restrict__ nquads) {
  tr_scan_block(blk + (long)blockIdx.x * nchunk, nchunk, nquads + blockIdx.x);
}

// grid (nchunk, steps): the quads of chunk b of step t go to quads[t][blk[t][b] + rank in support order], below quad_cap
__global__ __launch_bounds__(QD_THREADS) void k_quad_write(const QdArgs a, QdQuad* __restrict__ quads, int quad_cap) {
  const int t = blockIdx.y;
  const int m = tr_count(a.nsup, t, a.cap_s);
  const int i0 = blockIdx.x * QD_CHUNK;
  if (i0 >= m) return;  // (uniform over the workgroup)
  const int32_t* cd = a.cand + (long)t * a.cap_s;
  __shared__ int s_w[QD_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pos = a.blk[(long)t * a.nchunk + blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < QD_CHUNK / QD_THREADS; ++k) {
    if (pos >= quad_cap) return;  // (uniform: nothing of this chunk is left to write)
    const int i = i0 + k * QD_THREADS + threadIdx.x;
    const bool keep = i < m && cd[i] >= 0;
    const unsigned long long mk = __ballot(keep);
    if (lane == 0) s_w[wave] = __popcll(mk);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < QD_THREADS / 64; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    if (keep) {
      const int at = pos + woff + __popcll(mk & ((1ull << lane) - 1ull));
      QdQuad q;
      if (at < quad_cap && qd_circle(a, t, i, &q)) quads[(long)t * quad_cap + at] = q;  // (the circle is the one k_quad_close saw)
    }
    pos += tot;
    __syncthreads();
  }
}

// grid (x, N, 2): image 2 t + side -> image t of side's block, 16 bytes per thread and turn.  g_code / g_cand: 16-byte
// groups of a code image / of an image of candidate bytes (cand null: none are copied); statistics words: N x GPC_STAT_STRIDE
// per side, by the first workgroup of every image.
__global__ __launch_bounds__(QD_THREADS) void k_quad_sides(const uint4* __restrict__ codes, uint4* __restrict__ codes_l,
                                                           uint4* __restrict__ codes_r, long g_code, const uint4* __restrict__ cand,
                                                           uint4* __restrict__ cand_l, uint4* __restrict__ cand_r, long g_cand,
                                                           const int32_t* __restrict__ stats, int32_t* __restrict__ side_stats) {
  const int t = blockIdx.y, side = blockIdx.z, N = gridDim.y;
  const long img = 2l * t + side;
  const uint4* src = codes + img * g_code;
  uint4* dst = (side ? codes_r : codes_l) + (long)t * g_code;
  for (long i = (long)blockIdx.x * QD_THREADS + threadIdx.x; i < g_code; i += (long)gridDim.x * QD_THREADS) dst[i] = src[i];
  if (cand) {
    const uint4* cs = cand + img * g_cand;
    uint4* cd = (side ? cand_r : cand_l) + (long)t * g_cand;
    for (long i = (long)blockIdx.x * QD_THREADS + threadIdx.x; i < g_cand; i += (long)gridDim.x * QD_THREADS) cd[i] = cs[i];
  }
  if (blockIdx.x == 0 && threadIdx.x < GPC_STAT_STRIDE)
    side_stats[((long)side * N + t) * GPC_STAT_STRIDE + threadIdx.x] = stats[img * GPC_STAT_STRIDE + threadIdx.x];
}

}  // namespace gpc
