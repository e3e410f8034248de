// k_pyramid.h -- matching over an image pyramid (gpc_hip_pyramid_*): the 2x2-mean downsampling step and the merge of the
// levels' records.
//
// k_pyr_down   one step of the pyramid: out[y][x] = (a + b + c + d + 2) >> 2 over in[2y .. 2y+1][2x .. 2x+1].
//
// The merge of one pair: level 0's records, then level 1's whose source block holds the source pixel of no record kept so
// far, and so on.  "Holds a source pixel" is a lookup in a per-pair occupancy BIT plane over level 0's pixels
// ([npairs][H][wpr] words, wpr = ceil(W / 32), cleared by the host per call): a kept level-l record sets the bit of its
// mapped source pixel (x << l, y << l); a level-l block is 2^l aligned bits in each of 2^l rows, so its test is 2^l word
// reads and one mask.  Per level, in launch order:
//   k_pyr_keep   tests a chunk of PY_CHUNK records against the plane (level 0: nothing to test), stores the keep bits as
//                one ballot word per wave and the chunk's count;
//   k_pyr_scan   per pair, exclusive scan of the chunk counts behind the pair's total so far; the level's count and the
//                new total;
//   k_pyr_write  the kept records, mapped to level 0, at their place (those below the capacity), and -- the tests of the
//                whole level being done with the launch before -- their bits in the plane.
// The keep bits are computed once and read twice, so what is written and what is marked cannot differ.
#pragma once
#include "gpc_device.h"

#define PY_THREADS 256
#define PY_CHUNK (PY_THREADS * 8)  // records per workgroup of k_pyr_keep and k_pyr_write
#define PY_DOWN_COLS 64            // lanes along a row per workgroup of k_pyr_down: 512 source bytes
#define PY_DOWN_ROWS 4             // output rows per workgroup

namespace gpc {

// grid (ceil(W / 8 / PY_DOWN_COLS), ceil(H / 2 / PY_DOWN_ROWS), nimages).  A lane reads 8 bytes of two source rows and
// writes 4 bytes.  Per 32-bit word (v & 0x00FF00FF) + ((v >> 8) & 0x00FF00FF) holds the two horizontal pair sums in its
// halves; two rows of them plus 2 stay below 1024 (4 * 255 + 2 = 1022), so after >> 2 bytes 0 and 2 of the word are the two
// results, and one v_perm packs those of both words.
__global__ __launch_bounds__(PY_DOWN_COLS* PY_DOWN_ROWS) void k_pyr_down(const uint8_t* __restrict__ src, int W, int H,
                                                                         uint8_t* __restrict__ dst) {
  const int col = blockIdx.x * PY_DOWN_COLS + (threadIdx.x & (PY_DOWN_COLS - 1));
  const int y = blockIdx.y * PY_DOWN_ROWS + (threadIdx.x / PY_DOWN_COLS);
  const int Wo = W >> 1, Ho = H >> 1;
  if (col * 8 >= W || y >= Ho) return;
  const size_t img = blockIdx.z;
  const uint8_t* s = src + img * (size_t)W * H + (size_t)(2 * y) * W + (size_t)col * 8;
  const uint2 a = *reinterpret_cast<const uint2*>(s);
  const uint2 b = *reinterpret_cast<const uint2*>(s + W);
  const uint32_t m = 0x00FF00FFu;
  const uint32_t s0 = ((a.x & m) + ((a.x >> 8) & m) + (b.x & m) + ((b.x >> 8) & m) + 0x00020002u) >> 2;
  const uint32_t s1 = ((a.y & m) + ((a.y >> 8) & m) + (b.y & m) + ((b.y >> 8) & m) + 0x00020002u) >> 2;
  // bytes 0, 2 of s0 then bytes 0, 2 of s1 (v_perm_b32: selectors 0 .. 3 take the second operand's bytes, 4 .. 7 the first's)
  const uint32_t o = __builtin_amdgcn_perm(s1, s0, 0x06040200u);
  *reinterpret_cast<uint32_t*>(dst + img * (size_t)Wo * Ho + (size_t)y * Wo + (size_t)col * 4) = o;
}

// Does the level-l block of source (x, y) -- level-0 pixels [x << l, (x << l) + 2^l) x [y << l, (y << l) + 2^l) -- hold a
// set bit?  (x, y) lies inside level l's image, so the block lies inside level 0's.
__device__ __forceinline__ bool py_block_hit(const uint32_t* __restrict__ plane, int wpr, int x, int y, int l) {
  const int n = 1 << l, x0 = x << l;
  const uint32_t mask = ((1u << n) - 1u) << (x0 & 31);  // (n <= 8, x0 a multiple of n: one word)
  const uint32_t* row = plane + (size_t)(y << l) * wpr + (x0 >> 5);
  uint32_t hit = 0;
  for (int j = 0; j < n; ++j) hit |= row[(size_t)j * wpr] & mask;
  return hit != 0;
}

// grid (nchunk, npairs).  rec: [npairs][cap] records of `stride` 32-bit words whose first two are the source (x, y).
// flags[p][i / 64] = the keep bits of records i .. i + 63 (every word of a pair's nchunk * 32 is written), blkcnt[p * nchunk
// + b] = records kept in chunk b.  A record whose source lies outside level l's image Wl x Hl has no block: it is kept and,
// later, marks nothing.
__global__ __launch_bounds__(PY_THREADS) void k_pyr_keep(const int32_t* __restrict__ rec, int stride, long cap,
                                                         const int32_t* __restrict__ cnt, int l, int Wl, int Hl,
                                                         const uint32_t* __restrict__ plane, int wpr, int H0,
                                                         unsigned long long* __restrict__ flags, int32_t* __restrict__ blkcnt,
                                                         int nchunk) {
  const int p = blockIdx.y;
  const long n = min(max((long)cnt[p], 0l), cap);
  const long i0 = (long)blockIdx.x * PY_CHUNK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* r = rec + (size_t)p * cap * stride;
  const uint32_t* pl = plane + (size_t)p * H0 * wpr;
  unsigned long long* fl = flags + ((size_t)p * nchunk + blockIdx.x) * (PY_CHUNK / 64);
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int kept = 0;
#pragma unroll 1
  for (int k = 0; k < PY_CHUNK / PY_THREADS; ++k) {
    const long i = i0 + k * PY_THREADS + threadIdx.x;
    bool keep = i < n;
    if (keep && l > 0) {
      const int x = r[i * stride], y = r[i * stride + 1];
      if (x >= 0 && x < Wl && y >= 0 && y < Hl) keep = !py_block_hit(pl, wpr, x, y, l);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) {
      fl[k * (PY_THREADS / 64) + wave] = m;
      kept += __popcll(m);
    }
  }
  if (lane == 0 && kept) atomicAdd(&s_n, kept);
  __syncthreads();
  if (threadIdx.x == 0) blkcnt[(size_t)p * nchunk + blockIdx.x] = s_n;
}

// One workgroup per pair: blkcnt[p][0 .. nchunk) becomes its exclusive scan behind the pair's total so far (total[p];
// first: 0), level_cnt[p] the level's kept count, total[p] the new total.
__global__ __launch_bounds__(1024) void k_pyr_scan(int32_t* __restrict__ blkcnt, int nchunk, int first,
                                                   int32_t* __restrict__ level_cnt, int32_t* __restrict__ total) {
  const int p = blockIdx.x;
  int32_t* a = blkcnt + (size_t)p * nchunk;
  __shared__ int s_w[16];
  __shared__ int s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int base = first ? 0 : total[p];
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nchunk; b0 += blockDim.x) {
    const int i = b0 + threadIdx.x;
    const int x = i < nchunk ? a[i] : 0;
    int incl = x;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
      if (w < wave) woff += s_w[w];
      tot += s_w[w];
    }
    const int carry = s_carry;
    if (i < nchunk) a[i] = base + carry + woff + incl - x;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    level_cnt[p] = s_carry;
    total[p] = base + s_carry;
  }
}

template <bool CORR>
struct PyRec;
template <>
struct PyRec<false> {  // gpc_support
  int32_t x, y;
  float d;
};
template <>
struct PyRec<true> {  // gpc_correspondence
  int32_t sx, sy, tx, ty;
};

__device__ __forceinline__ int py_src_x(const PyRec<false>& r) { return r.x; }
__device__ __forceinline__ int py_src_y(const PyRec<false>& r) { return r.y; }
__device__ __forceinline__ int py_src_x(const PyRec<true>& r) { return r.sx; }
__device__ __forceinline__ int py_src_y(const PyRec<true>& r) { return r.sy; }

// a level-l record in level 0's coordinates; (x, y): its mapped source pixel.  d * 2^l is exact in float.
__device__ __forceinline__ PyRec<false> py_map(PyRec<false> r, int l, int& x, int& y) {
  r.x <<= l;
  r.y <<= l;
  r.d *= (float)(1 << l);
  x = r.x;
  y = r.y;
  return r;
}
__device__ __forceinline__ PyRec<true> py_map(PyRec<true> r, int l, int& x, int& y) {
  r.sx <<= l;
  r.sy <<= l;
  r.tx <<= l;
  r.ty <<= l;
  x = r.sx;
  y = r.sy;
  return r;
}

// grid (nchunk, npairs): the kept records of chunk b of pair p, mapped, go to out[p][blkoff + their rank], those below cap;
// mark: their source pixels are set in the plane (no later level: nothing to mark)
template <bool CORR>
__global__ __launch_bounds__(PY_THREADS) void k_pyr_write(const PyRec<CORR>* __restrict__ rec, long cap_in, int l, int Wl, int Hl,
                                                          const unsigned long long* __restrict__ flags,
                                                          const int32_t* __restrict__ blkoff, int nchunk,
                                                          PyRec<CORR>* __restrict__ out, long cap, uint32_t* __restrict__ plane,
                                                          int wpr, int H0, int mark) {
  const int p = blockIdx.y;
  const long i0 = (long)blockIdx.x * PY_CHUNK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PyRec<CORR>* r = rec + (size_t)p * cap_in;
  PyRec<CORR>* o = out + (size_t)p * cap;
  uint32_t* pl = plane + (size_t)p * H0 * wpr;
  const unsigned long long* fl = flags + ((size_t)p * nchunk + blockIdx.x) * (PY_CHUNK / 64);
  long pos = blkoff[(size_t)p * nchunk + blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < PY_CHUNK / PY_THREADS; ++k) {
    int woff = 0, tot = 0;
    unsigned long long mine = 0;
#pragma unroll
    for (int w = 0; w < PY_THREADS / 64; ++w) {
      const unsigned long long m = fl[k * (PY_THREADS / 64) + w];
      const int c = __popcll(m);
      if (w < wave) woff += c;
      if (w == wave) mine = m;
      tot += c;
    }
    if ((mine >> lane) & 1ull) {
      const long at = pos + woff + __popcll(mine & ((1ull << lane) - 1ull));
      const PyRec<CORR> in = r[i0 + k * PY_THREADS + threadIdx.x];
      const int sx = py_src_x(in), sy = py_src_y(in);
      int x, y;
      const PyRec<CORR> q = py_map(in, l, x, y);
      if (at < cap) o[at] = q;
      // (inside level l's image, so inside the plane: a record from elsewhere marks nothing)
      if (mark && sx >= 0 && sx < Wl && sy >= 0 && sy < Hl) atomicOr(&pl[(size_t)y * wpr + (x >> 5)], 1u << (x & 31));
    }
    pos += tot;
  }
}

}  // namespace gpc
