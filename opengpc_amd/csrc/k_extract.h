// k_extract.h -- training-set EXTRACTION: smoothed frames -> the device layout of k_train.h, and back.
//
// Replaces the patch cutting of Feature::extractAllTriplets (Feature.hpp:191-245: getPatch(.., x, y, 27) of the smoothed
// left image at the reference point, of the smoothed right image at the positive and the negative point) and the
// repacking gpc_hip_train_set_create does after it (k_ts_transpose): the patches go from the smoothed frames straight into
// planes[patch][byte][triplet] (k_train.h), so the training set never exists as host objects.
//
// Patch byte order (Buffer::getPatch, buffer.hpp:534-544): byte 27 * ix + iy is pixel (x + ix - 13, y + iy - 13), i.e. a
// patch ROW follows the image X offset.
//
// The host (gpc_hip.hip) works through the frames in chunks and hands every chunk's kernel a list of COLUMN GROUPS: four
// consecutive triplet columns 4q .. 4q+3 of the set and, for each of them and each patch, where the patch's top-left
// pixel lies in the chunk's smoothed frames -- or EX_KEEP (the column's triplet comes from another chunk: its byte is
// left as it is) or EX_ZERO (a padding column past the last triplet).  A group occurs at most once per chunk, so one
// launch never writes a dword twice; chunks run in stream order, so a column of an earlier chunk is in place when a later
// chunk merges its own bytes into the same dword.  Without a permutation a chunk's columns are one contiguous range and
// only the dwords at its two ends are merged; with one, most groups hold one column of the chunk.
#pragma once
#include "gpc_device.h"
#include "k_train.h"

namespace gpc {

#define EX_KEEP (-1)
#define EX_ZERO (-2)
#define EX_GROUPS 16  // column groups per workgroup: 64 triplet columns

struct ExGroup {
  int32_t q;        // the group's columns are 4q .. 4q+3
  int32_t off[12];  // off[4 * patch + b]: top-left pixel of column 4q+b's patch in the chunk's smooth frames, or EX_KEEP / EX_ZERO
};

// grid: (ceil(ngroups / 16), 3 patches, 3 thirds of the 729 bytes: ix in [9z, 9z + 9)), 256 threads.
// Phase 1 stages the workgroup's 64 columns x 243 bytes in LDS, transposed (s[byte][column]); neighbouring lanes read
// neighbouring pixels of one patch row (9 of them per row).  Phase 2 writes each plane row as dwords of four columns:
// sixteen lanes cover the 64 columns of one row -- 64 contiguous bytes when the groups are consecutive.
__global__ __launch_bounds__(TS_THREADS) void k_extract_gather(const uint8_t* __restrict__ smooth, int W,
                                                               const ExGroup* __restrict__ groups, int ngroups, long np,
                                                               uint8_t* __restrict__ planes) {
  __shared__ uint32_t s[243][17];  // [byte][column / 4]: 68-byte rows (17 dwords, odd: the byte stores of phase 1 spread over the banks)
  __shared__ int32_t s_off[4 * EX_GROUPS];
  __shared__ int32_t s_q[EX_GROUPS];
  const int tid = threadIdx.x, patch = blockIdx.y, z = blockIdx.z;
  const int g0 = blockIdx.x * EX_GROUPS;
  if (tid < 4 * EX_GROUPS) {
    const int g = g0 + tid / 4;
    s_off[tid] = g < ngroups ? groups[g].off[4 * patch + (tid & 3)] : EX_KEEP;
  }
  if (tid < EX_GROUPS) s_q[tid] = (g0 + tid) < ngroups ? groups[g0 + tid].q : -1;
  __syncthreads();
  uint8_t* sb = reinterpret_cast<uint8_t*>(&s[0][0]);
  for (int e = tid; e < 64 * 243; e += TS_THREADS) {
    const int tt = e / 243, k = e - tt * 243;  // column, then (patch row iy, x offset ixl within this third)
    const int iy = k / 9, ixl = k - iy * 9;
    const int off = s_off[tt];
    uint8_t v = 0;
    if (off >= 0) v = smooth[(long)off + (long)iy * W + 9 * z + ixl];
    sb[(27 * ixl + iy) * 68 + tt] = v;
  }
  __syncthreads();
  for (int e = tid; e < 243 * EX_GROUPS; e += TS_THREADS) {
    const int c = e >> 4, gi = e & 15;
    const int q = s_q[gi];
    if (q < 0) continue;
    uint32_t w = s[c][gi];
    uint32_t keep = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (s_off[4 * gi + b] == EX_KEEP) keep |= 0xFFu << (8 * b);
    uint32_t* dst = reinterpret_cast<uint32_t*>(planes + ((long)patch * TS_PATCH + 243 * z + c) * np + 4l * q);
    if (keep) w = (w & ~keep) | (*dst & keep);
    *dst = w;
  }
}

// The inverse of k_ts_transpose: triplets [first, first + n) of planes [3][729][np] -> aos [n][3][729] (file order of
// Feature::storeAllTriplets).  grid: (ceil(n / 64), 3, 3), 256 threads; aos may be the device's view of page-locked host memory.
__global__ __launch_bounds__(TS_THREADS) void k_ts_read(const uint8_t* __restrict__ planes, long np, int first, int n,
                                                        uint8_t* __restrict__ aos) {
  __shared__ uint8_t s[64][244];
  const int t0 = blockIdx.x * 64, patch = blockIdx.y, c0 = blockIdx.z * 243;
  for (int e = threadIdx.x; e < 64 * 243; e += TS_THREADS) {
    const int c = e >> 6, tt = e & 63;
    if (t0 + tt < n) s[tt][c] = planes[((long)patch * TS_PATCH + c0 + c) * np + first + t0 + tt];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 243; e += TS_THREADS) {
    const int tt = e / 243, c = e - tt * 243;
    if (t0 + tt < n) aos[((long)(t0 + tt) * 3 + patch) * TS_PATCH + c0 + c] = s[tt][c];
  }
}

}  // namespace gpc
