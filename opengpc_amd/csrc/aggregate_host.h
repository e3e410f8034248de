// aggregate_host.h -- the host-side checks and the geometry of the scanline aggregation (gpc_hip_aggregate_*) that need no
// HIP: the parameters, the numbers of labels and of stored cost cells, the chunk a horizontal path stages, the bytes of
// workspace a pair takes and the pairs that go through the launches together.  Plain C++ so that a stand-alone program can
// drive it under the sanitizers (tests/cpp/aggregate_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "search_host.h"

#define AG_LANES 64                              // chains per workgroup: one wave, one lane per column (vertical) or row (horizontal)
#define AG_CHOOSE_THREADS 256                    // pixels per workgroup of the choice
#define AG_GROUP_BYTES ((int64_t)1 << 30)        // what the cost and path volumes of one group of pairs may take
#define AG_NONE 0xFFFFu                          // the mark of a cell that is no candidate's cost, and of a path value nobody reads
#define AG_MAX_COST (81 * 255)                   // the largest SAD (radius 4)
#define AG_MAX_PENALTY 32767

namespace gpc {

inline int ag_params(const gpc_aggregate* p) {
  if (!p) return GPC_E_INVALID;
  const gpc_search s = {p->radius, p->range, p->subpixel, p->max_cost};
  if (sr_params(&s) != GPC_OK) return GPC_E_INVALID;
  if (p->p1 < 0 || p->p2 < p->p1 || p->p2 > AG_MAX_PENALTY) return GPC_E_INVALID;
  if (p->paths < 0 || p->paths > 15) return GPC_E_INVALID;
  return GPC_OK;
}

inline int ag_labels(int channels, int range) { return channels == 2 ? (2 * range + 1) * (2 * range + 1) : 2 * range + 1; }
// the cells of the cost volume: the labels and the ring of one more shift around them, which the parabola reads
inline int ag_cells(int channels, int range) { return channels == 2 ? (2 * range + 3) * (2 * range + 3) : 2 * range + 3; }
inline int ag_dirs(int paths) { return (paths & 1) + (paths >> 1 & 1) + (paths >> 2 & 1) + (paths >> 3 & 1); }
// the columns a horizontal path stages at a time: what keeps the tile, the bases and the gather slots within 64 KB of LDS
inline int ag_chunk(int labels) { return labels > 9 ? 8 : labels > 5 ? 16 : 32; }

// bytes of workspace per pixel: 2 per cost cell and 2 per label and direction
inline int64_t ag_pixel_bytes(int channels, int range, int paths) {
  return 2 * ((int64_t)ag_cells(channels, range) + (int64_t)ag_dirs(paths) * ag_labels(channels, range));
}

// pairs that go through the launches together: what `budget` bytes hold, at least one, at most all
inline int ag_group(int channels, int W, int H, int npairs, int range, int paths, int64_t budget) {
  const int64_t per_pair = ag_pixel_bytes(channels, range, paths) * W * H;
  int64_t g = budget / per_pair;
  if (g < 1) g = 1;
  return g > npairs ? npairs : (int)g;
}

// the largest path value: a cost and the largest penalty
inline uint32_t ag_max_path() { return AG_MAX_COST + AG_MAX_PENALTY; }

inline int ag_blocks(int extent) { return (extent + AG_LANES - 1) / AG_LANES; }

}  // namespace gpc
