// propagate_host.h -- the host-side part of the propagation of field values between neighbours (gpc_hip_propagate_*) that
// needs no HIP: the parameters, the size limits, the aliasing rule of the output, the stride of an iteration and the plan of
// the ping-pong -- which block an iteration reads and which it writes, so that the last one lands in the caller's output for
// every parity of N and for out == field.  Plain C++ so that a stand-alone program can drive it under the sanitizers
// (tests/cpp/propagate_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"
#include "search_host.h"

#define PG_MAX_SPAN 64
#define PG_MAX_ITERATIONS 16

namespace gpc {

inline int pg_params(const gpc_propagate* p) {
  if (!p) return GPC_E_INVALID;
  if (p->radius < 1 || p->radius > SR_MAX_RADIUS) return GPC_E_INVALID;
  if (p->span < 1 || p->span > PG_MAX_SPAN) return GPC_E_INVALID;
  if (p->iterations < 1 || p->iterations > PG_MAX_ITERATIONS) return GPC_E_INVALID;
  if (p->neighbours != 4 && p->neighbours != 8) return GPC_E_INVALID;
  return GPC_OK;
}

// the limits of the densify block, as the search has them
inline int pg_limits(int channels, int W, int H, int npairs) { return sr_limits(channels, W, H, npairs); }

// the search's rule: out may be the field itself; any other byte shared with the field or with an image is refused
inline bool pg_alias_ok(uintptr_t out, uintptr_t field, int64_t field_bytes, uintptr_t imgL, uintptr_t imgR, int64_t img_bytes) {
  return sr_alias_ok(out, field, field_bytes, imgL, imgR, img_bytes);
}

// s_i = max(1, span >> i)
inline int pg_stride(int span, int i) {
  const int s = i < 31 ? span >> i : 0;
  return s < 1 ? 1 : s;
}

// The blocks an iteration may read or write: the caller's field, the caller's output, the context's workspace.
enum PgBlock { PG_FIELD = 0, PG_OUT = 1, PG_WS = 2 };

// Iteration N-1 writes out, and the iterations before it alternate backwards from there.
inline PgBlock pg_dst(int i, int N) { return ((N - 1 - i) & 1) ? PG_WS : PG_OUT; }
// With out == field and an odd N iteration 0 would write what it reads: the field is copied into the workspace first.
inline bool pg_copy_first(int N, bool in_place) { return in_place && (N & 1); }
inline PgBlock pg_src(int i, int N, bool in_place) {
  if (i > 0) return pg_dst(i - 1, N);
  return pg_copy_first(N, in_place) ? PG_WS : PG_FIELD;
}
// whether the call needs the workspace at all (one field's bytes)
inline bool pg_needs_ws(int N, bool in_place) { return N >= 2 || pg_copy_first(N, in_place); }

}  // namespace gpc
