// Stand-alone check of opengpc_amd/csrc/propagate_host.h (no HIP) against the C ABI's struct and constants: the parameter
// and size checks of the propagation, the aliasing rule of the output, the stride of every iteration for every (span,
// iterations) in range, and the plan of the ping-pong -- every iteration reads what the one before it wrote and never what it
// writes, the last one writes the caller's output, the caller's field is written only where it is the output.  Built plainly
// and with -fsanitize=address,undefined by tests/test_propagate_cpp.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "propagate_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_propagate def = {2, 1, 6, 8};
  EXPECT(sizeof(gpc_propagate) == 16 && PG_MAX_SPAN == 64 && PG_MAX_ITERATIONS == 16);
  EXPECT(pg_params(&def) == GPC_OK && pg_params(nullptr) == GPC_E_INVALID);
  const gpc_propagate bad[] = {{0, 4, 3, 4},         {5, 4, 3, 4},         {2, 0, 3, 4},         {2, 65, 3, 4},
                               {2, 4, 0, 4},         {2, 4, 17, 4},        {2, 4, 3, 0},         {2, 4, 3, 5},
                               {2, 4, 3, 6},         {2, 4, 3, 9},         {2, 4, 3, -4},        {2, 4, 3, 12},
                               {INT32_MIN, 4, 3, 4}, {2, INT32_MIN, 3, 4}, {2, 4, INT32_MIN, 4}, {2, 4, 3, INT32_MIN},
                               {INT32_MAX, 4, 3, 4}, {2, INT32_MAX, 3, 4}, {2, 4, INT32_MAX, 4}, {2, 4, 3, INT32_MAX}};
  for (const gpc_propagate& b : bad) EXPECT(pg_params(&b) == GPC_E_INVALID);
  const gpc_propagate edge[] = {{1, 1, 1, 4}, {4, 64, 16, 8}, {1, 64, 1, 8}, {4, 1, 16, 4}};
  for (const gpc_propagate& e : edge) EXPECT(pg_params(&e) == GPC_OK);

  EXPECT(pg_limits(1, 1, 1, 1) == GPC_OK && pg_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(pg_limits(0, 4, 4, 1) == GPC_E_INVALID && pg_limits(3, 4, 4, 1) == GPC_E_INVALID);
  EXPECT(pg_limits(1, 0, 4, 1) == GPC_E_INVALID && pg_limits(1, 4, -1, 1) == GPC_E_INVALID && pg_limits(1, 4, 4, 0) == GPC_E_INVALID);
  EXPECT(pg_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && pg_limits(1, 1, 32769, 1) == GPC_E_UNSUPPORTED);
  EXPECT(pg_limits(1, 0x7FFFFFFF, 0x7FFFFFFF, 1) == GPC_E_UNSUPPORTED && pg_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);

  // aliasing, on real arrays so that the addresses mean something
  std::vector<int32_t> f(64), o(64);
  std::vector<uint8_t> l(64), r(64);
  const uintptr_t pf = (uintptr_t)f.data(), po = (uintptr_t)o.data(), pl = (uintptr_t)l.data(), pr = (uintptr_t)r.data();
  EXPECT(pg_alias_ok(po, pf, 256, pl, pr, 64) && pg_alias_ok(pf, pf, 256, pl, pr, 64));           // apart, and in place
  EXPECT(!pg_alias_ok(pf + 4, pf, 256, pl, pr, 64) && !pg_alias_ok(pf + 252, pf, 256, pl, pr, 64));
  EXPECT(!pg_alias_ok(pf, pf + 4, 256, pl, pr, 64));
  EXPECT(!pg_alias_ok(pl, pf, 64, pl, pr, 64) && !pg_alias_ok(pr + 63, pf, 64, pl, pr, 64) && !pg_alias_ok(pl, pf, 64, pr, pl, 64));
  EXPECT(!pg_alias_ok(pf, pf, 256, pf + 8, pr, 64) && !pg_alias_ok(pf, pf, 256, pl, pf + 255, 64));  // in place over an image
  EXPECT(pg_alias_ok(pl, pf, 64, pl + 64, pr, 64));                                                 // end to end is no overlap

  // the stride schedule and the plan, for every (span, iterations) in range and both forms of the output
  for (int span = 1; span <= PG_MAX_SPAN; ++span)
    for (int N = 1; N <= PG_MAX_ITERATIONS; ++N) {
      int want = span;
      for (int i = 0; i < N; ++i) {
        EXPECT(pg_stride(span, i) == (want < 1 ? 1 : want) && pg_stride(span, i) >= 1 && pg_stride(span, i) <= span);
        if (i) EXPECT(pg_stride(span, i) <= pg_stride(span, i - 1));
        want >>= 1;
      }
      EXPECT(pg_stride(span, 7) == 1 && pg_stride(span, 31) == 1 && pg_stride(span, 40) == 1);
      for (int in_place = 0; in_place < 2; ++in_place) {
        bool ws_used = pg_copy_first(N, in_place);
        // what each block holds: -1 nothing, 0 the input, i + 1 the field of iteration i; with out == field one block is both
        int holds[3] = {0, in_place ? 0 : -1, pg_copy_first(N, in_place) ? 0 : -1};
        for (int i = 0; i < N; ++i) {
          const PgBlock s = pg_src(i, N, in_place), d = pg_dst(i, N);
          EXPECT(d != PG_FIELD);                                          // the caller's field is written only as out
          EXPECT(s != d && !(in_place && s + d == PG_FIELD + PG_OUT));    // never the block it reads
          EXPECT(holds[s] == i);                                          // it reads what iteration i-1 wrote (the input first)
          holds[d] = i + 1;
          if (in_place && d == PG_OUT) holds[PG_FIELD] = i + 1;
          ws_used = ws_used || s == PG_WS || d == PG_WS;
        }
        EXPECT(pg_dst(N - 1, N) == PG_OUT && holds[PG_OUT] == N);
        EXPECT(in_place || holds[PG_FIELD] == 0);
        EXPECT(ws_used == pg_needs_ws(N, in_place));
        EXPECT(pg_copy_first(N, in_place) == (in_place && N % 2 == 1));
      }
    }
  EXPECT(!pg_needs_ws(1, false) && pg_needs_ws(1, true) && pg_needs_ws(2, false) && pg_needs_ws(2, true));
  puts("ok");
  return 0;
}
