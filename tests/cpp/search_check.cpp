// Stand-alone check of opengpc_amd/csrc/search_host.h (no HIP) against the C ABI's struct and constants: the parameter and
// size checks of the local dense search, the aliasing rule of the output against the field and the images, the rounding of
// a field value at the ends of int32, the tile geometry.  Built plainly and with -fsanitize=address,undefined by
// tests/test_search_cpp.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "search_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_search def = {2, 1, 1, 0xFFFF};
  EXPECT(sizeof(gpc_search) == 16 && SR_TILE_W == 32 && SR_TILE_H == 8 && SR_MAX_RADIUS == 4 && SR_MAX_RANGE == 2);
  EXPECT(2 * SR_MAX_RADIUS + 1 + 2 * (SR_MAX_RANGE + 1) <= 15);  // a target row with all its shifts: one 16-byte load
  EXPECT(sr_params(&def) == GPC_OK && sr_params(nullptr) == GPC_E_INVALID);
  const gpc_search bad[] = {{0, 1, 1, 0xFFFF},  {5, 1, 1, 0xFFFF},        {2, -1, 1, 0xFFFF},       {2, 3, 1, 0xFFFF},
                            {2, 1, -1, 0xFFFF}, {2, 1, 2, 0xFFFF},        {2, 1, 1, -1},            {2, 1, 1, 0x10000},
                            {INT32_MIN, 0, 0, 0}, {1, INT32_MAX, 0, 0},   {1, 0, INT32_MAX, 0},     {1, 0, 0, INT32_MAX},
                            {INT32_MAX, 0, 0, 0}, {1, INT32_MIN, 0, 0},   {1, 0, INT32_MIN, 0},     {1, 0, 0, INT32_MIN}};
  for (const gpc_search& b : bad) EXPECT(sr_params(&b) == GPC_E_INVALID);
  const gpc_search edge[] = {{1, 0, 0, 0}, {4, 2, 1, 0xFFFF}, {1, 2, 0, 20655}, {4, 0, 1, 1}};
  for (const gpc_search& e : edge) EXPECT(sr_params(&e) == GPC_OK);

  EXPECT(sr_limits(1, 1, 1, 1) == GPC_OK && sr_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(sr_limits(0, 4, 4, 1) == GPC_E_INVALID && sr_limits(3, 4, 4, 1) == GPC_E_INVALID);
  EXPECT(sr_limits(1, 0, 4, 1) == GPC_E_INVALID && sr_limits(1, 4, -1, 1) == GPC_E_INVALID && sr_limits(1, 4, 4, 0) == GPC_E_INVALID);
  EXPECT(sr_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && sr_limits(1, 1, 32769, 1) == GPC_E_UNSUPPORTED);
  EXPECT(sr_limits(1, 0x7FFFFFFF, 0x7FFFFFFF, 1) == GPC_E_UNSUPPORTED && sr_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);

  // aliasing, on real arrays so that the addresses mean something
  std::vector<int32_t> f(64), o(64);
  std::vector<uint8_t> l(64), r(64);
  const uintptr_t pf = (uintptr_t)f.data(), po = (uintptr_t)o.data(), pl = (uintptr_t)l.data(), pr = (uintptr_t)r.data();
  EXPECT(sr_alias_ok(po, pf, 256, pl, pr, 64) && sr_alias_ok(pf, pf, 256, pl, pr, 64));           // apart, and in place
  EXPECT(!sr_alias_ok(pf + 4, pf, 256, pl, pr, 64) && !sr_alias_ok(pf + 252, pf, 256, pl, pr, 64));
  EXPECT(!sr_alias_ok(pf, pf + 4, 256, pl, pr, 64));
  EXPECT(!sr_alias_ok(pl, pf, 64, pl, pr, 64) && !sr_alias_ok(pr + 63, pf, 64, pl, pr, 64) && !sr_alias_ok(pl, pf, 64, pr, pl, 64));
  EXPECT(!sr_alias_ok(pf, pf, 256, pf + 8, pr, 64) && !sr_alias_ok(pf, pf, 256, pl, pf + 255, 64));  // in place over an image
  EXPECT(sr_alias_ok(pl, pf, 64, pl + 64, pr, 64));                                                 // end to end is no overlap

  // the cleaner's rounding at the ends of int32 and around the halves
  EXPECT(sr_round(0) == 0 && sr_round(127) == 0 && sr_round(128) == 1 && sr_round(-127) == 0 && sr_round(-128) == -1);
  EXPECT(sr_round(383) == 1 && sr_round(384) == 2 && sr_round(-383) == -1 && sr_round(-384) == -2);
  EXPECT(sr_round(INT32_MAX) == (1 << 23) && sr_round(INT32_MIN + 1) == -(1 << 23) && sr_round(INT32_MIN) == -(1 << 23));
  const std::unique_ptr<int32_t> v(new int32_t(INT32_MAX - 127));
  EXPECT(sr_round(*v) == (1 << 23) && sr_round(*v - 1) == (1 << 23) - 1);

  EXPECT(sr_tiles_x(1) == 1 && sr_tiles_x(32) == 1 && sr_tiles_x(33) == 2 && sr_tiles_x(32768) == 1024);
  EXPECT(sr_tiles_y(1) == 1 && sr_tiles_y(8) == 1 && sr_tiles_y(9) == 2 && sr_tiles_y(32768) == 4096);
  puts("ok");
  return 0;
}
