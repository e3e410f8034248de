// Stand-alone check of opengpc_amd/csrc/gapfill_host.h (no HIP) against the C ABI's struct and constants: the parameter and
// size checks of the scanline hole closing, the aliasing rule of the output, the bands of the column scan -- they cover every
// row once, and a band is never shorter than the look-back -- and the workspace size.  Built plainly and with
// -fsanitize=address,undefined by tests/test_gapfill_cpp.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gapfill_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_gapfill def = {64, 128, 0, 1};
  EXPECT(sizeof(gpc_gapfill) == 16 && GF_MAX_GAP == 32767 && GF_MAX_DISCON == (1 << 24));
  EXPECT(GF_NO_END == 0xFFFFu && GF_FAR == 0xFFFEu && 32768u < GF_FAR);  // a real distance (at most the image's extent) is no code
  EXPECT(gf_params(&def, false) == GPC_OK && gf_params(&def, true) == GPC_OK && gf_params(nullptr, true) == GPC_E_INVALID);
  const gpc_gapfill bad[] = {{0, 256, 0, 1},         {32768, 256, 0, 1},     {-1, 256, 0, 1},        {16, -1, 0, 1},
                             {16, (1 << 24) + 1, 0, 1}, {16, 256, 2, 1},     {16, 256, -1, 1},       {16, 256, 0, 2},
                             {16, 256, 0, -1},       {INT32_MIN, 256, 0, 1}, {16, INT32_MIN, 0, 1},  {16, 256, INT32_MIN, 1},
                             {16, 256, 0, INT32_MIN}, {INT32_MAX, 256, 0, 1}, {16, INT32_MAX, 0, 1}, {16, 256, INT32_MAX, 1},
                             {16, 256, 0, INT32_MAX}};
  for (const gpc_gapfill& b : bad) EXPECT(gf_params(&b, true) == GPC_E_INVALID);
  const gpc_gapfill edge[] = {{1, 0, 0, 0}, {32767, 1 << 24, 1, 1}, {1, 1 << 24, 0, 1}, {32767, 0, 1, 0}};
  for (const gpc_gapfill& e : edge) EXPECT(gf_params(&e, true) == GPC_OK);
  const gpc_gapfill guided = {16, 256, 1, 1};
  EXPECT(gf_params(&guided, true) == GPC_OK && gf_params(&guided, false) == GPC_E_INVALID);  // select = 1 needs the guide

  EXPECT(gf_limits(1, 1, 1, 1) == GPC_OK && gf_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(gf_limits(0, 4, 4, 1) == GPC_E_INVALID && gf_limits(3, 4, 4, 1) == GPC_E_INVALID);
  EXPECT(gf_limits(1, 0, 4, 1) == GPC_E_INVALID && gf_limits(1, 4, -1, 1) == GPC_E_INVALID && gf_limits(1, 4, 4, 0) == GPC_E_INVALID);
  EXPECT(gf_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && gf_limits(1, 1, 32769, 1) == GPC_E_UNSUPPORTED);
  EXPECT(gf_limits(1, 0x7FFFFFFF, 0x7FFFFFFF, 1) == GPC_E_UNSUPPORTED && gf_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);

  // aliasing, on real arrays so that the addresses mean something
  std::vector<int32_t> f(64), o(64);
  std::vector<uint8_t> g(64);
  const uintptr_t pf = (uintptr_t)f.data(), po = (uintptr_t)o.data(), pg = (uintptr_t)g.data();
  EXPECT(gf_alias_ok(po, pf, 256, pg, 64) && gf_alias_ok(pf, pf, 256, pg, 64));  // apart, and in place
  EXPECT(gf_alias_ok(po, pf, 256, 0, 64) && gf_alias_ok(pf, pf, 256, 0, 64));    // no guide
  EXPECT(!gf_alias_ok(pf + 4, pf, 256, pg, 64) && !gf_alias_ok(pf + 252, pf, 256, pg, 64) && !gf_alias_ok(pf, pf + 4, 256, pg, 64));
  EXPECT(!gf_alias_ok(pg, pf, 64, pg, 64) && !gf_alias_ok(pg + 63, pf, 64, pg, 64) && !gf_alias_ok(pf, pf, 256, pf + 255, 64));
  EXPECT(gf_alias_ok(pg, pf, 64, pg + 64, 64));                                   // end to end is no overlap

  // the bands: at least GF_BAND rows and at least the look-back, and together every row once
  for (int max_gap = 1; max_gap <= GF_MAX_GAP; max_gap = max_gap < 200 ? max_gap + 1 : max_gap * 2 + 1) {
    const int band = gf_band(max_gap);
    EXPECT(band >= GF_BAND && band >= max_gap && (band == GF_BAND || band == max_gap));
    for (int H : {1, 63, 64, 65, 67, 130, 436, 32768}) {
      const int nb = gf_bands(H, max_gap);
      EXPECT(nb >= 1 && (int64_t)(nb - 1) * band < H && (int64_t)nb * band >= H && nb <= 512);
    }
  }
  EXPECT(gf_band(GF_MAX_GAP) == GF_MAX_GAP && gf_bands(32768, GF_MAX_GAP) == 2 && gf_bands(32768, 1) == 512);

  EXPECT(gf_plane_pixels(1024, 436, 32) == (int64_t)1024 * 436 * 32 && gf_ws_bytes(1024, 436, 32) == (int64_t)8 * 1024 * 436 * 32);
  EXPECT(gf_ws_bytes(32768, 32768, 65535) == (int64_t)8 * 65535 * ((int64_t)1 << 30));  // no overflow at the limits
  puts("ok");
  return 0;
}
