// Stand-alone check of opengpc_amd/csrc/pyramid_host.h (no HIP): the geometry of the levels, the settings and the capacity
// of a level, the argument checks of the downsampling step and of the merge.  Built with -fsanitize=address,undefined by
// tests/test_pyramid.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pyramid_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  // heap arrays of exactly `levels` entries: a write behind them is the sanitizer's to find
  for (int levels = 1; levels <= GPC_MAX_PYRAMID_LEVELS; ++levels) {
    std::vector<int32_t> w(levels), h(levels);
    EXPECT(pyr_levels(1024, 436, levels, w.data(), h.data()) == GPC_OK);
    for (int l = 0; l < levels; ++l) EXPECT(w[l] == 1024 >> l && h[l] == 436 >> l);
  }
  int32_t w[4], h[4];
  EXPECT(pyr_levels(1024, 436, 3, w, h) == GPC_OK && w[2] == 256 && h[2] == 109);
  EXPECT(pyr_levels(1920, 1080, 3, w, h) == GPC_OK && w[2] == 480 && h[2] == 270);
  EXPECT(pyr_levels(256, 102, 2, w, h) == GPC_OK && h[1] == 51);
  EXPECT(pyr_levels(320, 163, 2, w, h) == GPC_OK && h[1] == 81);          // an odd last row is dropped
  EXPECT(pyr_levels(192, 120, 3, w, h) == GPC_OK && w[2] == 48 && h[2] == 30);
  EXPECT(pyr_levels(192, 120, 3, nullptr, nullptr) == GPC_OK);
  EXPECT(pyr_levels(192, 119, 3, w, h) == GPC_E_INVALID);                  // level 2 would be 29 rows
  EXPECT(pyr_levels(128, 120, 3, w, h) == GPC_E_INVALID);                  // level 2 would be 32 px wide
  EXPECT(pyr_levels(160, 100, 3, w, h) == GPC_E_INVALID);                  // 40 x 25
  EXPECT(pyr_levels(160, 100, 1, w, h) == GPC_OK);
  EXPECT(pyr_levels(224, 200, 3, w, h) == GPC_E_INVALID);                  // W % 64 != 0
  EXPECT(pyr_levels(224, 200, 2, w, h) == GPC_OK);
  EXPECT(pyr_levels(384, 240, 4, w, h) == GPC_OK && w[3] == 48 && h[3] == 30);
  EXPECT(pyr_levels(384, 240, 0, w, h) == GPC_E_INVALID && pyr_levels(384, 240, 5, w, h) == GPC_E_INVALID);
  EXPECT(pyr_levels(384, 240, -1, w, h) == GPC_E_INVALID);
  EXPECT(pyr_levels(0, 240, 1, w, h) == GPC_E_INVALID && pyr_levels(384, -3, 1, w, h) == GPC_E_INVALID);
  EXPECT(pyr_levels(16400, 64, 1, w, h) == GPC_E_UNSUPPORTED);
  EXPECT(pyr_levels(16384, 65536, 1, w, h) == GPC_OK && pyr_levels(16384, 65537, 1, w, h) == GPC_E_UNSUPPORTED);
  EXPECT(pyr_levels(0x7FFFFFF0, 0x7FFFFFFF, 4, w, h) == GPC_E_UNSUPPORTED);  // (no overflow on the way)

  gpc_settings s = {10, 128, 1, 1, 0, 3};
  for (int l = 0; l < 4; ++l) {
    const gpc_settings t = pyr_level_settings(s, l);
    EXPECT(t.disp_high == 128 >> l && t.vertical_tolerance == (1 >> l) && t.gradient_threshold == 10);
    EXPECT(t.epipolar_mode == 1 && t.use_hashtable == 0 && t.num_threads == 3);
    EXPECT((t.disp_high << l) <= s.disp_high && (t.vertical_tolerance << l) <= s.vertical_tolerance);
  }
  s.disp_high = 5;
  EXPECT(pyr_level_settings(s, 3).disp_high == 0);

  EXPECT(pyr_level_cap(48, 30) == 22 * 4 + 1 && pyr_level_cap(1024, 436) == 998 * 410 + 1);
  EXPECT(pyr_level_cap(16384, 65536) == (int64_t)16358 * 65510 + 1);

  alignas(16) static unsigned char buf[64];
  EXPECT(pyr_down_check(buf, buf + 32, 32, 2, 1) == GPC_OK);
  EXPECT(pyr_down_check(buf, buf + 32, 16, 2, 1) == GPC_E_INVALID);     // width % 32
  EXPECT(pyr_down_check(buf, buf + 32, 32, 1, 1) == GPC_E_INVALID);
  EXPECT(pyr_down_check(buf, buf + 32, 32, 2, 0) == GPC_E_INVALID);
  EXPECT(pyr_down_check(nullptr, buf, 32, 2, 1) == GPC_E_INVALID && pyr_down_check(buf, nullptr, 32, 2, 1) == GPC_E_INVALID);
  EXPECT(pyr_down_check(buf + 4, buf + 32, 32, 2, 1) == GPC_E_INVALID);  // the source is read 8 bytes at a time
  EXPECT(pyr_down_check(buf, buf + 34, 32, 2, 1) == GPC_E_INVALID);
  EXPECT(pyr_down_check(buf, buf + 36, 32, 2, 1) == GPC_OK);
  EXPECT(pyr_down_check(buf, buf + 32, 32, 2, 65536) == GPC_E_UNSUPPORTED);
  EXPECT(pyr_down_check(buf, buf + 32, 16384, 4, 1) == GPC_OK);

  const int32_t caps[4] = {5, 1, 7, 2}, bad[4] = {5, 0, 7, 2};
  EXPECT(pyr_merge_check(64, 40, 3, 4, caps, 9) == GPC_OK);
  EXPECT(pyr_merge_check(64, 40, 3, 4, bad, 9) == GPC_E_INVALID && pyr_merge_check(64, 40, 3, 1, bad, 9) == GPC_OK);
  EXPECT(pyr_merge_check(64, 40, 3, 5, caps, 9) == GPC_E_INVALID && pyr_merge_check(64, 40, 3, 0, caps, 9) == GPC_E_INVALID);
  EXPECT(pyr_merge_check(64, 40, 0, 2, caps, 9) == GPC_E_INVALID && pyr_merge_check(64, 40, 3, 2, caps, 0) == GPC_E_INVALID);
  EXPECT(pyr_merge_check(64, 40, 3, 2, nullptr, 9) == GPC_E_INVALID && pyr_merge_check(0, 40, 3, 2, caps, 9) == GPC_E_INVALID);
  EXPECT(pyr_merge_check(64, 40, 65536, 2, caps, 9) == GPC_E_UNSUPPORTED);
  EXPECT(pyr_merge_check(65536, 32768, 1, 2, caps, 9) == GPC_E_UNSUPPORTED);
  puts("ok");
  return 0;
}
