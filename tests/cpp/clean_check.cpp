// Stand-alone check of opengpc_amd/csrc/clean_host.h (no HIP): the parameter and size checks of the field cleaner, the
// overlap test, the tile geometry and the workspace sizes.  Built with -fsanitize=address,undefined by tests/test_clean.py;
// prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "clean_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_clean def = {256, 256, 64, 1};
  EXPECT(sizeof(gpc_clean) == 16 && CL_TILE == 32);
  EXPECT(cl_params(&def, true) == GPC_OK && cl_params(&def, false) == GPC_E_INVALID && cl_params(nullptr, true) == GPC_E_INVALID);
  const gpc_clean bad[] = {{-2, 256, 64, 1},      {(1 << 24) + 1, 256, 64, 1}, {256, -1, 64, 1},  {256, (1 << 24) + 1, 64, 1},
                           {256, 256, -1, 1},     {256, 256, (1 << 30) + 1, 1}, {256, 256, 64, -1}, {256, 256, 64, 3},
                           {INT32_MIN, 0, 0, 0},  {0, INT32_MAX, 0, 0},         {0, 0, INT32_MAX, 0}, {0, 0, 0, INT32_MAX}};
  for (const gpc_clean& b : bad) EXPECT(cl_params(&b, true) == GPC_E_INVALID);
  const gpc_clean edge[] = {{0, 0, 0, 0}, {1 << 24, 1 << 24, 1 << 30, 2}, {-1, 0, 1, 0}};
  for (const gpc_clean& e : edge) EXPECT(cl_params(&e, true) == GPC_OK);
  const gpc_clean nocheck = {-1, 256, 64, 1};
  EXPECT(cl_params(&nocheck, false) == GPC_OK);  // only the check needs bwd

  EXPECT(cl_limits(1, 1, 1, 1) == GPC_OK && cl_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(cl_limits(0, 4, 4, 1) == GPC_E_INVALID && cl_limits(3, 4, 4, 1) == GPC_E_INVALID);
  EXPECT(cl_limits(1, 0, 4, 1) == GPC_E_INVALID && cl_limits(1, 4, -1, 1) == GPC_E_INVALID && cl_limits(1, 4, 4, 0) == GPC_E_INVALID);
  EXPECT(cl_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && cl_limits(1, 1, 32769, 1) == GPC_E_UNSUPPORTED);
  EXPECT(cl_limits(1, 0x7FFFFFFF, 0x7FFFFFFF, 1) == GPC_E_UNSUPPORTED);  // (no overflow on the way)
  EXPECT(cl_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);

  // overlap, on a real array so that the addresses mean something
  std::vector<int32_t> a(64);
  const uintptr_t p = (uintptr_t)a.data();
  EXPECT(cl_overlap(p, 64, p, 64) && cl_overlap(p, 64, p + 63, 64) && cl_overlap(p + 63, 64, p, 64));
  EXPECT(!cl_overlap(p, 64, p + 64, 64) && !cl_overlap(p + 64, 64, p, 64));
  EXPECT(!cl_overlap(p, 64, 0, 64) && !cl_overlap(0, 64, p, 64) && !cl_overlap(p, 0, p, 64));
  EXPECT(cl_overlap(p + 8, 8, p, 256) && cl_overlap(p, 256, p + 8, 8));

  EXPECT(cl_tiles(1) == 1 && cl_tiles(32) == 1 && cl_tiles(33) == 2 && cl_tiles(200) == 7 && cl_tiles(32768) == 1024);
  EXPECT(cl_border_pixels(1, 1) == 0 && cl_border_pixels(32, 32) == 0 && cl_border_pixels(33, 17) == 17);
  EXPECT(cl_border_pixels(200, 90) == 6 * 90 + 2 * 200 && cl_border_pixels(1, 40) == 1 && cl_border_pixels(40, 1) == 1);
  EXPECT(cl_border_pixels(32768, 32768) == (int64_t)2 * 1023 * 32768);   // (a lane index fits an int)
  EXPECT(cl_field_bytes(2, 1024, 436, 16) == (int64_t)4 * 2 * 1024 * 436 * 16);
  EXPECT(cl_field_bytes(2, 32768, 32768, 65535) == (int64_t)8 * 65535 * ((int64_t)1 << 30));
  EXPECT(cl_label_bytes(200, 90, 3) == 4 * 200 * 90 * 3 && cl_size_bytes(200, 90, 3) == cl_label_bytes(200, 90, 3));

  std::unique_ptr<gpc_clean> q(new gpc_clean(def));
  EXPECT(cl_labels_needed(*q, false) && cl_labels_needed(*q, true));
  q->speckle_min = 1;
  EXPECT(!cl_labels_needed(*q, false) && cl_labels_needed(*q, true));
  q->speckle_min = 0;
  EXPECT(!cl_labels_needed(*q, false));
  puts("ok");
  return 0;
}
