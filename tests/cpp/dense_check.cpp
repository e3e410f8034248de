// Stand-alone check of opengpc_amd/csrc/dense_host.h (no HIP): the parameter and size checks of the densifier, Lmax, the
// geometry of the cell pyramid and the workspace sizes.  Built with -fsanitize=address,undefined by tests/test_dense.py;
// prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "dense_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_densify def = {15, 1, 1, 0xFFFF};
  EXPECT(sizeof(gpc_densify) == 16 && GPC_DENSE_NONE == INT32_MIN);
  EXPECT(dn_params(&def, false) == GPC_OK && dn_params(&def, true) == GPC_OK && dn_params(nullptr, true) == GPC_E_INVALID);
  const gpc_densify bad[] = {{0, 1, 1, 0xFFFF},  {16, 1, 1, 0xFFFF}, {15, 0, 1, 0xFFFF},  {15, 65537, 1, 0xFFFF}, {15, 1, 2, 0xFFFF},
                             {15, 1, -1, 0xFFFF}, {15, 1, 1, -1},     {15, 1, 1, 0x10000}, {-1, 1, 1, 0xFFFF}};
  for (const gpc_densify& b : bad) EXPECT(dn_params(&b, true) == GPC_E_INVALID);
  const gpc_densify edge[] = {{1, 1, 0, 0xFFFF}, {15, 65536, 1, 0xFFFF}};
  for (const gpc_densify& e : edge) EXPECT(dn_params(&e, false) == GPC_OK);
  const gpc_densify ceil0 = {15, 1, 1, 0}, ceil1 = {15, 1, 1, 0xFFFE};
  EXPECT(dn_params(&ceil0, true) == GPC_OK && dn_params(&ceil1, true) == GPC_OK);
  EXPECT(dn_params(&ceil0, false) == GPC_E_INVALID && dn_params(&ceil1, false) == GPC_E_INVALID);  // a ceiling needs ref

  EXPECT(dn_limits(1, 1, 1, 1) == GPC_OK && dn_limits(32768, 32768, 1, 1) == GPC_OK);
  EXPECT(dn_limits(0, 4, 1, 1) == GPC_E_INVALID && dn_limits(4, -1, 1, 1) == GPC_E_INVALID);
  EXPECT(dn_limits(4, 4, 0, 1) == GPC_E_INVALID && dn_limits(4, 4, 1, 0) == GPC_E_INVALID);
  EXPECT(dn_limits(32769, 1, 1, 1) == GPC_E_UNSUPPORTED && dn_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED);
  EXPECT(dn_limits(0x7FFFFFFF, 0x7FFFFFFF, 1, 1) == GPC_E_UNSUPPORTED);  // (no overflow on the way)
  EXPECT(dn_limits(4, 4, 65535, 1) == GPC_OK && dn_limits(4, 4, 65536, 1) == GPC_E_UNSUPPORTED);
  EXPECT(dn_limits(4, 4, 2048, 1 << 20) == GPC_E_UNSUPPORTED && dn_limits(4, 4, 1, 0x7FFFFFFF) == GPC_OK);
  EXPECT(dn_limits(4, 4, 2, 0x7FFFFFFF) == GPC_E_UNSUPPORTED);

  EXPECT(dn_lmax(1, 1) == 1 && dn_lmax(2, 2) == 1 && dn_lmax(3, 1) == 2 && dn_lmax(7, 5) == 3 && dn_lmax(33, 17) == 6);
  EXPECT(dn_lmax(96, 64) == 7 && dn_lmax(128, 128) == 7 && dn_lmax(129, 2) == 8 && dn_lmax(1024, 436) == 10);
  EXPECT(dn_lmax(1920, 1080) == 11 && dn_lmax(32768, 32768) == 15 && dn_lmax(1, 32768) == 15);

  // a geometry on the heap: a write behind it is the sanitizer's to find
  std::unique_ptr<DnGeom> g(new DnGeom(dn_geom(33, 17, def)));
  EXPECT(g->top == 6 && g->W == 33 && g->H == 17 && g->min_count == 1 && g->spread == 1);
  const int gw[7] = {0, 17, 9, 5, 3, 2, 1}, gh[7] = {0, 9, 5, 3, 2, 1, 1};
  int at = 0;
  for (int l = 1; l <= 6; ++l) {
    EXPECT(g->gw[l] == gw[l] && g->gh[l] == gh[l] && g->off[l] == at);
    at += gw[l] * gh[l];
  }
  EXPECT(g->off[7] == at && dn_cells(*g) == at);
  const gpc_densify shallow = {3, 2, 0, 0xFFFF};
  *g = dn_geom(200, 90, shallow);
  EXPECT(g->top == 3 && g->min_count == 2 && g->spread == 0 && dn_cells(*g) == 100 * 45 + 50 * 23 + 25 * 12);
  *g = dn_geom(1, 1, def);
  EXPECT(g->top == 1 && g->gw[1] == 1 && g->gh[1] == 1 && dn_cells(*g) == 1);
  *g = dn_geom(32768, 32768, def);
  EXPECT(g->top == 15 && g->gw[15] == 1 && g->gw[1] == 16384 && dn_cells(*g) == ((int64_t)1 << 30) / 3);
  *g = dn_geom(32768, 1, def);
  EXPECT(g->top == 15 && dn_cells(*g) == 32767);
  // bytes per pixel: 4 for the owners, at most (4 + 8 C) / 3 + 1 for the cells
  *g = dn_geom(1024, 436, def);
  const int64_t px = 1024 * 436;
  EXPECT(dn_owner_bytes(1024, 436, 3) == 12 * px);
  EXPECT(dn_count_bytes(*g, 1) + dn_sum_bytes(*g, 1, 1) <= px * 5 && dn_count_bytes(*g, 1) + dn_sum_bytes(*g, 1, 2) <= px * 23 / 3);
  EXPECT(dn_sum_bytes(*g, 2, 2) == 4 * dn_sum_bytes(*g, 1, 1) && dn_count_bytes(*g, 7) == 28 * dn_cells(*g));
  puts("ok");
  return 0;
}
