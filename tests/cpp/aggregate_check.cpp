// Stand-alone check of opengpc_amd/csrc/aggregate_host.h (no HIP) against the C ABI's struct and constants: the parameter
// checks of the scanline aggregation, the numbers of labels, cells and directions, the chunk of a horizontal path, the bytes
// of workspace a pixel takes and the grouping of pairs under a budget.  Built plainly and with -fsanitize=address,undefined
// by tests/test_aggregate_cpp.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "aggregate_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace gpc;
  const gpc_aggregate def = {2, 1, 1, 0xFFFF, 128, 512, 15};
  EXPECT(sizeof(gpc_aggregate) == 28 && AG_LANES == 64 && AG_MAX_COST == 20655 && AG_MAX_PENALTY == 32767);
  EXPECT(ag_max_path() == 53422 && ag_max_path() < AG_NONE && 4 * ag_max_path() < (1u << 18));
  EXPECT(ag_params(&def) == GPC_OK && ag_params(nullptr) == GPC_E_INVALID);
  const gpc_aggregate bad[] = {{0, 1, 1, 0xFFFF, 8, 32, 15},  {5, 1, 1, 0xFFFF, 8, 32, 15}, {2, -1, 1, 0xFFFF, 8, 32, 15},
                               {2, 3, 1, 0xFFFF, 8, 32, 15},  {2, 1, 2, 0xFFFF, 8, 32, 15}, {2, 1, 1, 0x10000, 8, 32, 15},
                               {2, 1, 1, 0xFFFF, -1, 32, 15}, {2, 1, 1, 0xFFFF, 33, 32, 15}, {2, 1, 1, 0xFFFF, 8, 32768, 15},
                               {2, 1, 1, 0xFFFF, 8, 32, -1},  {2, 1, 1, 0xFFFF, 8, 32, 16},  {2, 1, 1, 0xFFFF, INT32_MIN, INT32_MAX, 15},
                               {2, 1, 1, 0xFFFF, INT32_MAX, INT32_MAX, 15}, {2, 1, 1, 0xFFFF, 0, 0, INT32_MAX},
                               {2, 1, 1, 0xFFFF, 0, 0, INT32_MIN}, {2, 1, 1, 0xFFFF, 0, INT32_MIN, 0}};
  for (const gpc_aggregate& b : bad) EXPECT(ag_params(&b) == GPC_E_INVALID);
  const gpc_aggregate edge[] = {{1, 0, 0, 0, 0, 0, 0}, {4, 2, 1, 0xFFFF, 32767, 32767, 15}, {1, 2, 0, 20655, 0, 32767, 8}, {4, 0, 1, 1, 5, 5, 1}};
  for (const gpc_aggregate& e : edge) EXPECT(ag_params(&e) == GPC_OK);

  EXPECT(ag_labels(1, 0) == 1 && ag_labels(1, 2) == 5 && ag_labels(2, 0) == 1 && ag_labels(2, 1) == 9 && ag_labels(2, 2) == 25);
  EXPECT(ag_cells(1, 0) == 3 && ag_cells(1, 2) == 7 && ag_cells(2, 0) == 9 && ag_cells(2, 1) == 25 && ag_cells(2, 2) == 49);
  EXPECT(ag_dirs(0) == 0 && ag_dirs(1) == 1 && ag_dirs(6) == 2 && ag_dirs(11) == 3 && ag_dirs(15) == 4);
  EXPECT(ag_chunk(1) == 32 && ag_chunk(5) == 32 && ag_chunk(9) == 16 && ag_chunk(25) == 8);
  EXPECT(ag_blocks(1) == 1 && ag_blocks(64) == 1 && ag_blocks(65) == 2 && ag_blocks(32768) == 512);
  // the header: 10 + 6 d and 50 + 18 d bytes a pixel at range 1
  for (int paths = 0; paths < 16; ++paths) {
    EXPECT(ag_pixel_bytes(1, 1, paths) == 10 + 6 * ag_dirs(paths) && ag_pixel_bytes(2, 1, paths) == 50 + 18 * ag_dirs(paths));
  }
  EXPECT(ag_pixel_bytes(2, 2, 15) == 2 * (49 + 4 * 25));
  // groups: what the budget holds, at least one pair, at most all; the largest image times the largest pixel fits 64 bits
  const std::unique_ptr<int64_t> budget(new int64_t(AG_GROUP_BYTES));
  EXPECT(ag_group(2, 1024, 436, 32, 1, 15, *budget) == 19 && ag_group(2, 1024, 436, 32, 2, 15, *budget) == 8);
  EXPECT(ag_group(1, 1024, 436, 32, 1, 15, *budget) == 32 && ag_group(1, 8, 8, 5, 1, 15, 1) == 1);
  EXPECT(ag_group(2, 41, 23, 5, 1, 15, 2 * 122 * 41 * 23 + 5) == 2 && ag_group(2, 32768, 32768, 65535, 2, 15, *budget) == 1);
  puts("ok");
  return 0;
}
