// forest_groups_check -- Forest::readForestGroups + the group-mode matchPair of include/gpc/inference.hpp for pytest.
//   forest_groups_check <forest.txt> <width> <height> <left.raw> <right.raw>
// prints "GROUPS <n> <tests of group 0> ..." and "RESULT <supports> <candidates L> <candidates R> <fnv1a64 of the
// int32 (x, y, d) triples in output order>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpc/inference.hpp"

static bool read_raw(const char* path, ndb::Buffer<uint8_t>& b, int W, int H) {
  std::vector<uint8_t> bytes((size_t)W * H);
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(bytes.data(), 1, bytes.size(), f);
  fclose(f);
  if (got != bytes.size()) return false;
  b = ndb::Buffer<uint8_t>(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) b(y, x) = bytes[(size_t)y * W + x];
  return true;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]);
  gpc::inference::Forest forest;
  std::vector<gpc::inference::Forest::FilterMask> groups = forest.readForestGroups(argv[1], W, H);
  printf("GROUPS %zu", groups.size());
  for (const auto& g : groups) printf(" %zu", g.mask.size() / 2);
  printf("\n");
  if (groups.empty()) return 1;
  ndb::Buffer<uint8_t> L, R;
  if (!read_raw(argv[4], L, W, H) || !read_raw(argv[5], R, W, H)) return 3;
  forest.warmUp(groups);
  gpc::inference::InferenceSettings s(5, 128, 0, true, false, 1);
  int cl = 0, cr = 0;
  std::vector<ndb::Support> supp = forest.matchPair(L, R, groups, s, &cl, &cr);
  if (gpc::inference::lastStatus() != GPC_OK) return 4;
  uint64_t h = 1469598103934665603ull;  // (the oracle's gpc_oracle_fnv1a64)
  for (const ndb::Support& p : supp) {
    const int32_t v[3] = {(int32_t)p.x, (int32_t)p.y, (int32_t)p.d};
    const uint8_t* b = reinterpret_cast<const uint8_t*>(v);
    for (int i = 0; i < 12; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  printf("RESULT %zu %d %d %llu\n", supp.size(), cl, cr, (unsigned long long)h);
  return 0;
}
