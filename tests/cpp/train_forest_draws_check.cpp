// train_forest_draws_check -- host only (tests/test_train_forest_draws.py): the bootstraps gpc::training::Forest draws
// for its device overload after seed(s) are std::mt19937(s) through std::uniform_int_distribution<int>(0, perFern - 1),
// taken nferns * perFern times in fern order -- the numbers the host-vector overload draws (training.hpp:113-121) -- and
// GPC_TRAIN_DUMP_DRAWS receives exactly them.
//   train_forest_draws_check <seed> <nferns> <perFern> [dump file]      exit status 0 and "DRAWS OK <count>" when they agree
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <vector>

#include "gpc/training.hpp"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const unsigned seed = (unsigned)std::strtoul(argv[1], nullptr, 10);
  const int nferns = std::atoi(argv[2]), perFern = std::atoi(argv[3]);
  if (argc >= 5) setenv("GPC_TRAIN_DUMP_DRAWS", argv[4], 1);

  gpc::training::Forest forest;
  forest.seed(seed);
  const std::vector<int32_t> got = forest.drawBootstraps((size_t)nferns, perFern);

  std::vector<int32_t> want;
  std::mt19937 rng(seed);
  std::uniform_int_distribution<int> randSample(0, perFern - 1);
  for (int f = 0; f < nferns; ++f)
    for (int k = 0; k < perFern; ++k) want.push_back(randSample(rng));
  if (got != want) {
    std::printf("DRAWS DIFFER %zu %zu\n", got.size(), want.size());
    return 1;
  }
  // seeded: a second forest, and a second call of the same one, repeat the first
  gpc::training::Forest again;
  again.seed(seed);
  if (again.drawBootstraps((size_t)nferns, perFern) != want || forest.drawBootstraps((size_t)nferns, perFern) != want) {
    std::printf("DRAWS NOT REPRODUCIBLE\n");
    return 1;
  }
  // another seed gives other draws (as soon as there is something to choose)
  gpc::training::Forest other;
  other.seed(seed + 1);
  if (perFern > 1 && want.size() >= 16 && other.drawBootstraps((size_t)nferns, perFern) == want) {
    std::printf("SEED IGNORED\n");
    return 1;
  }
  if (argc >= 5) {  // four calls appended to the dump; the first three wrote `want`
    std::ifstream f(argv[4]);
    std::vector<int32_t> dumped;
    for (int32_t v; f >> v;) dumped.push_back(v);
    const size_t calls = (perFern > 1 && want.size() >= 16) ? 4 : 3;
    if (dumped.size() != calls * want.size()) {
      std::printf("DUMP SIZE %zu\n", dumped.size());
      return 1;
    }
    for (size_t c = 0; c < 3; ++c)
      for (size_t k = 0; k < want.size(); ++k)
        if (dumped[c * want.size() + k] != want[k]) {
          std::printf("DUMP DIFFERS\n");
          return 1;
        }
  }
  std::printf("DRAWS OK %zu\n", got.size());
  return 0;
}
