// train_forest_check -- gpc::training::Forest::trainAndExport over a device-resident set, for tests/test_gpu_train_forest.py.
//   train_forest_check <triplets.bin> <out.txt> <forest seed> <fern seed> <taulo> <tauhi> <only> <w1>
// Loads the triplets, uploads them once (DeviceTrainingSet::fromHost) and trains three ferns, one per scale, of depth 3
// with 4 resamples on 70 % bootstraps.  The forest's generator is seeded with <forest seed>, fern f's hyperplane generator
// with <fern seed> + f, so a second run repeats the first; GPC_TRAIN_DUMP_CANDIDATES and GPC_TRAIN_DUMP_DRAWS receive what
// was drawn.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "gpc/training.hpp"

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  gpc::datasource::SintelOpticalFlow src;
  gpc::datasource::DeviceTrainingSet dev;
  {
    auto data = src.loadTrainingData(argv[1]);
    dev = gpc::datasource::DeviceTrainingSet::fromHost(data);
  }
  std::printf("SIZE %d\n", dev.size());
  gpc::training::OptimizerSettings opt(std::atoi(argv[5]), std::atoi(argv[6]), 4, std::atoi(argv[7]) != 0, std::atof(argv[8]));
  gpc::training::ForestSettings fs(gpc::training::FernFactory(1, 1, 1, 3), 0.7);
  for (size_t f = 0; f < fs.ferns.size(); ++f) fs.ferns[f].seed((unsigned)std::atoi(argv[4]) + (unsigned)f);
  gpc::training::Forest forest;
  forest.seed((unsigned)std::atoi(argv[3]));
  forest.trainAndExport(dev, fs, opt, argv[2]);
  // an empty set is refused like an empty vector
  gpc::datasource::DeviceTrainingSet none;
  forest.trainAndExport(none, fs, opt, std::string(argv[2]) + ".none");
  return 0;
}
