// gpc/training.hpp -- MI355X-native mirror of the reference's forest trainer (lib/gpc/training.hpp):
// ForestSettings and Forest::trainAndExport (bootstrap of the training set per fern, Fern::train on
// the GPU, export in the text format Forest::readForest reads).
// Extensions: Forest::trainAndExport over a gpc::datasource::DeviceTrainingSet (the set stays on the device, every
// fern's bootstrap is a multiplicity per triplet, one gpc_hip_train_forest call trains all ferns), Forest::seed and
// Forest::drawBootstraps.
//
// The Sintel datasources of the reference (gpc::datasource::SintelOpticalFlow, SintelStereo) are in
// gpc/SintelOpticalFlow.hpp and gpc/SintelStereo.hpp, included here as the reference does.
#ifndef _GPC_training
#define _GPC_training
#include <sys/stat.h>

#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpc/Feature.hpp"
#include "gpc/Fern.hpp"
#include "gpc/SintelOpticalFlow.hpp"
#include "gpc/SintelStereo.hpp"
#include "gpc/buffer.hpp"

namespace gpc {

namespace training {
// training.hpp:59-74
struct ForestSettings {
  enum FernType { Zero, Tau };
  FernType fernType;
  std::string getFernTypeName() { return fernType == FernType::Zero ? "zero" : "tau"; }
  double sampleFraction;
  std::vector<gpc::training::Fern> ferns;
  ForestSettings(std::vector<gpc::training::Fern> ferns, double sampleFraction)
      : sampleFraction(sampleFraction), ferns(ferns) {}
};

// training.hpp:91-159
class Forest {
 private:
  typedef gpc::training::Feature::GPCPatchTriplet GPCTriplet_t;
  std::mt19937 rng;
  std::uniform_int_distribution<int> randSample;

  // one line per fern ("<index> <s|m|l> <levels>") followed by one line per level
  // ("<level> <ix> <iy> <jx> <jy> <tau>"): the format Forest::readForest parses (inference.hpp:404-446)
  static void writeForest(std::vector<gpc::training::Fern>& ferns, const std::string& filename) {
    std::ofstream file(filename, std::ios::out | std::ios::trunc);
    file << ferns.size() << endl;
    for (size_t f = 0; f < ferns.size(); ++f) {
      const std::vector<gpc::training::Feature::params> levels = ferns[f].getParameters();
      const int scale = ferns[f].getScale();  // 2: small, 1: medium, 0: large
      file << f << " " << (scale == 2 ? "s" : (scale == 1 ? "m" : "l")) << " " << levels.size() << endl;
      for (size_t l = 0; l < levels.size(); ++l)
        file << l << " " << levels[l].ix << " " << levels[l].iy << " " << levels[l].jx << " " << levels[l].jy << " "
             << levels[l].tau << endl;
    }
  }

 public:
  Forest() {}
  // Every fern trains on its own bootstrap sample (with replacement) of sampleFraction * N triplets, drawn
  // from the first sampleFraction * N triplets like the reference does (training.hpp:113-121).
  void trainAndExport(std::vector<GPCTriplet_t>& trainingSamples, gpc::training::ForestSettings forestSettings,
                      gpc::training::OptimizerSettings optSettings, std::string filename) {
    if (trainingSamples.empty()) {
      cout << "ERR: Training set is empty. Aborting." << endl;
      return;
    }
    std::random_device seedSource;
    rng = std::mt19937(seedSource());
    const int perFern = int(forestSettings.sampleFraction * trainingSamples.size());
    randSample = std::uniform_int_distribution<int>(0, perFern - 1);
    const size_t total = forestSettings.ferns.size();
    for (size_t f = 0; f < total; ++f) {
      std::vector<GPCTriplet_t> bootstrap;
      bootstrap.reserve(perFern > 0 ? perFern : 0);
      for (int k = 0; k < perFern; ++k) bootstrap.push_back(trainingSamples[randSample(rng)]);
      cout << "Fern(" << (f + 1) << "/" << total << ") num samples:" << bootstrap.size() << endl
           << std::string(90, '*') << endl;
      const auto started = std::chrono::high_resolution_clock::now();
      forestSettings.ferns[f].train(bootstrap, optSettings);
      const std::chrono::duration<double> took = std::chrono::high_resolution_clock::now() - started;
      cout << "done in " << took.count() << " s" << endl << endl;
    }
    cout << "Exporting forest" << endl;
    writeForest(forestSettings.ferns, filename);
  }

  // ---- extensions: a forest trained over ONE device-resident set (gpc_hip_train_forest, include/gpc_hip.h)

  // The bootstraps below draw from std::mt19937(s) instead of a generator seeded from std::random_device.  (The host-vector
  // overload above reseeds from std::random_device in every call, like the reference.)
  void seed(unsigned s) {
    seeded = true;
    seedValue = s;
  }
  // Every fern's bootstrap as indices into the set, in fern order: perFern draws each from
  // std::uniform_int_distribution<int>(0, perFern - 1) over the forest's generator, exactly the numbers the host-vector
  // overload draws (training.hpp:113-121).  GPC_TRAIN_DUMP_DRAWS=<file>: appended there, one index per line (tests).
  std::vector<int32_t> drawBootstraps(size_t numFerns, int perFern) {
    if (seeded) {
      rng = std::mt19937(seedValue);
    } else {
      std::random_device seedSource;
      rng = std::mt19937(seedSource());
    }
    std::vector<int32_t> draws;
    if (perFern <= 0) return draws;
    randSample = std::uniform_int_distribution<int>(0, perFern - 1);
    draws.resize(numFerns * (size_t)perFern);
    for (int32_t& d : draws) d = randSample(rng);
    if (const char* dump = std::getenv("GPC_TRAIN_DUMP_DRAWS")) {
      std::ofstream f(dump, std::ios::app);
      for (int32_t d : draws) f << d << "\n";
    }
    return draws;
  }
  // The same forest from a set that is already on the device (SintelOpticalFlow::extractTrainingSet,
  // DeviceTrainingSet::fromHost): a fern's bootstrap is a multiplicity per triplet instead of a copy, and all ferns are
  // trained by one call.  Hyperplanes come from every fern's own generator in the reference's order; the printed header
  // and table per fern are the reference's; one "done in" line for the whole forest.  (Ferns of different depths go in
  // runs of equal depth, one call each.)
  void trainAndExport(gpc::datasource::DeviceTrainingSet& trainingSamples, gpc::training::ForestSettings forestSettings,
                      gpc::training::OptimizerSettings optSettings, std::string filename) {
    const int perFern = int(forestSettings.sampleFraction * trainingSamples.size());
    if (trainingSamples.empty() || perFern <= 0) {
      cout << "ERR: Training set is empty. Aborting." << endl;
      return;
    }
    std::vector<gpc::training::Fern>& ferns = forestSettings.ferns;
    const size_t total = ferns.size();
    const std::vector<int32_t> draws = drawBootstraps(total, perFern);
    const int nres = optSettings.numResamples_;
    const auto started = std::chrono::high_resolution_clock::now();
    for (size_t f0 = 0, f1; f0 < total; f0 = f1) {
      const int depth = ferns[f0].getMaxDepth();
      for (f1 = f0 + 1; f1 < total && ferns[f1].getMaxDepth() == depth; ++f1) {}
      const size_t run = f1 - f0;
      std::vector<gpc_split> cand;
      for (size_t f = f0; f < f1; ++f) {
        const std::vector<gpc_split> c = ferns[f].drawHyperplanes(optSettings);
        cand.insert(cand.end(), c.begin(), c.end());
      }
      cand.resize(cand.size() + 1);  // (never a null pointer, also without resamples)
      std::vector<gpc_split> chosen(run * depth);
      std::vector<gpc_split_stats> stats(run * depth);
      const int st = gpc_hip_train_forest(trainingSamples.ctx(), trainingSamples.set(), (int)run, depth, cand.data(), nres,
                                          optSettings.taulo_, optSettings.tauhi_,
                                          optSettings.onlyScoreNonSplitSamples_ ? 1 : 0, optSettings.w1_,
                                          draws.data() + f0 * (size_t)perFern, perFern, chosen.data(), stats.data());
      if (st != GPC_OK) {
        gpc::inference::detail::fail(st, trainingSamples.ctx(), "gpc_hip_train_forest");
        std::abort();  // as Fern::train: a training run cannot go on without its device results
      }
      for (size_t f = f0; f < f1; ++f) {
        cout << "Fern(" << (f + 1) << "/" << total << ") num samples:" << perFern << endl << std::string(90, '*') << endl;
        ferns[f].adoptTrained(&chosen[(f - f0) * depth], &stats[(f - f0) * depth]);
        cout << endl;
      }
    }
    const std::chrono::duration<double> took = std::chrono::high_resolution_clock::now() - started;
    cout << "done in " << took.count() << " s" << endl << endl;
    cout << "Exporting forest" << endl;
    writeForest(ferns, filename);
  }

 private:
  bool seeded = false;
  unsigned seedValue = 0;
};  // Forest
}  // namespace training
}  // namespace gpc
#endif
