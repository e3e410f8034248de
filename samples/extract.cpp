// extract -- samples ground-truth patch triplets from the MPI-Sintel training set and writes them in the file format
// samples/train reads (3 x 729 bytes per triplet).  Same role and defaults as the reference's samples/extract.cpp; the
// patches are cut on the MI355X (gpc/SintelOpticalFlow.hpp, gpc/SintelStereo.hpp -> libgpc_hip.so).
//
// usage: extract <sintel root> <out.bin> [flow|stereo] [triplets per pair] [r_lo] [r_hi] [seed]
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "gpc/training.hpp"

int main(int argc, char** argv) {
  std::string sintelPath = "../../data/MPI-Sintel-complete";
  std::string outputFile = "../../data/SintelOpticalFlow-extracted.bin";
  if (argc >= 3) {
    sintelPath = argv[1];
    outputFile = argv[2];
  } else {
    std::cout << "Usage: " << argv[0]
              << " <sintel training set root dir path> <extracted dataset path> [flow|stereo] [triplets per pair]"
                 " [r_lo] [r_hi] [seed]"
              << std::endl;
    std::cout << "Trying defaults:" << std::endl;
    std::cout << "Sintel dataset location    : " << sintelPath << std::endl;
    std::cout << "Export extracted dataset to: " << outputFile << std::endl;
  }
  const bool stereo = argc >= 4 && !std::strcmp(argv[3], "stereo");
  // the reference's choice: up to 1000 triplets per pair, the negative from the annulus of radii 20 .. 40 around the match
  const int perPair = argc >= 5 ? std::atoi(argv[4]) : 1000;
  const int rlo = argc >= 6 ? std::atoi(argv[5]) : 20;
  const int rhi = argc >= 7 ? std::atoi(argv[6]) : 40;

  std::vector<gpc::training::Feature::GPCPatchTriplet> trainingData;
  std::cout << "Extracting samples" << std::endl;
  if (stereo) {
    gpc::datasource::SintelStereo source(sintelPath);
    if (argc >= 8) source.seed((unsigned)std::strtoul(argv[7], nullptr, 10));
    trainingData = source.extractTrainingData(perPair, rlo, rhi);
    source.storeTrainingData(trainingData, outputFile);
  } else {
    gpc::datasource::SintelOpticalFlow source(sintelPath);
    if (argc >= 8) source.seed((unsigned)std::strtoul(argv[7], nullptr, 10));
    trainingData = source.extractTrainingData(perPair, rlo, rhi);
    source.storeTrainingData(trainingData, outputFile);
  }
  std::cout << "Extracted " << trainingData.size() << " triplets" << std::endl;
  return trainingData.empty() ? 1 : 0;
}
