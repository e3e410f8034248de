// gpc/SintelOpticalFlow.hpp -- MI355X-native mirror of the reference's optical-flow datasource
// (lib/gpc/SintelOpticalFlow.hpp): walks the MPI-Sintel training set, samples ground-truth triplets from the flow
// fields, and extracts their patches on the GPU (gpc/SintelCommon.hpp -> gpc_hip_extract_triplets).
//
// Draw order.  The sampler draws from one std::mt19937 per frame in the reference's source order.  The reference writes
// the negative offset as `xCoord2 + randOffset(rng) * sig()` (SintelOpticalFlow.hpp:544-545), whose operand order C++
// leaves unspecified; g++ 11 (-O0, -O2, -O3) evaluates that expression left to right -- the offset, then the sign --
// and so does this header, with the two draws spelled out.  Where the reference tree is present,
// tests/test_extract.py compiles the reference's own getGroundTruthMatches unchanged (Eigen and std::random_device
// replaced by stand-ins with a fixed seed) and checks that both draw the same keypoints.
#ifndef _GPC_SintelOpticalFlow
#define _GPC_SintelOpticalFlow

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpc/Feature.hpp"
#include "gpc/SintelCommon.hpp"
#include "gpc/buffer.hpp"

namespace gpc {
namespace datasource {

// a .flo file: u, v per pixel, x-major access as the reference's Eigen matrices u(x, y) (SintelOpticalFlow.hpp:407-420)
struct FlowField {
  int width = 0, height = 0;
  std::vector<float> u, v;  // row-major [height][width]
  double U(int x, int y) const { return u[(size_t)y * width + x]; }
  double V(int x, int y) const { return v[(size_t)y * width + x]; }
};

class SintelOpticalFlow {
 private:
  typedef gpc::training::Feature F;
  typedef F::GPCPatchTriplet GPCTriplet_t;
  bool canDoExtraction = false;

 public:
  // SintelOpticalFlow.hpp:85-101
  SintelOpticalFlow(std::string basePath) {
    if (basePath.empty() || basePath.back() != '/') basePath += "/";
    cleanDir = basePath + "training/clean";
    finalDir = basePath + "training/final";
    flowDir = basePath + "training/flow";
    oclDir = basePath + "training/occlusions";
    invDir = basePath + "training/invalid";
    numFrames = countImages();
    canDoExtraction = true;
  }
  SintelOpticalFlow() { canDoExtraction = false; }

  // extension: reproducible extraction (tests)
  void seed(unsigned s) {
    gen.seeded = true;
    gen.seed = s;
  }

  // SintelOpticalFlow.hpp:112-162, the patches cut on the GPU: extractTrainingSet() read back into host objects
  std::vector<GPCTriplet_t> extractTrainingData(int numTripletsPerPair, int radiusLower, int radiusUpper) {
    detail::FrameBatch batch;
    std::vector<int32_t> order;
    if (!walk(numTripletsPerPair, radiusLower, radiusUpper, batch)) return std::vector<GPCTriplet_t>();
    DeviceTrainingSet dev = batch.extract(gen, &order);
    return detail::toHost(dev, batch, order);
  }
  // extension: the same set left on the device
  DeviceTrainingSet extractTrainingSet(int numTripletsPerPair, int radiusLower, int radiusUpper) {
    detail::FrameBatch batch;
    if (!walk(numTripletsPerPair, radiusLower, radiusUpper, batch)) return DeviceTrainingSet();
    return batch.extract(gen);
  }
  // extension: the scene walk and the sampler alone (no device): the frames and keypoints extractTrainingSet() would cut
  detail::FrameBatch sampleFrames(int numTripletsPerPair, int radiusLower, int radiusUpper) {
    detail::FrameBatch batch;
    walk(numTripletsPerPair, radiusLower, radiusUpper, batch);
    return batch;
  }

  // SintelOpticalFlow.hpp:171-173
  void storeTrainingData(std::vector<GPCTriplet_t>& data, std::string path) { Feature.storeAllTriplets(data, path); }
  // SintelOpticalFlow.hpp:181-190
  std::vector<GPCTriplet_t> loadTrainingData(std::string path) {
    struct stat buffer;
    if (stat(path.c_str(), &buffer) != 0) {
      std::vector<GPCTriplet_t> emptyset;
      cout << "ERR: No extracted training set found at given path" << endl;
      return emptyset;
    } else {
      return Feature.loadAllTriplets(path);
    }
  }

  // SintelOpticalFlow.hpp:281-301: *.png files in the selected scene's clean directory
  int countImages(void) { return detail::countImages(cleanDir + "/" + selectedScene); }
  // SintelOpticalFlow.hpp:310-318
  void selectScene(std::string sceneName) {
    const std::vector<std::string>& names = detail::sceneNames();
    if (std::find(names.begin(), names.end(), sceneName) != names.end())
      selectedScene = sceneName;
    else
      std::cout << "ERR:Scene with name (" << sceneName << ") was not found" << std::endl;
  }
  // SintelOpticalFlow.hpp:327-334
  int selectScene(int idx) {
    if (idx > numScenes - 1) return 1;
    selectedScene = detail::sceneNames()[idx];
    numFrames = countImages();
    cout << "Scene name:" << selectedScene << " (" << numFrames << " imgs)" << std::endl;
    return 0;
  }
  const std::string& getSelectedScene() const { return selectedScene; }

  // SintelOpticalFlow.hpp:345-354: frames id and id + 1 of the clean pass, gray ((r+g+b)/3)
  int getBW(int id, ndb::Buffer<uint8_t>& L, ndb::Buffer<uint8_t>& R) {
    const int err1 = L.readPNG(cleanDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
    const int err2 = R.readPNG(cleanDir + "/" + selectedScene + "/" + detail::frameName(id + 1) + ".png");
    return err1 | err2;
  }
  // SintelOpticalFlow.hpp:365-373 (the same files: readPNG makes them gray)
  int getRGB(int id, ndb::Buffer<uint8_t>& L, ndb::Buffer<uint8_t>& R) { return getBW(id, L, R); }

  // SintelOpticalFlow.hpp:384-425: float tag 202021.25, int32 width, int32 height, then u, v float32 interleaved, row-major.
  // A tag other than 202021.25 is reported and the file read anyway, as the reference does.  0 = ok.  Extension: a file
  // that is missing or shorter than its header says returns 1 (the reference calls fseek on a null FILE* / reads past
  // its buffer), and the frame is skipped.
  int getFlow(int id, FlowField& flow) {
    const std::string filename = flowDir + "/" + selectedScene + "/" + detail::frameName(id) + ".flo";
    FILE* f = fopen(filename.c_str(), "rb");
    if (!f) {
      cout << "ERR: File" << filename << " could not be opened for reading" << endl;
      return 1;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    if (buf.size() < 12) {
      cout << "Read error" << endl;
      return 1;
    }
    float tag;
    int32_t w, h;
    std::memcpy(&tag, &buf[0], 4);
    std::memcpy(&w, &buf[4], 4);
    std::memcpy(&h, &buf[8], 4);
    if (tag != 202021.25f) cout << "TAG not found" << endl;
    if (w < 0 || h < 0 || buf.size() < 12 + 8 * (size_t)w * (size_t)h) {
      cout << "Read error" << endl;
      return 1;
    }
    flow.width = w;
    flow.height = h;
    flow.u.resize((size_t)w * h);
    flow.v.resize((size_t)w * h);
    const uint8_t* p = &buf[12];
    for (size_t k = 0; k < (size_t)w * h; ++k, p += 8) {
      std::memcpy(&flow.u[k], p, 4);
      std::memcpy(&flow.v[k], p + 4, 4);
    }
    return 0;
  }
  // SintelOpticalFlow.hpp:434-439
  int getOcclusion(int id, ndb::Buffer<uint8_t>& O) {
    return O.readPNG(oclDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
  }
  // SintelOpticalFlow.hpp:448-453
  int getInvalid(int id, ndb::Buffer<uint8_t>& I) {
    return I.readPNG(invDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
  }

  // SintelOpticalFlow.hpp:478-558 with the frame's generator passed in.  A pixel (x, y) of the 1024 x 436 frame matches
  // (x + round(u), y + round(v)); both points must be safe patch centres and the pixel free in both occlusion and both
  // invalid masks, all read at the SOURCE coordinates; then it is rejected with probability
  // (15 - min(|round(u), round(v)|, 15)) / 15 * 0.5 (the uniform draw only after the validity test passed).  The negative
  // lies at an offset of [radiusLower, radiusUpper] with a nonzero sign on each axis from the positive, redrawn until it
  // is a safe patch centre.  Extension: at most drawCap(numKpts) draws (positions and negative attempts); a frame whose
  // fields or masks are smaller than 1024 x 436 yields nothing (the reference reads past them).
  int getGroundTruthMatches(const FlowField& flow, ndb::Buffer<uint8_t>& oSrc, ndb::Buffer<uint8_t>& oTar,
                            ndb::Buffer<uint8_t>& invSrc, ndb::Buffer<uint8_t>& invTar, int numKpts, int radiusLower,
                            int radiusUpper, std::vector<ndb::Point>& kptsL, std::vector<ndb::Point>& kptsR,
                            std::vector<ndb::Point>& kptsN, std::mt19937& rng) {
    const int width = 1024, height = 436;
    for (const ndb::Buffer<uint8_t>* m : {&oSrc, &oTar, &invSrc, &invTar})
      if (m->width < width || m->height < height) return 1;
    if (flow.width < width || flow.height < height) return 1;
    std::uniform_int_distribution<int> randX(0, width - 1), randY(0, height - 1);
    std::uniform_int_distribution<int> randOffset(radiusLower, radiusUpper), signum(-1, 1);
    std::uniform_real_distribution<> rej(0, 1);
    auto sig = [&](void) {
      int k = signum(rng);
      while (k == 0) k = signum(rng);
      return k;
    };
    long draws = 0;
    const long cap = detail::drawCap(numKpts);
    while (kptsL.size() < (size_t)std::max(numKpts, 0)) {
      if (++draws > cap) {
        detail::warnDrawCap(kptsL.size(), numKpts);
        return 0;
      }
      const int xCoord = randX(rng);
      const int yCoord = randY(rng);
      const int ru = int(round(flow.U(xCoord, yCoord))), rv = int(round(flow.V(xCoord, yCoord)));
      const int xCoord2 = xCoord + ru;
      const int yCoord2 = yCoord + rv;
      const double disparity = sqrt(pow(ru, 2) + pow(rv, 2));
      const double alpha = 0.5;
      const double rejectionProp = (15 - std::min(disparity, 15.)) / 15 * alpha;
      if (detail::isSafePatchCenter(xCoord, yCoord, width, height) && detail::isSafePatchCenter(xCoord2, yCoord2, width, height) &&
          oSrc.getPixel(xCoord, yCoord) == 0x00 && oTar.getPixel(xCoord, yCoord) == 0x00 &&
          invSrc.getPixel(xCoord, yCoord) == 0x00 && invTar.getPixel(xCoord, yCoord) == 0x00) {
        if (rejectionProp < rej(rng)) {
          int newX, newY;
          while (true) {
            if (++draws > cap) {
              detail::warnDrawCap(kptsL.size(), numKpts);
              return 0;
            }
            const int ox = randOffset(rng);  // (left to right, see the top of this file)
            const int sx = sig();
            const int oy = randOffset(rng);
            const int sy = sig();
            newX = xCoord2 + ox * sx;
            newY = yCoord2 + oy * sy;
            if (detail::isSafePatchCenter(newX, newY, width, height)) break;
          }
          kptsL.push_back(ndb::Point(xCoord, yCoord));
          kptsR.push_back(ndb::Point(xCoord2, yCoord2));
          kptsN.push_back(ndb::Point(newX, newY));
        }
      }
    }
    return 0;
  }

  // the generator of frame `ordinal` of the walk (std::random_device, or seed + ordinal after seed())
  std::mt19937 frameGenerator(long ordinal) const { return gen.frame(ordinal); }

 private:
  // SintelOpticalFlow.hpp:119-157: scenes 0 .. 19, frames 1 .. n-2; a frame whose files do not all open is skipped
  bool walk(int numTripletsPerPair, int radiusLower, int radiusUpper, detail::FrameBatch& batch) {
    if (canDoExtraction == false) {
      cout << "ERR: No path for Sintel dataset specified" << endl;
      return false;
    }
    if (!(detail::isDir(cleanDir) && detail::isDir(finalDir) && detail::isDir(flowDir) && detail::isDir(oclDir) &&
          detail::isDir(invDir))) {
      cout << "ERR: This does not look like the Sintel Optical Flow dataset. Please verify paths." << endl;
      return false;
    }
    long ordinal = 0;
    for (int sceneId = 0; sceneId < detail::kVisitedScenes; sceneId++) {
      selectScene(sceneId);
      const int numImages = countImages();
      for (int imgId = 1; imgId < numImages - 1; imgId++, ordinal++) {
        std::vector<ndb::Point> kptsL, kptsR, kptsN;
        ndb::Buffer<uint8_t> oSrc, oTar, invSrc, invTar, imgL, imgR;
        FlowField flow;
        int err = 0;
        err |= getFlow(imgId, flow);
        err |= getBW(imgId, imgL, imgR);
        err |= getOcclusion(imgId, oSrc);
        err |= getOcclusion(imgId + 1, oTar);
        err |= getInvalid(imgId, invSrc);
        err |= getInvalid(imgId + 1, invTar);
        if (err) continue;
        std::mt19937 rng = gen.frame(ordinal);
        if (getGroundTruthMatches(flow, oSrc, oTar, invSrc, invTar, numTripletsPerPair, radiusLower, radiusUpper, kptsL,
                                  kptsR, kptsN, rng))
          continue;
        batch.add(selectedScene + "/" + detail::frameName(imgId), imgL, imgR, kptsL, kptsR, kptsN);
      }
    }
    return true;
  }

  std::string cleanDir, finalDir, flowDir, oclDir, invDir;
  std::string selectedScene = "alley_1";  // SintelOpticalFlow.hpp:193
  F Feature;
  detail::Generators gen;
  int numScenes = 23;
  int numFrames = 50;
};

}  // namespace datasource
}  // namespace gpc
#endif
