// gpc/SintelStereo.hpp -- MI355X-native mirror of the reference's stereo datasource (lib/gpc/SintelStereo.hpp): walks
// the MPI-Sintel stereo training set, samples ground-truth triplets from the disparity maps, and extracts their patches
// on the GPU (gpc/SintelCommon.hpp -> gpc_hip_extract_triplets).
//
// Draw order.  One std::mt19937 per frame, in the reference's source order.  The negative offset is
// `rightX + randOffset(rng) * signum(rng)` (SintelStereo.hpp:449-450), an expression whose operand order C++ leaves
// unspecified; g++ 11 (-O0, -O2, -O3) evaluates it left to right -- the offset, then the sign -- and so does this header,
// with the two draws spelled out.  Where the reference tree is present,
// tests/test_extract.py compiles the reference's own getGroundTruthMatches unchanged (std::random_device replaced by a
// stand-in with a fixed seed) and checks that both draw the same keypoints.
#ifndef _GPC_SintelStereo
#define _GPC_SintelStereo

#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpc/Feature.hpp"
#include "gpc/SintelCommon.hpp"
#include "gpc/buffer.hpp"

namespace gpc {
namespace datasource {

class SintelStereo {
 private:
  typedef gpc::training::Feature F;
  typedef F::GPCPatchTriplet GPCTriplet_t;
  bool canDoExtraction = false;

 public:
  // SintelStereo.hpp:79-95
  SintelStereo(std::string basePath) {
    if (basePath.empty() || basePath.back() != '/') basePath += "/";
    cleanLeftDir = basePath + "training/clean_left";
    cleanRightDir = basePath + "training/clean_right";
    dispDir = basePath + "training/disparities";
    oclDir = basePath + "training/occlusions";
    oofDir = basePath + "training/outofframe";
    numFrames = countImages();
    canDoExtraction = true;
  }
  SintelStereo() { canDoExtraction = false; }

  // extension: reproducible extraction (tests)
  void seed(unsigned s) {
    gen.seeded = true;
    gen.seed = s;
  }

  // SintelStereo.hpp:106-154, the patches cut on the GPU: extractTrainingSet() read back into host objects
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

  // SintelStereo.hpp:163-165
  void storeTrainingData(std::vector<GPCTriplet_t>& data, std::string path) { Feature.storeAllTriplets(data, path); }
  // SintelStereo.hpp:173-182
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

  // SintelStereo.hpp:229-249: *.png files in the selected scene's clean_left directory
  int countImages(void) { return detail::countImages(cleanLeftDir + "/" + selectedScene); }
  // SintelStereo.hpp:258-268
  int selectScene(std::string sceneName) {
    const std::vector<std::string>& names = detail::sceneNames();
    if (std::find(names.begin(), names.end(), sceneName) != names.end()) {
      selectedScene = sceneName;
      return 0;
    }
    std::cout << "ERR:Scene with name (" << sceneName << ") was not found" << std::endl;
    return 1;
  }
  // SintelStereo.hpp:277-284
  int selectScene(int idx) {
    if (idx > numScenes - 1) return 1;
    selectedScene = detail::sceneNames()[idx];
    numFrames = countImages();
    cout << "Scene name:" << selectedScene << " (" << numFrames << " imgs)" << std::endl;
    return 0;
  }
  const std::string& getSelectedScene() const { return selectedScene; }

  // SintelStereo.hpp:295-303: left and right view of frame id, gray ((r+g+b)/3)
  int getBW(int id, ndb::Buffer<uint8_t>& L, ndb::Buffer<uint8_t>& R) {
    const int err1 = L.readPNG(cleanLeftDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
    const int err2 = R.readPNG(cleanRightDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
    return err1 | err2;
  }
  // SintelStereo.hpp:314-321 (the same files: readPNG makes them gray)
  int getRGB(int id, ndb::Buffer<uint8_t>& L, ndb::Buffer<uint8_t>& R) { return getBW(id, L, R); }
  // SintelStereo.hpp:331-336
  int getOcclusion(int id, ndb::Buffer<uint8_t>& O) {
    return O.readPNG(oclDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
  }
  // SintelStereo.hpp:345-350: the disparity map, an RGB PNG
  int getDisparity(int id, ndb::RGBBuffer& D) {
    return D.readPNGRGB(dispDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
  }
  // SintelStereo.hpp:360-365: the out-of-frame mask
  int getInvalid(int id, ndb::Buffer<uint8_t>& I) {
    return I.readPNG(oofDir + "/" + selectedScene + "/" + detail::frameName(id) + ".png");
  }
  // SintelStereo.hpp:421-422: the disparity a pixel of the map encodes, 4 * r + g / 64 (integer)
  static int decodeDisparity(const ndb::RGBColor& c) { return 4 * c.r + c.g / 64; }

  // SintelStereo.hpp:390-463 with the frame's generator passed in.  A pixel (x, y) of the 1024 x 436 frame matches
  // (x - d, y); both must be safe patch centres and the pixel free in the occlusion and the out-of-frame mask; then it is
  // rejected with probability (15 - min(|d|, 15)) / 15 * 0.5 in INTEGER division -- 0.5 at d == 0, 0 elsewhere (the uniform
  // draw only after the validity test passed).  The negative lies at an offset of [radiusLower, radiusUpper] times a raw
  // signum draw in {-1, 0, 1} on each axis -- so about one in nine negatives sits exactly on the positive -- redrawn until
  // it is a safe patch centre.  Extension: at most drawCap(numKpts) draws (positions and negative attempts); a frame whose
  // maps are smaller than 1024 x 436 yields nothing (the reference reads past them).
  int getGroundTruthMatches(ndb::RGBBuffer& disp, ndb::Buffer<uint8_t>& oof, ndb::Buffer<uint8_t>& occ, int numKpts,
                            int radiusLower, int radiusUpper, std::vector<ndb::Point>& kptsL, std::vector<ndb::Point>& kptsR,
                            std::vector<ndb::Point>& kptsN, std::mt19937& rng) {
    const int width = 1024, height = 436;
    if (disp.width < width || disp.height < height || oof.width < width || oof.height < height || occ.width < width ||
        occ.height < height)
      return 1;
    std::uniform_int_distribution<int> randX(0, width - 1), randY(0, height - 1);
    std::uniform_int_distribution<int> randOffset(radiusLower, radiusUpper), signum(-1, 1);
    std::uniform_real_distribution<> rej(0, 1);
    long draws = 0;
    const long cap = detail::drawCap(numKpts);
    while (kptsL.size() < (size_t)std::max(numKpts, 0)) {
      if (++draws > cap) {
        detail::warnDrawCap(kptsL.size(), numKpts);
        return 0;
      }
      const int xCoord = randX(rng);
      const int yCoord = randY(rng);
      const int disparityGroundTruth = decodeDisparity(disp.getPixel(xCoord, yCoord));
      const int rightX = xCoord - disparityGroundTruth;
      const double alpha = 0.5;
      const double rejectionProp = (15 - std::min(abs(disparityGroundTruth), 15)) / 15 * alpha;
      if (detail::isSafePatchCenter(xCoord, yCoord, width, height) && detail::isSafePatchCenter(rightX, yCoord, width, height) &&
          occ.getPixel(xCoord, yCoord) == 0x00 && oof.getPixel(xCoord, yCoord) == 0x00) {
        if (rejectionProp < rej(rng)) {
          int newX, newY;
          while (true) {
            if (++draws > cap) {
              detail::warnDrawCap(kptsL.size(), numKpts);
              return 0;
            }
            const int ox = randOffset(rng);  // (left to right, see the top of this file)
            const int sx = signum(rng);
            const int oy = randOffset(rng);
            const int sy = signum(rng);
            newX = rightX + ox * sx;
            newY = yCoord + oy * sy;
            if (detail::isSafePatchCenter(newX, newY, width, height)) break;
          }
          kptsL.push_back(ndb::Point(xCoord, yCoord));
          kptsR.push_back(ndb::Point(rightX, yCoord));
          kptsN.push_back(ndb::Point(newX, newY));
        }
      }
    }
    return 0;
  }

  // the generator of frame `ordinal` of the walk (std::random_device, or seed + ordinal after seed())
  std::mt19937 frameGenerator(long ordinal) const { return gen.frame(ordinal); }

 private:
  // SintelStereo.hpp:113-151: scenes 0 .. 19, frames 1 .. n-2; a frame whose files do not all open is skipped
  bool walk(int numTripletsPerPair, int radiusLower, int radiusUpper, detail::FrameBatch& batch) {
    if (canDoExtraction == false) {
      cout << "ERR: No path for Sintel dataset specified" << endl;
      return false;
    }
    if (!(detail::isDir(cleanLeftDir) && detail::isDir(cleanRightDir) && detail::isDir(dispDir) && detail::isDir(oclDir) &&
          detail::isDir(oofDir))) {
      cout << "ERR: This does not look like the Sintel Stereo dataset. Please verify paths." << endl;
      return false;
    }
    long ordinal = 0;
    for (int sceneId = 0; sceneId < detail::kVisitedScenes; sceneId++) {
      selectScene(sceneId);
      const int numImages = countImages();
      for (int imgId = 1; imgId < numImages - 1; imgId++, ordinal++) {
        std::vector<ndb::Point> kptsL, kptsR, kptsN;
        ndb::Buffer<uint8_t> occ, oof, imgL, imgR;
        ndb::RGBBuffer disp;
        int err = 0;
        err |= getBW(imgId, imgL, imgR);
        err |= getDisparity(imgId, disp);
        err |= getOcclusion(imgId, occ);
        err |= getInvalid(imgId, oof);
        if (err) continue;
        std::mt19937 rng = gen.frame(ordinal);
        if (getGroundTruthMatches(disp, oof, occ, numTripletsPerPair, radiusLower, radiusUpper, kptsL, kptsR, kptsN, rng))
          continue;
        batch.add(selectedScene + "/" + detail::frameName(imgId), imgL, imgR, kptsL, kptsR, kptsN);
      }
    }
    return true;
  }

  std::string dispDir, cleanLeftDir, cleanRightDir, oclDir, oofDir;
  std::string selectedScene = "alley_1";  // SintelStereo.hpp:185
  F Feature;
  detail::Generators gen;
  int numScenes = 23;
  int numFrames = 50;
};

}  // namespace datasource
}  // namespace gpc
#endif
