// extract_check -- drives the Sintel datasources (include/gpc/Sintel*.hpp) and the extraction paths for
// tests/test_extract.py.
//   flo <root> <scene> <id> <x> <y>               -> SintelOpticalFlow::getFlow: "FLO w h u(x,y) v(x,y)"
//   disp <root> <scene> <id> <x> <y>              -> SintelStereo::getDisparity: "DISP d r g b"
//   points <root> flow|stereo <per> <lo> <hi> <seed> -> sampleFrames: "F <scene/frame> <first>" per frame, "P rx ry px py nx ny"
//   cap                                           -> the draw cap on frames without a valid pixel: "CAP <flow> <stereo>"
//   extract <root> flow|stereo <per> <lo> <hi> <seed> <out.bin>  -> extractTrainingSet, read back, written like storeAllTriplets
//   host <L.bin> <R.bin> <pts.bin> <W> <H> <nframes> <first.bin> <out.bin>
//        -> Feature::extractAllTriplets frame by frame (the existing host path), stored with storeAllTriplets
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>

#include "gpc/training.hpp"

using gpc::datasource::SintelOpticalFlow;
using gpc::datasource::SintelStereo;

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream in(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "flo") {
    SintelOpticalFlow ds(argv[2]);
    ds.selectScene(std::string(argv[3]));
    gpc::datasource::FlowField f;
    const int rc = ds.getFlow(std::atoi(argv[4]), f);
    if (rc) {
      std::printf("FLO missing\n");
      return 0;
    }
    const int x = std::atoi(argv[5]), y = std::atoi(argv[6]);
    std::printf("FLO %d %d %.9g %.9g\n", f.width, f.height, f.U(x, y), f.V(x, y));
    return 0;
  }
  if (cmd == "disp") {
    SintelStereo ds(argv[2]);
    ds.selectScene(std::string(argv[3]));
    ndb::RGBBuffer d;
    if (ds.getDisparity(std::atoi(argv[4]), d)) return 1;
    const ndb::RGBColor c = d.getPixel(std::atoi(argv[5]), std::atoi(argv[6]));
    std::printf("DISP %d %d %d %d\n", SintelStereo::decodeDisparity(c), c.r, c.g, c.b);
    return 0;
  }
  if (cmd == "points" || cmd == "extract") {
    const bool stereo = !std::strcmp(argv[3], "stereo");
    const int per = std::atoi(argv[4]), lo = std::atoi(argv[5]), hi = std::atoi(argv[6]);
    const unsigned seed = (unsigned)std::strtoul(argv[7], nullptr, 10);
    SintelOpticalFlow flow(argv[2]);
    SintelStereo st(argv[2]);
    flow.seed(seed);
    st.seed(seed);
    if (cmd == "points") {
      gpc::datasource::detail::FrameBatch b = stereo ? st.sampleFrames(per, lo, hi) : flow.sampleFrames(per, lo, hi);
      for (int f = 0; f < b.nframes; ++f) {
        std::printf("F %s %d\n", b.names[f].c_str(), b.first[f]);
        for (int k = b.first[f]; k < b.first[f + 1]; ++k)
          std::printf("P %d %d %d %d %d %d\n", b.pts[k].rx, b.pts[k].ry, b.pts[k].px, b.pts[k].py, b.pts[k].nx, b.pts[k].ny);
      }
      return 0;
    }
    gpc::datasource::DeviceTrainingSet dev = stereo ? st.extractTrainingSet(per, lo, hi) : flow.extractTrainingSet(per, lo, hi);
    std::vector<uint8_t> aos((size_t)dev.size() * 3 * 729);
    if (dev.read(0, dev.size(), aos.data()) != GPC_OK) return 1;
    std::ofstream(argv[8], std::ios::binary).write(reinterpret_cast<const char*>(aos.data()), aos.size());
    std::printf("EXTRACTED %d\n", dev.size());
    return 0;
  }
  if (cmd == "cap") {
    // nothing valid: every pixel occluded
    ndb::Buffer<uint8_t> occ(436, 1024, 255), clear(436, 1024, 0);
    gpc::datasource::FlowField f;
    f.width = 1024;
    f.height = 436;
    f.u.assign(1024 * 436, 0.f);
    f.v.assign(1024 * 436, 0.f);
    ndb::RGBBuffer d;
    static_cast<ndb::Buffer<ndb::RGBColor>&>(d) = ndb::Buffer<ndb::RGBColor>(436, 1024);
    std::vector<ndb::Point> a, b, c, e, g, h;
    std::mt19937 r1(1), r2(2);
    SintelOpticalFlow().getGroundTruthMatches(f, occ, clear, clear, clear, 5, 20, 40, a, b, c, r1);
    SintelStereo().getGroundTruthMatches(d, clear, occ, 5, 20, 40, e, g, h, r2);
    std::printf("CAP %zu %zu\n", a.size(), e.size());
    return 0;
  }
  if (cmd == "host") {
    const std::vector<uint8_t> L = slurp(argv[2]), R = slurp(argv[3]), P = slurp(argv[4]), FF = slurp(argv[8]);
    const int W = std::atoi(argv[5]), H = std::atoi(argv[6]), nframes = std::atoi(argv[7]);
    const gpc_triplet_points* pts = reinterpret_cast<const gpc_triplet_points*>(P.data());
    const int32_t* first = reinterpret_cast<const int32_t*>(FF.data());
    gpc::training::Feature feature;
    std::vector<gpc::training::Feature::GPCPatchTriplet> triplets;
    for (int f = 0; f < nframes; ++f) {
      ndb::Buffer<uint8_t> bl(H, W), br(H, W);
      std::memcpy(bl.data(), &L[(size_t)f * W * H], (size_t)W * H);
      std::memcpy(br.data(), &R[(size_t)f * W * H], (size_t)W * H);
      std::vector<ndb::Point> kr, kp, kn;
      for (int k = first[f]; k < first[f + 1]; ++k) {
        kr.emplace_back(pts[k].rx, pts[k].ry);
        kp.emplace_back(pts[k].px, pts[k].py);
        kn.emplace_back(pts[k].nx, pts[k].ny);
      }
      feature.extractAllTriplets(bl, br, kr, kp, kn, triplets);
    }
    feature.storeAllTriplets(triplets, argv[9]);
    std::printf("HOST %zu\n", triplets.size());
    return 0;
  }
  return 2;
}
