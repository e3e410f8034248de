// consensus -- match, then filter the matches by grid motion consensus (include/gpc/consensus.hpp):
//   consensus forest.txt stereo left.png right.png [disparity.png]
//   consensus forest.txt flow frame0.png frame1.png [frame2.png ...] [flow0.flo flow1.flo ...]
// stereo matches one rectified pair (Forest::matchPair), flow every consecutive pair of frames (Forest::sequenceMatch),
// and both print the number of matches before and after the filter (cell 16, shifts 4, alpha 6 / 1; --cell, --shifts,
// --alpha NUM DEN change them).  With ground truth -- a Sintel RGB disparity map for stereo, one .flo file per frame pair
// for flow -- the precision within 1 and 3 pixels (gpc_hip_score_*) is printed before and after as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/consensus.hpp"
#include "gpc/evaluation.hpp"

using gpc::evaluation::Score;
using gpc::evaluation::Truth;

// a Middlebury .flo file: the float 202021.25, width, height, then u and v of every pixel, row by row
static bool readFlo(const std::string& path, gpc::datasource::FlowField& f) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  float tag = 0.f;
  int32_t w = 0, h = 0;
  bool ok = fread(&tag, 4, 1, fp) == 1 && fread(&w, 4, 1, fp) == 1 && fread(&h, 4, 1, fp) == 1 && tag == 202021.25f && w > 0 &&
            h > 0 && w <= 16384 && h <= 16384;
  if (ok) {
    std::vector<float> uv((size_t)w * h * 2);
    ok = fread(uv.data(), sizeof(float), uv.size(), fp) == uv.size();
    f.width = w, f.height = h;
    f.u.resize((size_t)w * h), f.v.resize((size_t)w * h);
    for (size_t i = 0; ok && i < (size_t)w * h; ++i) f.u[i] = uv[2 * i], f.v[i] = uv[2 * i + 1];
  }
  fclose(fp);
  return ok;
}

static void printScore(const char* what, const Score& s) {
  std::printf("  %-7s %9lld records, %9lld judged, within 1 px %.4f, within 3 px %.4f\n", what, (long long)s.n_records,
              (long long)s.n_judged, s.precision(0), s.precision(1));
}

static bool ends_with(const std::string& s, const char* e) { return s.size() >= strlen(e) && s.compare(s.size() - strlen(e), strlen(e), e) == 0; }

int main(int argc, char** argv) {
  gpc::consensus::Settings cs;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--cell") && i + 1 < argc) cs.cell = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--shifts") && i + 1 < argc) cs.shifts = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--alpha") && i + 2 < argc) cs.alphaNum = atoi(argv[i + 1]), cs.alphaDen = atoi(argv[i + 2]), i += 2;
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 4 || (pos[1] != "stereo" && pos[1] != "flow")) {
    std::printf("usage: consensus forest.txt stereo left.png right.png [disparity.png]\n"
                "       consensus forest.txt flow frame0.png frame1.png [...] [flow0.flo ...]\n"
                "       options: --cell C --shifts 1|4 --alpha NUM DEN\n");
    return 1;
  }
  const std::vector<float> thr = {1.f, 3.f};
  gpc::inference::Forest forest;
  if (pos[1] == "stereo") {
    ndb::Buffer<uint8_t> L, R;
    if (L.readPNG(pos[2]) || R.readPNG(pos[3]) || L.cols() != R.cols() || L.rows() != R.rows()) return 1;
    gpc::inference::Forest::FilterMask fm = forest.readForest(pos[0], L.cols(), L.rows());
    gpc::inference::InferenceSettings settings(5, 128, 0, true, false, 1);
    std::vector<ndb::Support> raw = forest.matchPair(L, R, fm, settings);
    if (gpc::inference::lastStatus() != GPC_OK) return 2;
    std::vector<ndb::Support> kept = gpc::consensus::filter(raw, L.cols(), L.rows(), cs);
    if (gpc::inference::lastStatus() != GPC_OK) return 2;
    std::printf("%zu matches, %zu kept\n", raw.size(), kept.size());
    if (pos.size() > 4) {
      ndb::RGBBuffer disp;
      if (disp.readPNGRGB(pos[4])) return 1;
      const ndb::Buffer<uint8_t> none;
      const Truth truth = Truth::fromDisparity(disp, none, none).resized(L.cols(), L.rows());
      printScore("before", gpc::evaluation::scoreSupports(raw, truth, thr));
      printScore("after", gpc::evaluation::scoreSupports(kept, truth, thr));
      if (gpc::inference::lastStatus() != GPC_OK) return 2;
    }
    return 0;
  }
  std::vector<ndb::Buffer<uint8_t>> frames;
  std::vector<std::string> flo;
  for (size_t k = 2; k < pos.size(); ++k) {
    if (ends_with(pos[k], ".flo")) {
      flo.push_back(pos[k]);
      continue;
    }
    ndb::Buffer<uint8_t> img;
    if (img.readPNG(pos[k])) return 1;
    if (!frames.empty() && (img.cols() != frames[0].cols() || img.rows() != frames[0].rows())) {
      std::printf("%s: another size than the first frame\n", pos[k].c_str());
      return 1;
    }
    frames.push_back(img);
  }
  if (frames.size() < 2 || (!flo.empty() && flo.size() != frames.size() - 1)) {
    std::printf("flow: at least two frames, and one .flo file per consecutive pair (or none)\n");
    return 1;
  }
  const int W = frames[0].cols(), H = frames[0].rows();
  gpc::inference::Forest::FilterMask fm = forest.readForest(pos[0], W, H);
  gpc::inference::InferenceSettings settings(5, 128, 0, false, false, 1);  // optical flow: no epipolar constraint
  std::vector<std::vector<ndb::Correspondence>> raw = forest.sequenceMatch(frames, fm, settings);
  if (gpc::inference::lastStatus() != GPC_OK) return 2;
  std::vector<std::vector<ndb::Correspondence>> kept = gpc::consensus::filter(raw, W, H, cs);
  if (gpc::inference::lastStatus() != GPC_OK) return 2;
  Score before, after;
  for (size_t t = 0; t < raw.size(); ++t) {
    std::printf("pair %zu: %zu matches, %zu kept\n", t, raw[t].size(), kept[t].size());
    if (flo.empty()) continue;
    gpc::datasource::FlowField f;
    if (!readFlo(flo[t], f)) {
      std::printf("cannot read %s\n", flo[t].c_str());
      return 1;
    }
    const ndb::Buffer<uint8_t> none;
    const Truth truth = Truth::fromFlow(f, none, none, none, none).resized(W, H);
    before += gpc::evaluation::scoreCorrespondences(raw[t], truth, thr);
    after += gpc::evaluation::scoreCorrespondences(kept[t], truth, thr);
    if (gpc::inference::lastStatus() != GPC_OK) return 2;
  }
  if (!flo.empty()) {
    printScore("before", before);
    printScore("after", after);
  }
  return 0;
}
