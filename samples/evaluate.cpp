// evaluate -- precision and recall of a forest's matches against Sintel ground truth, scored on the GPU.
//
//     evaluate forest.txt <sintel root> [flow|stereo] [scene] [first frame] [frames] [thr ...]
//
// Walks one scene with the datasources of gpc/SintelOpticalFlow.hpp / gpc/SintelStereo.hpp.  stereo: the left / right views
// of every frame, matched with sparsematch's settings and scored against the disparity map; flow: consecutive frames of
// the clean pass, matched with epipolarMode(false) and scored against the .flo fields.  One line per frame and a total:
// records, judged, within each threshold, matchable, precision and recall at each threshold.  All trees are used when the
// file holds more than 32 tests (stereo; sequences take the first 32).  A frame whose ground-truth files are missing or
// short is skipped with a message.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "gpc/evaluation.hpp"

using gpc::evaluation::Score;
using gpc::evaluation::Truth;
typedef gpc::inference::Forest Forest;

static void printScore(const std::string& name, const Score& s, const std::vector<float>& thr) {
  printf("%s records %lld judged %lld within", name.c_str(), (long long)s.n_records, (long long)s.n_judged);
  for (size_t k = 0; k < thr.size(); ++k) printf(" %lld", (long long)s.n_within[k]);
  printf(" matchable %lld precision", (long long)s.n_matchable);
  for (size_t k = 0; k < thr.size(); ++k) printf(" %.4f", s.precision((int)k));
  printf(" recall");
  for (size_t k = 0; k < thr.size(); ++k) printf(" %.4f", s.recall((int)k));
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cout << "Usage: " << argv[0] << " forest.txt <sintel root> [flow|stereo] [scene] [first frame] [frames] [thr ...]" << std::endl;
    return 1;
  }
  const std::string forestPath = argv[1], root = argv[2], kind = argc > 3 ? argv[3] : "stereo";
  const std::string scene = argc > 4 ? argv[4] : "alley_1";
  const int first = argc > 5 ? atoi(argv[5]) : 1;
  int count = argc > 6 ? atoi(argv[6]) : 0;
  std::vector<float> thr;
  for (int i = 7; i < argc && thr.size() < GPC_SCORE_MAX_THR; ++i) thr.push_back((float)atof(argv[i]));
  if (thr.empty()) thr = {1.f, 3.f, 10.f};
  if (kind != "flow" && kind != "stereo") {
    std::cout << "Usage: the third argument is flow or stereo" << std::endl;
    return 1;
  }
  Forest forest;
  Score total;
  int scored = 0;
  if (kind == "stereo") {
    gpc::datasource::SintelStereo src(root);
    if (src.selectScene(scene)) return 1;
    if (count <= 0) count = src.countImages() - first + 1;
    gpc::inference::InferenceSettings settings =
        gpc::inference::InferenceSettings().builder().gradientThreshold(5).verticalTolerance(0).dispHigh(128).epipolarMode(true).useHashtable(false);
    std::vector<Forest::FilterMask> groups;
    Forest::FilterMask fm(std::vector<int32_t>(), 0, 0, 0);
    bool have = false;
    for (int id = first; id < first + count; ++id) {
      ndb::Buffer<uint8_t> L, R, ocl, oof;
      ndb::RGBBuffer disp;
      if (src.getBW(id, L, R) | src.getDisparity(id, disp) | src.getOcclusion(id, ocl) | src.getInvalid(id, oof)) {
        std::cout << "ERR: " << scene << "/" << gpc::datasource::detail::frameName(id) << ": files missing, skipped" << std::endl;
        continue;
      }
      if (disp.cols() < ocl.cols() - 15 || disp.rows() != L.rows() || ocl.rows() != L.rows() || oof.rows() != L.rows()) {
        std::cout << "ERR: " << scene << "/" << gpc::datasource::detail::frameName(id) << ": ground truth of another size, skipped" << std::endl;
        continue;
      }
      if (!have) {
        groups = forest.readForestGroups(forestPath, L.cols(), L.rows());
        fm = forest.readForest(forestPath, L.cols(), L.rows());
        if (groups.size() > 1) std::cout << "using all " << groups.size() << " groups of the forest" << std::endl;
        have = true;
      }
      const Truth truth = Truth::fromDisparity(disp, ocl, oof).resized(L.cols(), L.rows());
      gpc::inference::clearStatus();
      const Score s = groups.size() > 1 ? forest.scorePair(L, R, groups, settings, truth, thr) : forest.scorePair(L, R, fm, settings, truth, thr);
      if (gpc::inference::lastStatus() != GPC_OK) return 2;
      printScore(scene + "/" + gpc::datasource::detail::frameName(id), s, thr);
      total += s;
      ++scored;
    }
  } else {
    gpc::datasource::SintelOpticalFlow src(root);
    src.selectScene(scene);
    if (src.getSelectedScene() != scene) return 1;
    if (count <= 0) count = src.countImages() - first;
    gpc::inference::InferenceSettings settings =
        gpc::inference::InferenceSettings().builder().gradientThreshold(5).verticalTolerance(0).dispHigh(128).epipolarMode(false).useHashtable(false);
    // runs of consecutive pairs whose files are all there: each run is one sequence (every frame hashed once)
    std::vector<ndb::Buffer<uint8_t>> frames;
    std::vector<Truth> truths;
    std::vector<std::string> names;
    Forest::FilterMask fm(std::vector<int32_t>(), 0, 0, 0);
    bool have = false;
    auto flush = [&]() -> bool {
      if (!truths.empty()) {
        gpc::inference::clearStatus();
        const std::vector<Score> sc = forest.scoreSequence(frames, fm, settings, truths, thr);
        if (gpc::inference::lastStatus() != GPC_OK || sc.size() != truths.size()) return false;
        for (size_t t = 0; t < sc.size(); ++t) {
          printScore(names[t], sc[t], thr);
          total += sc[t];
          ++scored;
        }
      }
      frames.clear();
      truths.clear();
      names.clear();
      return true;
    };
    for (int id = first; id < first + count; ++id) {
      ndb::Buffer<uint8_t> A, B, oS, oT, iS, iT;
      gpc::datasource::FlowField f;
      const int err = src.getFlow(id, f) | src.getBW(id, A, B) | src.getOcclusion(id, oS) | src.getOcclusion(id + 1, oT) |
                      src.getInvalid(id, iS) | src.getInvalid(id + 1, iT);
      if (err || f.height != A.rows() || f.width < A.cols() - 15 || f.width > A.cols()) {
        std::cout << "ERR: " << scene << "/" << gpc::datasource::detail::frameName(id) << ": ground truth missing or short, skipped" << std::endl;
        if (!flush()) return 2;
        continue;
      }
      if (!have) {
        fm = forest.readForest(forestPath, A.cols(), A.rows());
        have = true;
      }
      if (frames.empty()) frames.push_back(A);
      frames.push_back(B);
      truths.push_back(Truth::fromFlow(f, oS, oT, iS, iT).resized(A.cols(), A.rows()));
      names.push_back(scene + "/" + gpc::datasource::detail::frameName(id));
      if (frames.size() >= 16 && !flush()) return 2;
    }
    if (!flush()) return 2;
  }
  printf("frames %d\n", scored);
  printScore("TOTAL", total, thr);
  return 0;
}
