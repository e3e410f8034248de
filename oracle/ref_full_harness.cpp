// ref_full_harness.cpp -- C-ABI wrappers around the reference's own Forest, Fern, Feature and
// Buffer classes.
//
// TEST INFRASTRUCTURE ONLY.  Where ref_harness.cpp exports the raw-pointer kernels of
// filter.hpp, this translation unit includes gpc/inference.hpp, gpc/training.hpp and
// gpc/buffer.hpp of the reference tree where they lie (nothing is copied into this
// repository) and drives the glue between those kernels, so that oracle/gpc_oracle.c and
// gpc_oracle_train.c can be held to it: readForest, preprocessImage with its 13-pixel margin,
// evalFastMaskOnSubsetSSE, depthPriorFast, findCorrespondences, stereoMatch, rectifiedMatch,
// Fern::evalSplit / markSplitSamples, Feature::getDecisions and getDisparityVisualization.
//
// Those headers include <Eigen/Dense> and use it as a container only; the build puts
// oracle/eigen_standin (an own-written stand-in, see its header) on the include path of the
// _ref targets and of nothing else.
//
// Image widths must be multiples of 16 (ndb::Buffer pads its rows to that; the reference's
// kernels take cols() as the stride).  Every wrapper cites the reference lines it calls.  The
// reference prints progress on std::cout; the wrappers park its stream buffer while they run.
//
// Build: oracle/Makefile, targets _ref/libgpc_ref_full.so (-D_INTRINSICS_SSE, the reference's
// default) and _ref/libgpc_ref_full_naive.so (its SSE=OFF build).
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "gpc/inference.hpp"
#include "gpc/training.hpp"

namespace {

struct Quiet {  // the reference's cout chatter (inference.hpp:413, Fern.hpp:321) goes nowhere
  std::streambuf* old;
  Quiet() : old(std::cout.rdbuf(nullptr)) {}
  ~Quiet() {
    std::cout.rdbuf(old);
    std::cout.clear();
  }
};

typedef gpc::inference::Forest Forest;
typedef gpc::inference::InferenceSettings Settings;

Settings make_settings(int thr, int disp_high, int vtol, int epipolar, int hashtable) {
  return Settings((uint8_t)thr, disp_high, vtol, epipolar != 0, hashtable != 0, 1);  // inference.hpp:92-97
}

ndb::Buffer<uint8_t> image(const uint8_t* px, int W, int H) {
  ndb::Buffer<uint8_t> b(H, W);  // buffer.hpp:152
  memcpy(b.data(), px, (size_t)W * H);
  return b;
}

Forest::PreprocessedImage pre_from(const uint8_t* smooth, const uint8_t* grad, const int32_t* mask, int n, int W,
                                   int H) {
  ndb::Buffer<uint8_t> s = image(smooth, W, H), g = image(grad, W, H);
  std::vector<int> m(mask, mask + n);
  return Forest::PreprocessedImage(s, g, m);  // inference.hpp:160
}

struct MatchOut {  // caller-owned arrays; capacities: states nl / nr, corr and supp max(nl, nr, 1)
  uint64_t* states_l;
  uint64_t* states_r;
  int32_t* corr;  // sx, sy, tx, ty
  int32_t* n_corr;
  int32_t* supp_xy;  // x, y
  float* supp_d;
  int32_t* n_supp;
  uint64_t* sorted_t_state;  // sort matcher: the target array as findCorrespondences left it
  int32_t* sorted_t_xy;
};

// Returns 0, or 1 where the reference is undefined and nothing was matched (sort matcher, source
// candidates but no target candidate: tarStates.size() - 1 on an empty vector bounds the search of
// inference.hpp:243, which then reads tarStates[0]; without source candidates the loop of :236 never
// gets there and the call is defined), or 2 when stereoMatch and a direct findCorrespondences call on
// the same descriptors disagree.
int run_match(Forest& F, Forest::PreprocessedImage& L, Forest::PreprocessedImage& R, Forest::FilterMask& fm,
              Settings st, const MatchOut& o) {
  // inference.hpp:266 -- the descriptor level
  std::vector<ndb::Descriptor> dl = F.evalFastMaskOnSubsetSSE(L.smooth, L.grad, L.mask, fm, st);
  std::vector<ndb::Descriptor> dr = F.evalFastMaskOnSubsetSSE(R.smooth, R.grad, R.mask, fm, st);
  for (size_t i = 0; i < dl.size(); ++i) o.states_l[i] = dl[i].state;
  for (size_t i = 0; i < dr.size(); ++i) o.states_r[i] = dr[i].state;
  *o.n_corr = 0;
  *o.n_supp = 0;
  if (!st.useHashtable_ && dr.empty() && !dl.empty()) return 1;
  // inference.hpp:351 -- the unfiltered level
  std::vector<ndb::Correspondence> corr = F.stereoMatch(L, R, fm, st);
  for (size_t i = 0; i < corr.size(); ++i) {
    o.corr[4 * i] = corr[i].srcPt.x;
    o.corr[4 * i + 1] = corr[i].srcPt.y;
    o.corr[4 * i + 2] = corr[i].tarPt.x;
    o.corr[4 * i + 3] = corr[i].tarPt.y;
  }
  *o.n_corr = (int32_t)corr.size();
  // inference.hpp:383 -- the support level
  std::vector<ndb::Support> supp = F.rectifiedMatch(L, R, fm, st);
  for (size_t i = 0; i < supp.size(); ++i) {
    o.supp_xy[2 * i] = supp[i].x;
    o.supp_xy[2 * i + 1] = supp[i].y;
    o.supp_d[i] = supp[i].d;
  }
  *o.n_supp = (int32_t)supp.size();
  if (!st.useHashtable_) {
    // inference.hpp:228 called as depthPriorFast does (:195-204); it sorts its arguments in
    // place, which is how the caller gets to see the reference's own sorted target array
    if (st.epipolarMode_) {
      for (auto& e : dl) e.state |= uint64_t(e.point.y) << 32;
      for (auto& e : dr) e.state |= uint64_t(e.point.y) << 32;
    }
    std::vector<ndb::Correspondence> direct;
    if (!dl.empty()) direct = F.findCorrespondences(dl, dr);
    for (size_t i = 0; i < dr.size(); ++i) {
      o.sorted_t_state[i] = dr[i].state;
      o.sorted_t_xy[2 * i] = dr[i].point.x;
      o.sorted_t_xy[2 * i + 1] = dr[i].point.y;
    }
    if (direct.size() != corr.size()) return 2;
    for (size_t i = 0; i < corr.size(); ++i)
      if (direct[i].srcPt.x != corr[i].srcPt.x || direct[i].srcPt.y != corr[i].srcPt.y ||
          direct[i].tarPt.x != corr[i].tarPt.x || direct[i].tarPt.y != corr[i].tarPt.y)
        return 2;
  }
  return 0;
}

typedef gpc::training::Feature::GPCPatchTriplet Triplet;
typedef gpc::training::Feature::params SplitParams;

// triplets: n * 3 * 729 bytes (ref, pos, neg), the file order of Feature.hpp:247-256; marks: bit 0 =
// pos.split, bit 1 = neg.split
std::vector<Triplet> make_triplets(const uint8_t* t, const uint8_t* marks, int n) {
  std::vector<Triplet> v(n);
  for (int i = 0; i < n; ++i) {
    gpc::training::Feature::GPCDescriptor* d[3] = {&v[i].ref, &v[i].pos, &v[i].neg};
    for (int k = 0; k < 3; ++k) {
      d[k]->feature.resize(27, 27);  // as loadAllTriplets does, Feature.hpp:283-289
      memcpy(d[k]->feature.data(), t + ((size_t)i * 3 + k) * 729, 729);
    }
    v[i].pos.split = (marks[i] & 1) != 0;
    v[i].neg.split = (marks[i] & 2) != 0;
  }
  return v;
}

std::vector<SplitParams> make_params(const int32_t* ijt, int n) {
  std::vector<SplitParams> p(n);
  for (int i = 0; i < n; ++i) {
    p[i].i = ijt[3 * i];
    p[i].j = ijt[3 * i + 1];
    p[i].tau = ijt[3 * i + 2];
  }
  return p;
}

}  // namespace

extern "C" {

int gpc_reff_is_sse(void) {
#ifdef _INTRINSICS_SSE
  return 1;
#else
  return 0;
#endif
}

// inference.hpp:402 -- offs: 64 ints, taus: 32 ints; counts as the reference's vectors have them
// (a zero forest comes back with no tau vector at all, :437-440)
int gpc_reff_read_forest(const char* path, int W, int H, int32_t* offs, int32_t* taus, int32_t* n_offs,
                         int32_t* n_taus, int32_t* type) {
  Quiet q;
  Forest F;
  Forest::FilterMask fm = F.readForest(path, W, H);
  if (fm.mask.size() > 64 || fm.tau.size() > 32) return -1;
  for (size_t i = 0; i < fm.mask.size(); ++i) offs[i] = fm.mask[i];
  for (size_t i = 0; i < fm.tau.size(); ++i) taus[i] = fm.tau[i];
  *n_offs = (int32_t)fm.mask.size();
  *n_taus = (int32_t)fm.tau.size();
  *type = fm.type;
  return (fm.width == W && fm.height == H) ? 0 : -2;
}

// inference.hpp:298 -- smooth, grad: W*H bytes; mask: capacity W*H; returns the candidate count
int gpc_reff_preprocess(const uint8_t* raw, int W, int H, int thr, uint8_t* smooth, uint8_t* grad, int32_t* mask) {
  if (W % 16) return -1;
  Quiet q;
  Forest F;
  ndb::Buffer<uint8_t> img = image(raw, W, H);
  Forest::PreprocessedImage p = F.preprocessImage(img, make_settings(thr, 128, 0, 0, 0));
  memcpy(smooth, p.smooth.data(), (size_t)W * H);
  memcpy(grad, p.grad.data(), (size_t)W * H);
  for (size_t i = 0; i < p.mask.size(); ++i) mask[i] = p.mask[i];
  return (int)p.mask.size();
}

// readForest -> rectifiedMatch on preprocessed images handed in as arrays (inference.hpp:402, :266,
// :351, :383, :228); see run_match for the return value
int gpc_reff_match_pre(const uint8_t* smooth_l, const uint8_t* grad_l, const int32_t* mask_l, int nl,
                       const uint8_t* smooth_r, const uint8_t* grad_r, const int32_t* mask_r, int nr, int W, int H,
                       const char* forest_path, int thr, int disp_high, int vtol, int epipolar, int hashtable,
                       MatchOut* out) {
  if (W % 16) return -1;
  Quiet q;
  Forest F;
  Forest::FilterMask fm = F.readForest(forest_path, W, H);
  Forest::PreprocessedImage L = pre_from(smooth_l, grad_l, mask_l, nl, W, H);
  Forest::PreprocessedImage R = pre_from(smooth_r, grad_r, mask_r, nr, W, H);
  return run_match(F, L, R, fm, make_settings(thr, disp_high, vtol, epipolar, hashtable), *out);
}

// the timed region of samples/sparsematch.cpp:45-52 after readForest: preprocessImage x2
// (inference.hpp:298), then as above.  mask_l / mask_r: capacity W*H, counts in n_cand[2]; the
// output arrays of `out` need capacity W*H as the counts are not known beforehand.
int gpc_reff_match_pair(const uint8_t* raw_l, const uint8_t* raw_r, int W, int H, const char* forest_path, int thr,
                        int disp_high, int vtol, int epipolar, int hashtable, int32_t* mask_l, int32_t* mask_r,
                        int32_t* n_cand, MatchOut* out) {
  if (W % 16) return -1;
  Quiet q;
  Forest F;
  Forest::FilterMask fm = F.readForest(forest_path, W, H);
  Settings st = make_settings(thr, disp_high, vtol, epipolar, hashtable);
  ndb::Buffer<uint8_t> il = image(raw_l, W, H), ir = image(raw_r, W, H);
  Forest::PreprocessedImage L = F.preprocessImage(il, st);
  Forest::PreprocessedImage R = F.preprocessImage(ir, st);
  for (size_t i = 0; i < L.mask.size(); ++i) mask_l[i] = L.mask[i];
  for (size_t i = 0; i < R.mask.size(); ++i) mask_r[i] = R.mask[i];
  n_cand[0] = (int32_t)L.mask.size();
  n_cand[1] = (int32_t)R.mask.size();
  return run_match(F, L, R, fm, st, *out);
}

// inference.hpp:228 on bare (state, linear index) sets; both arrays come back sorted as std::sort
// left them.  corr: capacity ns, 2 ints (source k, target k) per record.  nt == 0 with ns > 0 is refused (-1).
int gpc_reff_find_correspondences(uint64_t* ss, int32_t* sk, int ns, uint64_t* ts, int32_t* tk, int nt,
                                  int32_t* corr) {
  if (nt <= 0 && ns > 0) return -1;
  Forest F;
  std::vector<ndb::Descriptor> S(ns), T(nt);
  for (int i = 0; i < ns; ++i) S[i] = ndb::Descriptor(ndb::Point(sk[i], 0), ss[i]);
  for (int i = 0; i < nt; ++i) T[i] = ndb::Descriptor(ndb::Point(tk[i], 0), ts[i]);
  std::vector<ndb::Correspondence> c = F.findCorrespondences(S, T);
  for (int i = 0; i < ns; ++i) { ss[i] = S[i].state; sk[i] = S[i].point.x; }
  for (int i = 0; i < nt; ++i) { ts[i] = T[i].state; tk[i] = T[i].point.x; }
  for (size_t i = 0; i < c.size(); ++i) {
    corr[2 * i] = c[i].srcPt.x;
    corr[2 * i + 1] = c[i].tarPt.x;
  }
  return (int)c.size();
}

// Fern.hpp:209 -- params: (i, j, tau) triples, at least score_until_level + 1 of them; stats: four
// doubles (prec, rec, hmean, convcomb) and four ints (tp, fp, fn, tot)
void gpc_reff_eval_split(const uint8_t* triplets, const uint8_t* marks, int n, const int32_t* params, int nparams,
                         int score_until_level, double w1, double* stats_d, int32_t* stats_i) {
  Quiet q;
  std::vector<Triplet> data = make_triplets(triplets, marks, n);
  std::vector<SplitParams> p = make_params(params, nparams);
  gpc::training::FernSettings fs(nparams, 0);
  gpc::training::Fern fern(fs);
  gpc::training::splitStats s;
  fern.evalSplit(data, p, fs, gpc::training::OptimizerSettings(0, 1, 1, false, w1), score_until_level, s);
  stats_d[0] = s.prec;
  stats_d[1] = s.rec;
  stats_d[2] = s.hmean;
  stats_d[3] = s.convcomb;
  stats_i[0] = s.tp;
  stats_i[1] = s.fp;
  stats_i[2] = s.fn;
  stats_i[3] = s.tot;
}

// Fern.hpp:271 -- marks are updated in place
void gpc_reff_mark_split_samples(const uint8_t* triplets, uint8_t* marks, int n, const int32_t* params,
                                 int num_params) {
  Quiet q;
  std::vector<Triplet> data = make_triplets(triplets, marks, n);
  std::vector<SplitParams> p = make_params(params, num_params);
  gpc::training::Fern fern(gpc::training::FernSettings(num_params, 0));
  fern.markSplitSamples(data, p, num_params);
  for (int i = 0; i < n; ++i) marks[i] = (uint8_t)((data[i].pos.split ? 1 : 0) | (data[i].neg.split ? 2 : 0));
}

// Feature.hpp:101 -- one triplet (3 * 729 bytes), one test; out: ref, pos, neg decisions
void gpc_reff_get_decisions(const uint8_t* triplet, int i, int j, int tau, uint8_t* out) {
  const uint8_t none = 0;
  std::vector<Triplet> data = make_triplets(triplet, &none, 1);
  gpc::training::Feature f;
  SplitParams p;
  p.i = i;
  p.j = j;
  p.tau = tau;
  bool r, a, b;
  f.getDecisions(r, a, b, p, data[0]);
  out[0] = r;
  out[1] = a;
  out[2] = b;
}

// buffer.hpp:949 -- img: W*H gray bytes; supports: n (x, y) pairs and n disparities; rgb: W*H*3 bytes
int gpc_reff_disparity_vis(const uint8_t* img, int W, int H, const int32_t* xy, const float* d, int n, uint8_t* rgb) {
  if (W % 16) return -1;
  ndb::Buffer<uint8_t> src = image(img, W, H);
  std::vector<ndb::Support> supp;
  for (int i = 0; i < n; ++i) supp.push_back(ndb::Support(xy[2 * i], xy[2 * i + 1], d[i]));
  ndb::Buffer<ndb::RGBColor> vis = ndb::getDisparityVisualization(src, supp);
  if (vis.cols() != W || vis.rows() != H) return -2;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const ndb::RGBColor c = vis.getPixel(x, y);
      rgb[3 * ((size_t)y * W + x)] = c.r;
      rgb[3 * ((size_t)y * W + x) + 1] = c.g;
      rgb[3 * ((size_t)y * W + x) + 2] = c.b;
    }
  return 0;
}

}  // extern "C"
