// ref_sampler_check -- the reference's own sampler functions against gpc/SintelOpticalFlow.hpp and gpc/SintelStereo.hpp
// (tests/test_extract.py, where the reference tree is present).  The test copies the reference's isSafePatchCenter and the
// two getGroundTruthMatches bodies (SintelOpticalFlow.hpp:269-274, 478-558; SintelStereo.hpp:390-463) unchanged into
// ref_safe.inc / ref_flow_fn.inc / ref_stereo_fn.inc of a temporary directory at test time; this file only supplies what
// they use: a stand-in for Eigen::MatrixXd (u(x, y)), minimal ndb::Point / Buffer / RGBBuffer types, and a
// std::random_device that returns a fixed seed -- so the reference's code and these headers draw from the same
// std::mt19937 on the same fields and masks, compiled by the same g++.  Prints "SAME <trials>" or the first difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gpc/SintelOpticalFlow.hpp"
#include "gpc/SintelStereo.hpp"

static unsigned g_seed = 1;
namespace std {
struct fixed_seed_device {
  unsigned operator()() { return g_seed; }
};
}  // namespace std
namespace Eigen {
struct MatrixXd {
  int w = 0;
  std::vector<double> d;
  double& operator()(int x, int y) { return d[(size_t)y * w + x]; }
};
}  // namespace Eigen
namespace refndb {
struct RGBColor {
  uint8_t b, g, r;
};
struct Point {
  int x, y;
  Point(int a, int b) : x(a), y(b) {}
};
template <class T>
struct Buffer {
  int W = 1024;
  std::vector<T> v;
  T getPixel(int x, int y) { return v[(size_t)y * W + x]; }
};
typedef Buffer<RGBColor> RGBBuffer;
}  // namespace refndb

#define random_device fixed_seed_device
#define ndb refndb
struct RefFlow {
#include "ref_safe.inc"
#include "ref_flow_fn.inc"
};
struct RefStereo {
#include "ref_safe.inc"
#include "ref_stereo_fn.inc"
};
#undef ndb
#undef random_device

template <class A, class B>
static bool same(const std::vector<A>& a, const std::vector<B>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k)
    if (a[k].x != b[k].x || a[k].y != b[k].y) return false;
  return true;
}

int main() {
  const int W = 1024, H = 436, trials = 40, per = 300;
  std::mt19937 g(7);
  size_t total = 0;
  for (int trial = 0; trial < trials; ++trial) {
    g_seed = 1000 + trial;
    Eigen::MatrixXd u, v;
    u.w = v.w = W;
    u.d.resize(W * H);
    v.d.resize(W * H);
    gpc::datasource::FlowField ff;
    ff.width = W;
    ff.height = H;
    ff.u.resize(W * H);
    ff.v.resize(W * H);
    refndb::Buffer<uint8_t> m[4];
    ndb::Buffer<uint8_t> mm[4];
    for (int k = 0; k < 4; ++k) {
      m[k].v.resize(W * H);
      mm[k] = ndb::Buffer<uint8_t>(H, W);
    }
    refndb::RGBBuffer disp;
    disp.v.resize(W * H);
    ndb::RGBBuffer d2;
    static_cast<ndb::Buffer<ndb::RGBColor>&>(d2) = ndb::Buffer<ndb::RGBColor>(H, W);
    std::uniform_real_distribution<float> fl(-20.f, 20.f);
    std::uniform_int_distribution<int> occl(0, 9), byte(0, 255);
    for (int i = 0; i < W * H; ++i) {
      float a = (trial % 3 == 0) ? std::round(fl(g)) : fl(g), c = fl(g);
      if (i % 7 == 0) a = 0.5f;  // halfway cases of round()
      u.d[i] = a;
      v.d[i] = c;
      ff.u[i] = a;
      ff.v[i] = c;
      for (int k = 0; k < 4; ++k) {
        const uint8_t x = occl(g) == 0 ? 255 : 0;
        m[k].v[i] = x;
        mm[k](i / W, i % W) = x;
      }
      int r = byte(g) % 8, gg = byte(g);
      if (trial % 2) r = 0, gg = gg % 128;  // many d == 0 pixels
      disp.v[i].r = (uint8_t)r;
      disp.v[i].g = (uint8_t)gg;
      disp.v[i].b = 0;
      d2(i / W, i % W) = ndb::RGBColor((uint8_t)r, (uint8_t)gg, 0);
    }
    const int lo = 5 + trial % 10, hi = lo + 20 + trial;
    std::vector<refndb::Point> a1, a2, a3, c1, c2, c3;
    std::vector<ndb::Point> b1, b2, b3, e1, e2, e3;
    RefFlow().getGroundTruthMatches(u, v, m[0], m[1], m[2], m[3], per, lo, hi, a1, a2, a3);
    std::mt19937 r1(g_seed);
    gpc::datasource::SintelOpticalFlow().getGroundTruthMatches(ff, mm[0], mm[1], mm[2], mm[3], per, lo, hi, b1, b2, b3, r1);
    RefStereo().getGroundTruthMatches(disp, m[0], m[1], per, lo, hi, c1, c2, c3);
    std::mt19937 r2(g_seed);
    gpc::datasource::SintelStereo().getGroundTruthMatches(d2, mm[0], mm[1], per, lo, hi, e1, e2, e3, r2);
    if (!(same(a1, b1) && same(a2, b2) && same(a3, b3))) {
      std::printf("DIFF flow trial %d\n", trial);
      return 1;
    }
    if (!(same(c1, e1) && same(c2, e2) && same(c3, e3))) {
      std::printf("DIFF stereo trial %d\n", trial);
      return 1;
    }
    total += a1.size() + c1.size();
  }
  std::printf("SAME %d %zu\n", trials, total);
  return 0;
}
