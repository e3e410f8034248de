// quads_check -- gpc::quads::closeRecords (include/gpc/quads.hpp) over records read from stdin, for tests/test_gpu_quads.py:
//   width height tol N, then per frame "m" and m supports "x y d", then per step and side (left, right) "m" and m
//   correspondences "sx sy tx ty".  Prints per step "step t n" and per quad its four points and two support indices.
#include <cstdio>
#include <vector>

#include "gpc/quads.hpp"

int main() {
  int W, H, tol, N;
  if (std::scanf("%d %d %d %d", &W, &H, &tol, &N) != 4 || N < 2) return 2;
  std::vector<std::vector<ndb::Support>> sup((size_t)N);
  std::vector<std::vector<ndb::Correspondence>> fl((size_t)N - 1), fr((size_t)N - 1);
  for (auto& s : sup) {
    int m;
    if (std::scanf("%d", &m) != 1) return 2;
    for (int i = 0; i < m; ++i) {
      int x, y;
      float d;
      if (std::scanf("%d %d %f", &x, &y, &d) != 3) return 2;
      s.push_back(ndb::Support(x, y, d));
    }
  }
  for (int t = 0; t < N - 1; ++t)
    for (auto* f : {&fl[(size_t)t], &fr[(size_t)t]}) {
      int m;
      if (std::scanf("%d", &m) != 1) return 2;
      for (int i = 0; i < m; ++i) {
        int a, b, c, d;
        if (std::scanf("%d %d %d %d", &a, &b, &c, &d) != 4) return 2;
        f->push_back(ndb::Correspondence(ndb::Point(a, b), ndb::Point(c, d)));
      }
    }
  const std::vector<std::vector<gpc::quads::Quad>> q = gpc::quads::closeRecords(sup, fl, fr, W, H, tol);
  if (gpc::inference::lastStatus() != GPC_OK) {
    std::printf("failed: %s\n", gpc::inference::lastError().c_str());
    return 1;
  }
  for (size_t t = 0; t < q.size(); ++t) {
    std::printf("step %zu %zu\n", t, q[t].size());
    for (const gpc::quads::Quad& k : q[t])
      std::printf("%d %d %d %d %d %d %d %d %d %d\n", k.l0.x, k.l0.y, k.r0.x, k.r0.y, k.l1.x, k.l1.y, k.r1.x, k.r1.y, k.support0, k.support1);
  }
  return 0;
}
