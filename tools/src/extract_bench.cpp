// extract_bench -- times training-set extraction for N synthetic 1024x436 frame pairs x K triplets (tools/extract_bench.py):
//   device: gpc_hip_extract_triplets from host memory (upload + smooth + gather), and from frames already in HBM
//           (gpc_hip_extract_triplets_device: smooth + gather);
//   host:   Feature::extractAllTriplets frame by frame (smoothing on the GPU, patches cut into ndb::Buffers) + the
//           packing and gpc_hip_train_set_create that detail::DeviceTriplets does before any scoring.
// usage: extract_bench <pairs> <triplets per pair> <reps>      prints one "RESULT key value" line per number (ms)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gpc/training.hpp"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? std::atoi(argv[1]) : 32, K = argc > 2 ? std::atoi(argv[2]) : 1000, reps = argc > 3 ? std::atoi(argv[3]) : 3;
  const int W = 1024, H = 436;
  const size_t npx = (size_t)W * H;
  std::mt19937 rng(1);
  std::vector<uint8_t> L(npx * N), R(npx * N);
  for (size_t i = 0; i < L.size(); ++i) {
    L[i] = (uint8_t)(rng() >> 24);
    R[i] = (uint8_t)(rng() >> 24);
  }
  std::vector<gpc_triplet_points> pts((size_t)N * K);
  std::vector<int32_t> first(N + 1);
  std::uniform_int_distribution<int> rx(21, W - 22), ry(21, H - 22);
  for (int f = 0; f <= N; ++f) first[f] = f * K;
  for (auto& p : pts) p = gpc_triplet_points{rx(rng), ry(rng), rx(rng), ry(rng), rx(rng), ry(rng)};
  gpc_hip_ctx* ctx = gpc::inference::detail::holder().ctx;
  if (!ctx) return 1;
  uint8_t *dL = nullptr, *dR = nullptr;
  if (hipMalloc((void**)&dL, L.size()) != hipSuccess || hipMalloc((void**)&dR, R.size()) != hipSuccess) return 1;
  (void)hipMemcpy(dL, L.data(), L.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dR, R.data(), R.size(), hipMemcpyHostToDevice);
  double best_host_in = 1e30, best_dev_in = 1e30, best_feat = 1e30, best_create = 1e30;
  for (int r = 0; r <= reps; ++r) {  // rep 0 warms up
    gpc_hip_train_set* set = nullptr;
    int n = 0;
    double t0 = now_ms();
    if (gpc_hip_extract_triplets(ctx, L.data(), R.data(), W, H, N, pts.data(), first.data(), nullptr, &set, &n) || n != N * K) return 2;
    double t1 = now_ms();
    gpc_hip_train_set_destroy(ctx, set);
    double t2 = now_ms();
    if (gpc_hip_extract_triplets_device(ctx, dL, dR, W, H, N, pts.data(), first.data(), nullptr, &set, &n) || n != N * K) return 3;
    double t3 = now_ms();
    gpc_hip_train_set_destroy(ctx, set);
    // the host path
    gpc::training::Feature feature;
    std::vector<gpc::training::Feature::GPCPatchTriplet> triplets;
    triplets.reserve((size_t)N * K);
    double t4 = now_ms();
    for (int f = 0; f < N; ++f) {
      ndb::Buffer<uint8_t> bl = ndb::Buffer<uint8_t>::uninitialized(H, W), br = ndb::Buffer<uint8_t>::uninitialized(H, W);
      std::memcpy(bl.data(), &L[f * npx], npx);
      std::memcpy(br.data(), &R[f * npx], npx);
      std::vector<ndb::Point> a, b, c;
      for (int k = first[f]; k < first[f + 1]; ++k) {
        a.emplace_back(pts[k].rx, pts[k].ry);
        b.emplace_back(pts[k].px, pts[k].py);
        c.emplace_back(pts[k].nx, pts[k].ny);
      }
      feature.extractAllTriplets(bl, br, a, b, c, triplets);
    }
    double t5 = now_ms();
    {
      gpc::training::detail::DeviceTriplets dev(triplets);
      (void)gpc_hip_synchronize(dev.ctx());
    }
    double t6 = now_ms();
    if (r == 0) continue;
    best_host_in = std::min(best_host_in, t1 - t0);
    best_dev_in = std::min(best_dev_in, t3 - t2);
    best_feat = std::min(best_feat, t5 - t4);
    best_create = std::min(best_create, t6 - t5);
  }
  std::printf("RESULT pairs %d\nRESULT triplets_per_pair %d\n", N, K);
  std::printf("RESULT device_from_host_ms %.3f\nRESULT device_from_hbm_ms %.3f\n", best_host_in, best_dev_in);
  std::printf("RESULT host_extract_all_triplets_ms %.3f\nRESULT host_train_set_create_ms %.3f\n", best_feat, best_create);
  (void)hipFree(dL);
  (void)hipFree(dR);
  return 0;
}
