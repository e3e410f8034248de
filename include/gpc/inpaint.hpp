// inpaint.hpp -- completing a cleaned dense field, guided by the image (extension; the reference writes disparity.png from
// the raw supports): a pixel without a value takes the weighted mean of the valued pixels in its window, and neighbours that
// look like it in the guide count more; integers only, run on the device by gpc_hip_inpaint_fields (include/gpc_hip.h has the
// rule).
//
//   gpc::inpaint::Params                         radius, rangeShift, minWeight, passes
//   gpc::inpaint::Result                         field (the completed values), pass, stats
//   gpc::inpaint::reference(field, guide, ...)   the rule restated on the CPU over plain arrays: what the device must give
//   gpc::inpaint::inpaint(field, guide, params)  one Result from a (cleaned) field and the left image, or frame t
//
//   gpc::clean::Result c = gpc::clean::clean(fwd, &bwd);
//   gpc::inpaint::Result r = gpc::inpaint::inpaint(c.field, left);
// Errors are reported as everywhere in inference.hpp: an empty Result and lastStatus() / lastError().
// With GPC_INPAINT_RULE_ONLY defined the header gives Params, weight, mean and reference alone and needs nothing but
// gpc_hip.h: no library to link, so a stand-alone program can run the rule under the sanitizers.
#ifndef GPC_AMD_INPAINT_HPP
#define GPC_AMD_INPAINT_HPP

#include <cstdint>
#include <vector>

#ifdef GPC_INPAINT_RULE_ONLY
#include "gpc_hip.h"
#else
#include "gpc/dense.hpp"
#endif

namespace gpc {
namespace inpaint {

struct Params {
  int radius = 4;       // 1 .. 8: the window is (2 radius + 1)^2, clipped to the image
  int rangeShift = 3;   // 0 .. 8: a neighbour's weight halves per 2^rangeShift grey levels of difference; 8: unguided
  int minWeight = 512;  // 1 .. 2^24: the total weight a hole needs before it is filled (a neighbour weighs at most 256)
  int passes = 32;      // 1 .. 254
  gpc_inpaint toC() const { return gpc_inpaint{radius, rangeShift, minWeight, passes}; }
};

#ifndef GPC_INPAINT_RULE_ONLY
struct Result {
  gpc::dense::Field field;     // the completed field; GPC_DENSE_NONE where a hole is left
  ndb::Buffer<uint8_t> pass;   // 0: valued on input; k: filled in pass k; 255: left a hole
  int32_t stats[2] = {0, 0};   // pixels filled, holes left
  bool empty() const { return field.empty(); }
};
#endif

// 256 >> min(8, |a - b| >> shift): 1 .. 256
inline int32_t weight(int a, int b, int shift) {
  const int d = a < b ? b - a : a - b, s = d >> shift;
  return 256 >> (s < 8 ? s : 8);
}

// sgn(S) * ((2 |S| + Wt) div (2 Wt)): half away from zero
inline int32_t mean(int64_t S, int64_t Wt) {
  const uint64_t a = S < 0 ? (uint64_t)0 - (uint64_t)S : (uint64_t)S, q = (2 * a + (uint64_t)Wt) / (2 * (uint64_t)Wt);
  return (int32_t)(S < 0 ? -(int64_t)q : (int64_t)q);
}

// The rule, restated plainly for one pair: field [C][H][W] and guide [H][W] -> out [C][H][W], pass [H][W], stats [2].
// Every pass scans the state of the pass before and commits afterwards.
inline void reference(const int32_t* field, const uint8_t* guide, int C, int W, int H, const Params& p, int32_t* out, uint8_t* pass,
                      int32_t* stats) {
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> F(field, field + (size_t)C * n);
  std::vector<uint8_t> pz(n);
  for (size_t i = 0; i < n; ++i) pz[i] = F[i] == GPC_DENSE_NONE ? 255 : 0;
  struct Fill {
    size_t at;
    int32_t v[2];
  };
  std::vector<Fill> fills;
  for (int k = 1; k <= p.passes; ++k) {
    fills.clear();
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t at = (size_t)y * W + x;
        if (pz[at] != 255) continue;
        int64_t Wt = 0, S[2] = {0, 0};
        for (int qy = y - p.radius < 0 ? 0 : y - p.radius; qy <= y + p.radius && qy < H; ++qy)
          for (int qx = x - p.radius < 0 ? 0 : x - p.radius; qx <= x + p.radius && qx < W; ++qx) {
            const size_t q = (size_t)qy * W + qx;
            if (pz[q] == 255) continue;
            const int64_t w = weight(guide[at], guide[q], p.rangeShift);
            Wt += w;
            for (int c = 0; c < C; ++c) S[c] += w * (int64_t)F[(size_t)c * n + q];
          }
        if (Wt >= p.minWeight) {
          Fill f{at, {0, 0}};
          for (int c = 0; c < C; ++c) f.v[c] = mean(S[c], Wt);
          fills.push_back(f);
        }
      }
    if (fills.empty()) break;
    for (const Fill& f : fills) {
      pz[f.at] = (uint8_t)k;
      for (int c = 0; c < C; ++c) F[(size_t)c * n + f.at] = f.v[c];
    }
  }
  int32_t filled = 0, left = 0;
  for (size_t i = 0; i < n; ++i) {
    filled += pz[i] > 0 && pz[i] < 255;
    left += pz[i] == 255;
    for (int c = 0; c < C; ++c) out[(size_t)c * n + i] = pz[i] == 255 ? GPC_DENSE_NONE : F[(size_t)c * n + i];
    if (pass) pass[i] = pz[i];
  }
  if (stats) stats[0] = filled, stats[1] = left;
}

#ifndef GPC_INPAINT_RULE_ONLY
inline Result inpaint(const gpc::dense::Field& field, const ndb::Buffer<uint8_t>& guide, const Params& p = Params()) {
  namespace inf = gpc::inference;
  const bool shaped = !field.empty() && field.width >= 1 && field.height >= 1 && (int)field.value.size() == field.channels &&
                      guide.cols() == field.width && guide.rows() == field.height;
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_inpaint_fields");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int W = field.width, H = field.height, C = field.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> f((size_t)C * n), out((size_t)C * n);
  std::vector<uint8_t> g(n), pass(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      g[at] = guide(y, x);
      for (int c = 0; c < C; ++c) f[(size_t)c * n + at] = field.value[(size_t)c](y, x);
    }
  const gpc_inpaint prm = p.toC();
  Result r;
  const int st = gpc_hip_inpaint_fields(h.ctx, f.data(), g.data(), C, W, H, 1, &prm, out.data(), pass.data(), r.stats);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_inpaint_fields");
    return Result();
  }
  r.field.width = W, r.field.height = H, r.field.channels = C;
  r.field.level = field.level;
  r.pass = ndb::Buffer<uint8_t>(H, W);
  for (int c = 0; c < C; ++c) r.field.value.emplace_back(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      r.pass(y, x) = pass[at];
      for (int c = 0; c < C; ++c) r.field.value[(size_t)c](y, x) = out[(size_t)c * n + at];
    }
  return r;
}
#endif

}  // namespace inpaint
}  // namespace gpc
#endif
