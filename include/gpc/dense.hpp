// dense.hpp -- dense disparity maps and flow fields from sparse matches (extension; the reference ends in disparity.png and
// leaves the interpolation of its matches to its caller).  A pixel with a match keeps it; a pixel without one takes the
// mean of the matches in the smallest aligned block around it that holds enough of them; integers only, run on the device
// by gpc_hip_densify_* (include/gpc_hip.h has the rule).
//
//   gpc::dense::Params                                   maxLevel, minCount, spread, maxCost (the documented defaults)
//   gpc::dense::Field                                    value planes in 1/256 pixel, level plane, float views
//   gpc::dense::densify(records, w, h, params)           one Field from the supports / correspondences of one pair
//   gpc::dense::densify(records, results, w, h, params)  ... with the sub-pixel shifts and costs of gpc::refine::refine
//
// Supports give one plane (the disparity), correspondences two (u, then v).  No forest is needed.  Errors are reported as
// everywhere in inference.hpp: an empty Field and lastStatus() / lastError().
#ifndef GPC_AMD_DENSE_HPP
#define GPC_AMD_DENSE_HPP

#include <cstdint>
#include <limits>
#include <vector>

#include "gpc/consensus.hpp"
#include "gpc/inference.hpp"
#include "gpc/refine.hpp"

namespace gpc {
namespace dense {

struct Params {
  int maxLevel = 15;      // 1 .. 15: the coarsest block a pixel may take its value from is 2^maxLevel pixels wide
  int minCount = 1;       // matches a block needs before it fills a pixel
  int spread = 1;         // 0: the pixel's own cell; 1: the 3x3 cells around it
  int maxCost = 0xFFFF;   // records dearer than this (gpc::refine::Result::cost) take no part; 0xFFFF: no ceiling
  gpc_densify toC() const { return gpc_densify{maxLevel, minCount, spread, maxCost}; }
};

struct Field {
  int width = 0, height = 0, channels = 0;
  std::vector<ndb::Buffer<int32_t>> value;  // [channels] planes in 1/256 pixel; GPC_DENSE_NONE where nothing fills the pixel
  ndb::Buffer<uint8_t> level;               // 0: the pixel's own match; l: filled from level l; 255: none
  bool empty() const { return channels == 0; }
  bool valid(int x, int y) const { return value[0](y, x) != GPC_DENSE_NONE; }
  // plane c in pixels, row-major width * height; NaN where nothing fills the pixel
  std::vector<float> asFloat(int c) const {
    std::vector<float> out((size_t)width * (size_t)height);
    for (int y = 0; y < height; ++y)
      for (int x = 0; x < width; ++x) {
        const int32_t v = value[(size_t)c](y, x);
        out[(size_t)y * width + x] = v == GPC_DENSE_NONE ? std::numeric_limits<float>::quiet_NaN() : (float)v / 256.f;
      }
    return out;
  }
};

namespace detail {
inline int call(gpc_hip_ctx* ctx, const gpc_correspondence* r, int cap, const int32_t* n, const gpc_refinement* ref, int w, int h,
                const gpc_densify* p, int32_t* value, uint8_t* level) {
  return gpc_hip_densify_correspondences(ctx, r, cap, n, ref, w, h, 1, p, value, level);
}
inline int call(gpc_hip_ctx* ctx, const gpc_support* r, int cap, const int32_t* n, const gpc_refinement* ref, int w, int h,
                const gpc_densify* p, int32_t* value, uint8_t* level) {
  return gpc_hip_densify_supports(ctx, r, cap, n, ref, w, h, 1, p, value, level);
}
inline gpc_refinement toC(const gpc::refine::Result& r) {
  gpc_refinement o;
  o.dx_q8 = (int16_t)(r.dx * 256.f), o.dy_q8 = (int16_t)(r.dy * 256.f);  // (exact: Result holds q8 / 256)
  o.cost = (uint16_t)r.cost;
  o.flags = (uint16_t)((r.evaluated ? 1 : 0) | (r.minimumX ? 2 : 0) | (r.minimumY ? 4 : 0));
  return o;
}

template <class Rec, class CRec, int C>
Field densifyOne(const std::vector<Rec>& records, const std::vector<gpc::refine::Result>* results, int width, int height,
                 const Params& p) {
  namespace inf = gpc::inference;
  if (results && results->size() != records.size()) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_densify");
    return Field();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Field();
  // (an empty list is a valid input: every pixel is none; the C call wants one slot)
  std::vector<CRec> rec(records.size() ? records.size() : 1);
  for (size_t i = 0; i < records.size(); ++i) rec[i] = gpc::consensus::detail::toC(records[i]);
  std::vector<gpc_refinement> ref;
  if (results) {
    ref.resize(rec.size());
    for (size_t i = 0; i < results->size(); ++i) ref[i] = toC((*results)[i]);
  }
  const int32_t n = (int32_t)records.size();
  const gpc_densify prm = p.toC();
  const bool sized = width >= 1 && height >= 1;
  std::vector<int32_t> value(sized ? (size_t)C * width * height : 1);
  std::vector<uint8_t> level(sized ? (size_t)width * height : 1);
  const int st = call(h.ctx, rec.data(), (int)rec.size(), &n, results ? ref.data() : nullptr, width, height, &prm, value.data(),
                      level.data());
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_densify");
    return Field();
  }
  Field f;
  f.width = width, f.height = height, f.channels = C;
  f.level = ndb::Buffer<uint8_t>(height, width);
  for (int c = 0; c < C; ++c) f.value.emplace_back(height, width);
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const size_t at = (size_t)y * width + x;
      f.level(y, x) = level[at];
      for (int c = 0; c < C; ++c) f.value[(size_t)c](y, x) = value[(size_t)c * width * height + at];
    }
  return f;
}
}  // namespace detail

inline Field densify(const std::vector<ndb::Support>& records, int width, int height, const Params& p = Params()) {
  return detail::densifyOne<ndb::Support, gpc_support, 1>(records, nullptr, width, height, p);
}
inline Field densify(const std::vector<ndb::Correspondence>& records, int width, int height, const Params& p = Params()) {
  return detail::densifyOne<ndb::Correspondence, gpc_correspondence, 2>(records, nullptr, width, height, p);
}
inline Field densify(const std::vector<ndb::Support>& records, const std::vector<gpc::refine::Result>& results, int width, int height,
                     const Params& p = Params()) {
  return detail::densifyOne<ndb::Support, gpc_support, 1>(records, &results, width, height, p);
}
inline Field densify(const std::vector<ndb::Correspondence>& records, const std::vector<gpc::refine::Result>& results, int width,
                     int height, const Params& p = Params()) {
  return detail::densifyOne<ndb::Correspondence, gpc_correspondence, 2>(records, &results, width, height, p);
}

}  // namespace dense
}  // namespace gpc
#endif
