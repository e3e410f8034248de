// aggregate.hpp -- the scanline aggregation of the search's costs (extension; the reference stops at sparse supports): the
// candidates and the SAD costs of gpc/search.hpp, but before the choice a smoothness term is added along scanlines, as the
// path aggregation of semi-global matching does: a candidate whose displacement differs from the neighbour's best by one
// pixel pays p1, by more p2.  Integers only, run on the device by gpc_hip_aggregate_fields (include/gpc_hip.h has the rule).
//
//   gpc::aggregate::Params                             radius, range, subpixel, maxCost as gpc::search; p1, p2, paths
//   gpc::aggregate::Result                             field, cost (raw), choice, stats as gpc::search; sum
//   gpc::aggregate::aggregate(field, left, right, p)   one Result from a filled field and the image pair
//
// It stands where the search stands, between the fill and the cleaner; the backward field takes the images exchanged:
//   Field fwd = gpc::dense::densify(supports, w, h), bwd = gpc::dense::densify(gpc::clean::reversed(supports), w, h);
//   fwd = gpc::aggregate::aggregate(fwd, L, R).field, bwd = gpc::aggregate::aggregate(bwd, R, L).field;
//   gpc::clean::Result r = gpc::clean::clean(fwd, &bwd);
// Errors are reported as everywhere in inference.hpp: an empty Result and lastStatus() / lastError().
#ifndef GPC_AMD_AGGREGATE_HPP
#define GPC_AMD_AGGREGATE_HPP

#include <cstdint>
#include <vector>

#include "gpc/dense.hpp"

namespace gpc {
namespace aggregate {

enum Path { Right = 1, Left = 2, Down = 4, Up = 8 };  // the way a path runs: left to right, right to left, top to bottom, bottom to top

struct Params {
  int radius = 2;         // the window is (2 radius + 1)^2; 1 .. 4
  int range = 1;          // candidates within this many whole pixels of the prior; 0 .. 2, 0: verify only
  bool subpixel = true;   // the parabola of gpc::refine per axis
  int maxCost = 0xFFFF;   // a best raw cost above it rejects the pixel; 0xFFFF: no ceiling
  int p1 = 128, p2 = 512;   // the penalties of a displacement one pixel off the neighbour's, and further off; 0 <= p1 <= p2 <= 32767
  int paths = Right | Left | Down | Up;
  gpc_aggregate toC() const { return gpc_aggregate{radius, range, subpixel ? 1 : 0, maxCost, p1, p2, paths}; }
};

enum Stat { Kept = 0, Hole = 1, Unmatched = 2, Rejected = 3 };

struct Result {
  gpc::dense::Field field;        // the chosen values; GPC_DENSE_NONE for holes, unmatched and rejected pixels
  ndb::Buffer<uint16_t> cost;     // the best candidate's cost, also of a rejected pixel; 0xFFFF for holes and unmatched pixels
  ndb::Buffer<uint8_t> choice;    // (ky + range) (2 range + 1) + (kx + range), kx + range for a disparity; 255 likewise
  ndb::Buffer<uint32_t> sum;      // the best candidate's aggregated cost; 0xFFFFFFFF for holes and unmatched pixels
  int32_t stats[4] = {0, 0, 0, 0};  // pixels per Stat
  bool empty() const { return field.empty(); }
};

inline Result aggregate(const gpc::dense::Field& f, const ndb::Buffer<uint8_t>& left, const ndb::Buffer<uint8_t>& right,
                     const Params& p = Params()) {
  namespace inf = gpc::inference;
  const bool shaped = !f.empty() && f.width >= 1 && f.height >= 1 && (int)f.value.size() == f.channels && left.cols() == f.width &&
                      left.rows() == f.height && right.cols() == f.width && right.rows() == f.height;
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_aggregate_fields");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int W = f.width, H = f.height, C = f.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> in((size_t)C * n), out((size_t)C * n);
  std::vector<uint8_t> l(n), r(n), choice(n);
  std::vector<uint16_t> cost(n);
  std::vector<uint32_t> sum(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      l[at] = left(y, x), r[at] = right(y, x);
      for (int c = 0; c < C; ++c) in[(size_t)c * n + at] = f.value[(size_t)c](y, x);
    }
  const gpc_aggregate prm = p.toC();
  Result res;
  const int st = gpc_hip_aggregate_fields(h.ctx, in.data(), l.data(), r.data(), C, W, H, 1, &prm, out.data(), cost.data(),
                                          choice.data(), res.stats, sum.data());
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_aggregate_fields");
    return Result();
  }
  res.field.width = W, res.field.height = H, res.field.channels = C;
  res.field.level = f.level;
  res.cost = ndb::Buffer<uint16_t>(H, W);
  res.choice = ndb::Buffer<uint8_t>(H, W);
  res.sum = ndb::Buffer<uint32_t>(H, W);
  for (int c = 0; c < C; ++c) res.field.value.emplace_back(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      res.cost(y, x) = cost[at];
      res.choice(y, x) = choice[at];
      res.sum(y, x) = sum[at];
      for (int c = 0; c < C; ++c) res.field.value[(size_t)c](y, x) = out[(size_t)c * n + at];
    }
  return res;
}

}  // namespace aggregate
}  // namespace gpc
#endif
