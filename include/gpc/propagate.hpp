// propagate.hpp -- the propagation of field values between neighbours (extension; the reference stops at sparse supports):
// a pixel of a filled field tries the whole-pixel values of its neighbours, at strides that halve from `span` down to 1, and
// keeps whichever gives the smallest SAD between the two images.  It carries the value of the correct side of an object
// edge into the pixels the fill interpolated across it, which lie further from the truth than the search looks.  Integers
// only, run on the device by gpc_hip_propagate_fields (include/gpc_hip.h has the rule).
//
//   gpc::propagate::Params                             radius, span, iterations, neighbours
//   gpc::propagate::Result                             field (the propagated values), cost, choice, stats per iteration
//   gpc::propagate::propagate(field, left, right, p)   one Result from a filled field and the image pair
//
// It belongs between the fill and the search, which supplies the sub-pixel part:
//   Field f = gpc::dense::densify(supports, w, h);
//   f = gpc::propagate::propagate(f, L, R).field;
//   f = gpc::search::search(f, L, R).field;
// Errors are reported as everywhere in inference.hpp: an empty Result and lastStatus() / lastError().
#ifndef GPC_AMD_PROPAGATE_HPP
#define GPC_AMD_PROPAGATE_HPP

#include <cstdint>
#include <vector>

#include "gpc/dense.hpp"

namespace gpc {
namespace propagate {

struct Params {
  int radius = 2;      // the window is (2 radius + 1)^2; 1 .. 4
  int span = 1;        // the stride of the first iteration, halved from one iteration to the next down to 1; 1 .. 64
  int iterations = 6;  // 1 .. 16
  int neighbours = 8;  // 4, or 8 with the diagonals
  gpc_propagate toC() const { return gpc_propagate{radius, span, iterations, neighbours}; }
};

enum Stat { Own = 0, Hole = 1, Unmatched = 2, Moved = 3 };

struct Result {
  gpc::dense::Field field;        // the values after the last iteration; holes stay holes, and no value is removed
  ndb::Buffer<uint16_t> cost;     // the winner's cost in the last iteration; 0xFFFF for holes and unmatched pixels
  ndb::Buffer<uint8_t> choice;    // the winner's index in the last iteration, 0: the pixel's own value; 255 likewise
  std::vector<int32_t> stats;     // [iterations][4]: pixels per Stat
  bool empty() const { return field.empty(); }
};

inline Result propagate(const gpc::dense::Field& f, const ndb::Buffer<uint8_t>& left, const ndb::Buffer<uint8_t>& right,
                        const Params& p = Params()) {
  namespace inf = gpc::inference;
  const bool shaped = !f.empty() && f.width >= 1 && f.height >= 1 && (int)f.value.size() == f.channels && left.cols() == f.width &&
                      left.rows() == f.height && right.cols() == f.width && right.rows() == f.height && p.iterations >= 1 &&
                      p.iterations <= 16;
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_propagate_fields");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int W = f.width, H = f.height, C = f.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> in((size_t)C * n), out((size_t)C * n);
  std::vector<uint8_t> l(n), r(n), choice(n);
  std::vector<uint16_t> cost(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      l[at] = left(y, x), r[at] = right(y, x);
      for (int c = 0; c < C; ++c) in[(size_t)c * n + at] = f.value[(size_t)c](y, x);
    }
  const gpc_propagate prm = p.toC();
  Result res;
  res.stats.assign(4 * (size_t)p.iterations, 0);
  const int st = gpc_hip_propagate_fields(h.ctx, in.data(), l.data(), r.data(), C, W, H, 1, &prm, out.data(), cost.data(),
                                          choice.data(), res.stats.data());
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_propagate_fields");
    return Result();
  }
  res.field.width = W, res.field.height = H, res.field.channels = C;
  res.field.level = f.level;
  res.cost = ndb::Buffer<uint16_t>(H, W);
  res.choice = ndb::Buffer<uint8_t>(H, W);
  for (int c = 0; c < C; ++c) res.field.value.emplace_back(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      res.cost(y, x) = cost[at];
      res.choice(y, x) = choice[at];
      for (int c = 0; c < C; ++c) res.field.value[(size_t)c](y, x) = out[(size_t)c * n + at];
    }
  return res;
}

}  // namespace propagate
}  // namespace gpc
#endif
