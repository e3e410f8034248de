// gapfill.hpp -- closing the holes of a cleaned field along scanlines from the background side (extension; the reference
// stops at sparse supports): a hole looks along its row and its column for the two valued ends of its run of holes.  Where
// the ends agree it interpolates between them; where they disagree the run is a depth edge, and the hole takes the
// background end -- a choice, not a mean.  Integers only, run on the device by gpc_hip_gapfill_fields (include/gpc_hip.h has
// the rule).
//
//   gpc::gapfill::Params                        maxGap, discon, select, border
//   gpc::gapfill::Result                        field (holes closed where an axis was usable), how, stats
//   gpc::gapfill::gapfill(field, p)             one Result from a cleaned field (select = Background)
//   gpc::gapfill::gapfill(field, guide, p)      the same with the image as a guide, which select = Guide needs
//
// It belongs between the cleaner and the completion, which then only closes what is left:
//   Field f = gpc::clean::clean(fwd, &bwd).field;
//   f = gpc::gapfill::gapfill(f).field;
//   f = gpc::inpaint::inpaint(f, L).field;
// Errors are reported as everywhere in inference.hpp: an empty Result and lastStatus() / lastError().
#ifndef GPC_AMD_GAPFILL_HPP
#define GPC_AMD_GAPFILL_HPP

#include <cstdint>
#include <vector>

#include "gpc/dense.hpp"

namespace gpc {
namespace gapfill {

enum Select { Background = 0, Guide = 1 };

struct Params {
  int maxGap = 64;     // the longest run of holes an axis may close; 1 .. 32767
  int discon = 128;    // ends further apart than this in a channel, in 1/256 pixel, are a depth edge; 0 .. 2^24
  int select = Background;  // at a depth edge: the end with the smaller value, or the end whose guide is nearer the hole's
  int border = 1;      // 1: a run with one end at the image border takes its other end's value
  gpc_gapfill toC() const { return gpc_gapfill{maxGap, discon, select, border}; }
};

enum How : uint8_t { Valued = 0, RowContinuous = 1, RowEdge = 2, RowBorder = 3, ColumnContinuous = 4, ColumnEdge = 5, ColumnBorder = 6, Left = 255 };
enum Stat { Continuous = 0, Edge = 1, Border = 2, HolesLeft = 3 };

struct Result {
  gpc::dense::Field field;    // valued pixels unchanged; GPC_DENSE_NONE where a hole is left
  ndb::Buffer<uint8_t> how;   // a How per pixel
  int32_t stats[4] = {0, 0, 0, 0};  // pixels per Stat
  bool empty() const { return field.empty(); }
};

inline Result gapfill(const gpc::dense::Field& f, const ndb::Buffer<uint8_t>* guide, const Params& p = Params()) {
  namespace inf = gpc::inference;
  const bool shaped = !f.empty() && f.width >= 1 && f.height >= 1 && (int)f.value.size() == f.channels &&
                      (!guide || (guide->cols() == f.width && guide->rows() == f.height));
  if (!shaped) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_gapfill_fields");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int W = f.width, H = f.height, C = f.channels;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<int32_t> in((size_t)C * n), out((size_t)C * n);
  std::vector<uint8_t> g(guide ? n : 0), how(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      if (guide) g[at] = (*guide)(y, x);
      for (int c = 0; c < C; ++c) in[(size_t)c * n + at] = f.value[(size_t)c](y, x);
    }
  const gpc_gapfill prm = p.toC();
  Result res;
  const int st = gpc_hip_gapfill_fields(h.ctx, in.data(), guide ? g.data() : nullptr, C, W, H, 1, &prm, out.data(), how.data(), res.stats);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_gapfill_fields");
    return Result();
  }
  res.field.width = W, res.field.height = H, res.field.channels = C;
  res.field.level = f.level;
  res.how = ndb::Buffer<uint8_t>(H, W);
  for (int c = 0; c < C; ++c) res.field.value.emplace_back(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t at = (size_t)y * W + x;
      res.how(y, x) = how[at];
      for (int c = 0; c < C; ++c) res.field.value[(size_t)c](y, x) = out[(size_t)c * n + at];
    }
  return res;
}

inline Result gapfill(const gpc::dense::Field& f, const Params& p = Params()) { return gapfill(f, nullptr, p); }
inline Result gapfill(const gpc::dense::Field& f, const ndb::Buffer<uint8_t>& guide, const Params& p = Params()) {
  return gapfill(f, &guide, p);
}

}  // namespace gapfill
}  // namespace gpc
#endif
