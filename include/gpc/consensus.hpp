// consensus.hpp -- filter matches by grid motion consensus (extension; the reference matches one pair and leaves every
// use of the result to its caller).  A match is kept when enough matches around its source move the same way: grid-based
// motion statistics in integers, run on the device by gpc_hip_consensus_* (include/gpc_hip.h has the rule).
//
//   gpc::consensus::Settings                       cell 16, shifts 4, alpha 6 / 1 unless changed
//   gpc::consensus::filter(records, w, h, s)       the kept correspondences / supports of one pair, in input order
//   gpc::consensus::filter(pairs, w, h, s)         the same for a list of pairs (one call for all of them)
//
// No forest is needed.  Errors are reported as everywhere in inference.hpp: an empty result and lastStatus() / lastError().
#ifndef GPC_AMD_CONSENSUS_HPP
#define GPC_AMD_CONSENSUS_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "gpc/inference.hpp"

namespace gpc {
namespace consensus {

struct Settings {
  int cell = 16;      // cell edge in pixels: even, 4 .. 256
  int shifts = 4;     // 1: one grid; 4: the grids shifted by half a cell too
  int alphaNum = 6;   // a record passes when S > alpha * sqrt(T / k), alpha = alphaNum / alphaDen
  int alphaDen = 1;
  gpc_consensus toC() const { return gpc_consensus{cell, shifts, alphaNum, alphaDen}; }
};

namespace detail {
inline gpc_correspondence toC(const ndb::Correspondence& c) { return gpc_correspondence{c.srcPt.x, c.srcPt.y, c.tarPt.x, c.tarPt.y}; }
inline gpc_support toC(const ndb::Support& s) { return gpc_support{s.x, s.y, s.d}; }
inline ndb::Correspondence fromC(const gpc_correspondence& c) {
  return ndb::Correspondence(ndb::Point(c.src_x, c.src_y), ndb::Point(c.tar_x, c.tar_y));
}
inline ndb::Support fromC(const gpc_support& s) { return ndb::Support(s.x, s.y, s.d); }
inline int call(gpc_hip_ctx* ctx, const gpc_correspondence* r, int cap, const int32_t* n, int w, int h, int P, const gpc_consensus* p,
                gpc_correspondence* out, int32_t* kept) {
  return gpc_hip_consensus_correspondences(ctx, r, cap, n, w, h, P, p, nullptr, out, cap, nullptr, kept);
}
inline int call(gpc_hip_ctx* ctx, const gpc_support* r, int cap, const int32_t* n, int w, int h, int P, const gpc_consensus* p,
                gpc_support* out, int32_t* kept) {
  return gpc_hip_consensus_supports(ctx, r, cap, n, w, h, P, p, nullptr, out, cap, nullptr, kept);
}

template <class Rec, class CRec>
std::vector<std::vector<Rec>> filterPairs(const std::vector<std::vector<Rec>>& pairs, int width, int height, const Settings& s) {
  namespace inf = gpc::inference;
  typedef std::vector<std::vector<Rec>> Result;
  if (pairs.empty()) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_consensus");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const int P = (int)pairs.size();
  size_t cap = 1;
  for (const auto& r : pairs) cap = std::max(cap, r.size());
  std::vector<CRec> rec((size_t)P * cap), out((size_t)P * cap);
  std::vector<int32_t> counts((size_t)P), kept((size_t)P, 0);
  for (int t = 0; t < P; ++t) {
    counts[(size_t)t] = (int32_t)pairs[t].size();
    for (size_t i = 0; i < pairs[t].size(); ++i) rec[(size_t)t * cap + i] = toC(pairs[t][i]);
  }
  const gpc_consensus prm = s.toC();
  const int st = call(h.ctx, rec.data(), (int)cap, counts.data(), width, height, P, &prm, out.data(), kept.data());
  if (st != GPC_OK) {  // (cap_out == cap_per_pair: a kept list always fits)
    inf::detail::fail(st, h.ctx, "gpc_hip_consensus");
    return Result();
  }
  Result res((size_t)P);
  for (int t = 0; t < P; ++t) {
    res[t].reserve((size_t)kept[t]);
    for (int i = 0; i < kept[t]; ++i) res[t].push_back(fromC(out[(size_t)t * cap + i]));
  }
  return res;
}
}  // namespace detail

inline std::vector<std::vector<ndb::Correspondence>> filter(const std::vector<std::vector<ndb::Correspondence>>& pairs, int width,
                                                            int height, const Settings& s = Settings()) {
  return detail::filterPairs<ndb::Correspondence, gpc_correspondence>(pairs, width, height, s);
}
inline std::vector<std::vector<ndb::Support>> filter(const std::vector<std::vector<ndb::Support>>& pairs, int width, int height,
                                                     const Settings& s = Settings()) {
  return detail::filterPairs<ndb::Support, gpc_support>(pairs, width, height, s);
}
inline std::vector<ndb::Correspondence> filter(const std::vector<ndb::Correspondence>& records, int width, int height,
                                               const Settings& s = Settings()) {
  auto r = filter(std::vector<std::vector<ndb::Correspondence>>(1, records), width, height, s);
  return r.empty() ? std::vector<ndb::Correspondence>() : r[0];
}
inline std::vector<ndb::Support> filter(const std::vector<ndb::Support>& records, int width, int height, const Settings& s = Settings()) {
  auto r = filter(std::vector<std::vector<ndb::Support>>(1, records), width, height, s);
  return r.empty() ? std::vector<ndb::Support>() : r[0];
}

}  // namespace consensus
}  // namespace gpc
#endif
