// tracking.hpp -- point tracks over a frame sequence (extension; the reference matches one pair at a time and has no
// counterpart).  The correspondences of consecutive frame pairs, chained on the device by gpc_hip_track_sequence /
// gpc_hip_track_records (include/gpc_hip.h has the linking rule), assembled here into one list of points per track.
//
//   gpc::tracking::Track                      firstFrame and the point's position in frames firstFrame, firstFrame + 1, ...
//   Forest::trackSequence(frames, fm, s, n)   sequenceMatch + linking in one call; tracks of at least n records
//   gpc::tracking::trackRecords(records, ..)  the same for correspondences the caller holds (no forest needed)
//   gpc::tracking::assemble(records, next, n) the host part alone: Track vectors from records and their links
//
// Errors are reported as everywhere in inference.hpp: an empty result and lastStatus() / lastError().
#ifndef GPC_AMD_TRACKING_HPP
#define GPC_AMD_TRACKING_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "gpc/inference.hpp"

namespace gpc {
namespace tracking {

struct Track {
  int firstFrame = 0;              // the frame points[0] lies in; points[k] lies in frame firstFrame + k
  std::vector<ndb::Point> points;  // records on the chain + 1: every record's source, then the last record's target
};

// Tracks from records[t][i] and next[t][i] (the successor of record i in records[t + 1], -1: none), in track-id order:
// heads by (t ascending, i ascending).  Tracks of fewer than minLength records are left out.  A link that points outside
// records[t + 1] ends its chain (the library writes none).
inline std::vector<Track> assemble(const std::vector<std::vector<ndb::Correspondence>>& records,
                                   const std::vector<std::vector<int32_t>>& next, int minLength = 1) {
  const size_t P = records.size();
  auto link = [&](size_t t, size_t i) -> long {
    if (t + 1 >= P || t >= next.size() || i >= next[t].size()) return -1;
    const long j = next[t][i];
    return (j >= 0 && (size_t)j < records[t + 1].size()) ? j : -1;
  };
  std::vector<std::vector<char>> has_pred(P);
  for (size_t t = 0; t < P; ++t) has_pred[t].assign(records[t].size(), 0);
  for (size_t t = 0; t + 1 < P; ++t)
    for (size_t i = 0; i < records[t].size(); ++i) {
      const long j = link(t, i);
      if (j >= 0) has_pred[t + 1][(size_t)j] = 1;
    }
  std::vector<Track> tracks;
  for (size_t t = 0; t < P; ++t)
    for (size_t i = 0; i < records[t].size(); ++i) {
      if (has_pred[t][i]) continue;
      Track tr;
      tr.firstFrame = (int)t;
      size_t tt = t, ii = i;
      for (;;) {
        tr.points.push_back(records[tt][ii].srcPt);
        const long j = link(tt, ii);
        if (j < 0) break;
        ++tt;
        ii = (size_t)j;
      }
      tr.points.push_back(records[tt][ii].tarPt);
      if ((int)tr.points.size() - 1 >= minLength) tracks.push_back(tr);
    }
  return tracks;
}

namespace detail {
// next[t][0 .. counts[t]) out of the [P][cap] array the library filled
inline std::vector<std::vector<int32_t>> links(const std::vector<int32_t>& next, const std::vector<int32_t>& counts, int cap) {
  std::vector<std::vector<int32_t>> r(counts.size());
  for (size_t t = 0; t < counts.size(); ++t)
    r[t].assign(next.begin() + (size_t)t * cap, next.begin() + (size_t)t * cap + (size_t)counts[t]);
  return r;
}
}  // namespace detail

// Correspondences the caller holds (records[t] = the matches of frames t, t + 1 of width x height) -> their tracks.
inline std::vector<Track> trackRecords(const std::vector<std::vector<ndb::Correspondence>>& records, int width, int height,
                                       int minLength = 1) {
  namespace inf = gpc::inference;
  if (records.empty()) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_track_records");
    return std::vector<Track>();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return std::vector<Track>();
  const int P = (int)records.size();
  size_t cap = 1, total = 0;
  for (const auto& r : records) cap = std::max(cap, r.size()), total += r.size();
  std::vector<gpc_correspondence> corr((size_t)P * cap);
  std::vector<int32_t> counts((size_t)P), next((size_t)P * cap, -1), id((size_t)P * cap, -1);
  for (int t = 0; t < P; ++t) {
    counts[(size_t)t] = (int32_t)records[t].size();
    for (size_t i = 0; i < records[t].size(); ++i) {
      const ndb::Correspondence& c = records[t][i];
      corr[(size_t)t * cap + i] = gpc_correspondence{c.srcPt.x, c.srcPt.y, c.tarPt.x, c.tarPt.y};
    }
  }
  std::vector<gpc_track> rows(total + 1);
  int32_t n = 0;
  const int st = gpc_hip_track_records(h.ctx, corr.data(), (int)cap, counts.data(), width, height, P, next.data(), id.data(),
                                       rows.data(), (int)rows.size(), &n);
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_track_records");
    return std::vector<Track>();
  }
  return assemble(records, detail::links(next, counts, (int)cap), minLength);
}

}  // namespace tracking

namespace inference {

inline std::vector<tracking::Track> Forest::trackSequence(std::vector<ndb::Buffer<uint8_t>>& frames, FilterMask& fm,
                                                          InferenceSettings settings, int minLength) {
  typedef std::vector<tracking::Track> Result;
  const int N = (int)frames.size();
  bool ok = N >= 2;
  const int W = N ? frames[0].cols() : 0, H = N ? frames[0].rows() : 0;
  for (int f = 0; ok && f < N; ++f) ok = frames[f].cols() == W && frames[f].rows() == H;
  if (!ok) {
    detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_track_sequence");
    return Result();
  }
  detail::ContextHolder& h = detail::holder();
  if (!h.ctx || !upload(h, fm)) return Result();
  const size_t n = (size_t)W * H;
  std::vector<uint8_t> fr(n * N);
  for (int f = 0; f < N; ++f) std::memcpy(&fr[n * f], frames[f].data(), n);
  const gpc_settings s = settings.toC();
  // a quarter of the pixels per pair first, the true largest count when that did not fit (as sequenceMatch)
  int cap = (int)std::max<size_t>(1024, n / 4);
  std::vector<gpc_correspondence> corr;
  std::vector<int32_t> counts((size_t)N - 1), next, id;
  std::vector<gpc_track> rows;
  int32_t nt = 0;
  int st = GPC_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const size_t slots = (size_t)cap * (N - 1);
    corr.resize(slots);
    next.assign(slots, -1);
    id.assign(slots, -1);
    rows.resize(slots);
    st = gpc_hip_track_sequence(h.ctx, fr.data(), W, H, N, &s, corr.data(), cap, counts.data(), nullptr, next.data(), id.data(),
                                rows.data(), (int)rows.size(), &nt);
    if (st != GPC_E_CAPACITY) break;
    cap = *std::max_element(counts.begin(), counts.end());
  }
  if (st != GPC_OK) {
    detail::fail(st, h.ctx, "gpc_hip_track_sequence");
    return Result();
  }
  std::vector<std::vector<ndb::Correspondence>> records((size_t)N - 1);
  for (int t = 0; t < N - 1; ++t) {
    const gpc_correspondence* c = corr.data() + (size_t)t * cap;
    records[t].reserve((size_t)counts[t]);
    for (int i = 0; i < counts[t]; ++i)
      records[t].push_back(ndb::Correspondence(ndb::Point(c[i].src_x, c[i].src_y), ndb::Point(c[i].tar_x, c[i].tar_y)));
  }
  return tracking::assemble(records, tracking::detail::links(next, counts, cap), minLength);
}

}  // namespace inference
}  // namespace gpc
#endif
