// tracking.hpp -- point tracks over a frame sequence (extension; the reference matches one pair at a time and has no
// counterpart).  The correspondences of consecutive frame pairs, chained on the device by gpc_hip_track_sequence /
// gpc_hip_track_records (include/gpc_hip.h has the linking rule), assembled here into one list of points per track.
//
//   gpc::tracking::Track                      firstFrame and the point's position in frames firstFrame, firstFrame + 1, ...
//   Forest::trackSequence(frames, fm, s, n)   sequenceMatch + linking in one call; tracks of at least n records
//   gpc::tracking::trackRecords(records, ..)  the same for correspondences the caller holds (no forest needed)
//   gpc::tracking::assemble(records, next, n) the host part alone: Track vectors from records and their links
//   gpc::tracking::TrackStream                frames pushed as they arrive, track ids kept alive across pushes
//                                             (gpc_hip_track_stream_*): a video without a known end
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

// A video that arrives a frame or a few frames at a time: every push returns the new pairs' correspondences with, per
// record, the index of its predecessor in the pair before (-1: it starts a track) and its track id -- the ids the offline
// Forest::trackSequence over all frames so far would give.  The track table stays on the device; tracks() reads rows of it.
// One stream object per video.  It lives on the context inference.hpp keeps for the CALLING THREAD: create, push and
// destroy it on one thread, and before that thread ends (another thread's context does not know the stream and cannot
// release it).  Every push hands the stream's own forest over, as the match calls do; a Forest call with ANOTHER forest on
// the same thread between two pushes makes the carried codes meaningless, and every later push then fails with
// GPC_E_INVALID until reset().
class TrackStream {
 public:
  struct Pair {                                  // one new pair of consecutive frames
    int pair = 0;                                // its global index: frames pair and pair + 1
    std::vector<ndb::Correspondence> records;
    std::vector<int32_t> prev, trackId;          // per record
  };
  // capPerPair / trackCap <= 0: a quarter of the pixels per pair / four times the pixels in all
  TrackStream(int width, int height, const inference::Forest::FilterMask& fm, inference::InferenceSettings settings, int capPerPair = 0,
              int trackCap = 0)
      : w_(width), h_(height), fm_(fm) {
    namespace inf = gpc::inference;
    inf::detail::ContextHolder& h = inf::detail::holder();
    if (!h.ctx) return;
    const size_t n = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
    cap_ = capPerPair > 0 ? capPerPair : (int)std::max<size_t>(1024, n / 4);
    trackCap_ = trackCap > 0 ? trackCap : (int)std::max<size_t>(4096, 4 * n);
    const gpc_settings s = settings.toC();
    const int st = gpc_hip_track_stream_create(h.ctx, width, height, &s, cap_, trackCap_, &s_);
    if (st != GPC_OK) inf::detail::fail(st, h.ctx, "gpc_hip_track_stream_create");
  }
  ~TrackStream() {
    if (s_) (void)gpc_hip_track_stream_destroy(gpc::inference::detail::holder(true).ctx, s_);
  }
  TrackStream(const TrackStream&) = delete;
  TrackStream& operator=(const TrackStream&) = delete;

  bool valid() const { return s_ != nullptr; }
  int framesSeen() const { return frames_; }
  int tracksSoFar() const { return total_; }

  // One frame, or a span of frames in arrival order -> the pairs they complete (none for the very first frame).  A pair
  // with more than capPerPair records is cut to its first capPerPair (lastStatus() is GPC_E_CAPACITY then).
  std::vector<Pair> push(ndb::Buffer<uint8_t>& frame) { return push(&frame, 1); }
  std::vector<Pair> push(std::vector<ndb::Buffer<uint8_t>>& frames) { return push(frames.data(), frames.size()); }
  std::vector<Pair> push(ndb::Buffer<uint8_t>* frames, size_t count) {
    namespace inf = gpc::inference;
    typedef std::vector<Pair> Result;
    bool ok = s_ != nullptr && count >= 1 && count <= 65535;
    for (size_t f = 0; ok && f < count; ++f) ok = frames[f].cols() == w_ && frames[f].rows() == h_;
    if (!ok) {
      inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_track_stream_push");
      return Result();
    }
    inf::detail::ContextHolder& h = inf::detail::holder();
    if (!h.ctx || !inf::Forest::upload(h, fm_)) return Result();
    const size_t n = (size_t)w_ * h_, slots = count * (size_t)cap_;
    std::vector<uint8_t> fr(n * count);
    for (size_t f = 0; f < count; ++f) std::memcpy(&fr[n * f], frames[f].data(), n);
    std::vector<gpc_correspondence> corr(slots);
    std::vector<int32_t> counts(count), prev(slots, -1), id(slots, -1);
    int k = 0;
    int32_t total = 0;
    const int st = gpc_hip_track_stream_push(h.ctx, s_, fr.data(), (int)count, corr.data(), counts.data(), nullptr, prev.data(),
                                             id.data(), &k, &total);
    if (st != GPC_OK) inf::detail::fail(st, h.ctx, "gpc_hip_track_stream_push");
    if (st != GPC_OK && st != GPC_E_CAPACITY) return Result();
    Result out((size_t)k);
    const int pair0 = frames_ > 0 ? frames_ - 1 : 0;
    for (int t = 0; t < k; ++t) {
      const int m = std::min(std::max(counts[(size_t)t], 0), cap_);
      const size_t at = (size_t)t * cap_;
      out[(size_t)t].pair = pair0 + t;
      out[(size_t)t].records.reserve((size_t)m);
      for (int i = 0; i < m; ++i) {
        const gpc_correspondence& c = corr[at + i];
        out[(size_t)t].records.push_back(ndb::Correspondence(ndb::Point(c.src_x, c.src_y), ndb::Point(c.tar_x, c.tar_y)));
      }
      out[(size_t)t].prev.assign(prev.begin() + at, prev.begin() + at + m);
      out[(size_t)t].trackId.assign(id.begin() + at, id.begin() + at + m);
    }
    frames_ += (int)count;
    total_ = total;
    return out;
  }

  // rows [first, first + n) of the track table that exist (first_pair is a global pair index)
  std::vector<gpc_track> tracks(int first, int n) {
    namespace inf = gpc::inference;
    inf::detail::ContextHolder& h = inf::detail::holder();
    std::vector<gpc_track> rows((size_t)std::max(n, 0));
    int32_t total = 0;
    const int st = (s_ && h.ctx) ? gpc_hip_track_stream_read_tracks(h.ctx, s_, first, n, rows.data(), &total) : GPC_E_INVALID;
    if (st != GPC_OK) {
      inf::detail::fail(st, h.ctx, "gpc_hip_track_stream_read_tracks");
      return std::vector<gpc_track>();
    }
    total_ = total;
    rows.resize((size_t)std::max(0, std::min(first + n, (int)total) - first));
    return rows;
  }

  // a new video: frames forgotten, ids restart at 0
  bool reset() {
    namespace inf = gpc::inference;
    inf::detail::ContextHolder& h = inf::detail::holder();
    const int st = (s_ && h.ctx) ? gpc_hip_track_stream_reset(h.ctx, s_) : GPC_E_INVALID;
    if (st != GPC_OK) inf::detail::fail(st, h.ctx, "gpc_hip_track_stream_reset");
    if (st == GPC_OK) frames_ = total_ = 0;
    return st == GPC_OK;
  }

 private:
  int w_ = 0, h_ = 0, cap_ = 0, trackCap_ = 0, frames_ = 0;
  int32_t total_ = 0;
  inference::Forest::FilterMask fm_;
  gpc_hip_track_stream* s_ = nullptr;
};

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
