// quads.hpp -- stereo sequences: circular matches closed into quads (extension; the reference matches one pair at a time
// and has no counterpart).  The supports of every stereo frame and the correspondences of both sides over time, joined on
// the device by gpc_hip_quads_sequence / gpc_hip_quads_records (include/gpc_hip.h has the rule): L_t -> R_t -> R_t+1 ->
// L_t+1 -> L_t.  What closes is a sparse scene-flow record: the point in the four images.
//
//   gpc::quads::Quad                                       the four points and the two support indices
//   Forest::stereoSequenceQuads(left, right, fm, ss, fs, tol)   match (each image hashed once) + closing in one call
//   gpc::quads::closeRecords(supports, flowL, flowR, w, h, tol) the closing for records the caller holds (no forest needed)
//
// Both return the quads of step t (frames t and t + 1) in result[t], by support0 ascending.  Errors are reported as
// everywhere in inference.hpp: an empty result and lastStatus() / lastError().
#ifndef GPC_AMD_QUADS_HPP
#define GPC_AMD_QUADS_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gpc/inference.hpp"

namespace gpc {
namespace quads {

struct Quad {
  ndb::Point l0, r0;  // the point in L_t and in R_t (the same row)
  ndb::Point l1, r1;  // ... in L_t+1 and in R_t+1
  int support0 = 0;   // the index of (l0, r0) among the supports of frame t
  int support1 = 0;   // the index of (l1, r1) among the supports of frame t + 1: chain steps by support1 == support0
};

namespace detail {
inline std::vector<std::vector<Quad>> unpack(const std::vector<gpc_quad>& q, const std::vector<int32_t>& nq, int cap) {
  std::vector<std::vector<Quad>> r(nq.size());
  for (size_t t = 0; t < nq.size(); ++t) {
    r[t].reserve((size_t)nq[t]);
    for (int k = 0; k < nq[t]; ++k) {
      const gpc_quad& g = q[t * (size_t)cap + (size_t)k];
      Quad o;
      o.l0 = ndb::Point(g.x, g.y);
      o.r0 = ndb::Point(g.x - g.d0, g.y);
      o.l1 = ndb::Point(g.x + g.u, g.y + g.v);
      o.r1 = ndb::Point(g.x + g.u - g.d1, g.y + g.v);
      o.support0 = g.support0;
      o.support1 = g.support1;
      r[t].push_back(o);
    }
  }
  return r;
}
}  // namespace detail

// Records the caller holds: supports[t] of the stereo frame t (N of them), flowL[t] / flowR[t] of the left / right frames
// t, t + 1 (N - 1 each), images of width x height -> the quads of every step.
inline std::vector<std::vector<Quad>> closeRecords(const std::vector<std::vector<ndb::Support>>& supports,
                                                   const std::vector<std::vector<ndb::Correspondence>>& flowL,
                                                   const std::vector<std::vector<ndb::Correspondence>>& flowR, int width,
                                                   int height, int tol) {
  namespace inf = gpc::inference;
  typedef std::vector<std::vector<Quad>> Result;
  const size_t N = supports.size();
  if (N < 2 || flowL.size() != N - 1 || flowR.size() != N - 1) {
    inf::detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_quads_records");
    return Result();
  }
  inf::detail::ContextHolder& h = inf::detail::holder();
  if (!h.ctx) return Result();
  const size_t P = N - 1;
  size_t cap_s = 1, cap_f = 1;
  for (const auto& s : supports) cap_s = std::max(cap_s, s.size());
  for (size_t t = 0; t < P; ++t) cap_f = std::max(cap_f, std::max(flowL[t].size(), flowR[t].size()));
  std::vector<gpc_support> sup(N * cap_s);
  std::vector<gpc_correspondence> fl(P * cap_f), fr(P * cap_f);
  std::vector<int32_t> nsup(N), nfl(P), nfr(P), nq(P);
  for (size_t t = 0; t < N; ++t) {
    nsup[t] = (int32_t)supports[t].size();
    for (size_t i = 0; i < supports[t].size(); ++i) sup[t * cap_s + i] = gpc_support{supports[t][i].x, supports[t][i].y, supports[t][i].d};
  }
  auto pack = [&](const std::vector<std::vector<ndb::Correspondence>>& src, std::vector<gpc_correspondence>& dst, std::vector<int32_t>& n) {
    for (size_t t = 0; t < P; ++t) {
      n[t] = (int32_t)src[t].size();
      for (size_t i = 0; i < src[t].size(); ++i) {
        const ndb::Correspondence& c = src[t][i];
        dst[t * cap_f + i] = gpc_correspondence{c.srcPt.x, c.srcPt.y, c.tarPt.x, c.tarPt.y};
      }
    }
  };
  pack(flowL, fl, nfl);
  pack(flowR, fr, nfr);
  std::vector<gpc_quad> q(P * cap_s);  // (a support starts at most one quad)
  const int st = gpc_hip_quads_records(h.ctx, sup.data(), (int)cap_s, nsup.data(), fl.data(), fr.data(), (int)cap_f, nfl.data(),
                                       nfr.data(), width, height, (int)N, tol, q.data(), (int)cap_s, nq.data());
  if (st != GPC_OK) {
    inf::detail::fail(st, h.ctx, "gpc_hip_quads_records");
    return Result();
  }
  return detail::unpack(q, nq, (int)cap_s);
}

}  // namespace quads

namespace inference {

inline std::vector<std::vector<quads::Quad>> Forest::stereoSequenceQuads(std::vector<ndb::Buffer<uint8_t>>& leftFrames,
                                                                         std::vector<ndb::Buffer<uint8_t>>& rightFrames,
                                                                         FilterMask& fm, InferenceSettings stereoSettings,
                                                                         InferenceSettings flowSettings, int tol) {
  typedef std::vector<std::vector<quads::Quad>> Result;
  const int N = (int)leftFrames.size();
  bool ok = N >= 2 && (int)rightFrames.size() == N;
  const int W = N ? leftFrames[0].cols() : 0, H = N ? leftFrames[0].rows() : 0;
  for (int f = 0; ok && f < N; ++f)
    ok = leftFrames[f].cols() == W && leftFrames[f].rows() == H && rightFrames[f].cols() == W && rightFrames[f].rows() == H;
  if (!ok) {
    detail::fail(GPC_E_INVALID, nullptr, "gpc_hip_quads_sequence");
    return Result();
  }
  detail::ContextHolder& h = detail::holder();
  if (!h.ctx || !upload(h, fm)) return Result();
  const size_t n = (size_t)W * H;
  std::vector<uint8_t> left(n * N), right(n * N);
  for (int f = 0; f < N; ++f) {
    std::memcpy(&left[n * f], leftFrames[f].data(), n);
    std::memcpy(&right[n * f], rightFrames[f].data(), n);
  }
  const gpc_settings ss = stereoSettings.toC(), fs = flowSettings.toC();
  // a quarter of the pixels per list first, the true largest counts when that did not fit (as sequenceMatch); a support
  // starts at most one quad, so cap_s quads per step always suffice
  int cap_s = (int)std::max<size_t>(1024, n / 4), cap_f = cap_s;
  std::vector<gpc_support> sup;
  std::vector<gpc_correspondence> fl, fr;
  std::vector<gpc_quad> q;
  std::vector<int32_t> nsup((size_t)N), nfl((size_t)N - 1), nfr((size_t)N - 1), nq((size_t)N - 1);
  int st = GPC_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    sup.resize((size_t)cap_s * N);
    fl.resize((size_t)cap_f * (N - 1));
    fr.resize((size_t)cap_f * (N - 1));
    q.resize((size_t)cap_s * (N - 1));
    st = gpc_hip_quads_sequence(h.ctx, left.data(), right.data(), W, H, N, &ss, &fs, tol, sup.data(), cap_s, nsup.data(), fl.data(),
                                fr.data(), cap_f, nfl.data(), nfr.data(), nullptr, q.data(), cap_s, nq.data());
    if (st != GPC_E_CAPACITY) break;
    cap_s = std::max(cap_s, *std::max_element(nsup.begin(), nsup.end()));
    cap_f = std::max(cap_f, std::max(*std::max_element(nfl.begin(), nfl.end()), *std::max_element(nfr.begin(), nfr.end())));
  }
  if (st != GPC_OK) {
    detail::fail(st, h.ctx, "gpc_hip_quads_sequence");
    return Result();
  }
  return quads::detail::unpack(q, nq, cap_s);
}

}  // namespace inference
}  // namespace gpc
#endif
