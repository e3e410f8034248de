// track_stream_host.h -- the host-side bookkeeping of a track stream (gpc_hip_track_stream_*) that needs no HIP: what a
// push may do given what the stream has seen, the 31-bit bound on the track ids, the limits of one push.  Plain C++ so
// that a stand-alone program can drive it under the sanitizers (tests/cpp/track_stream_book_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/gpc_hip.h"

namespace gpc {

enum { TRS_NONE = 0, TRS_FRAMES = 1, TRS_RECORDS = 2 };  // what a stream has been fed since create / reset

struct TrsBook {
  int W = 0, H = 0, cap = 0, track_cap = 0;
  int form = TRS_NONE;
  int frames_seen = 0, pairs_seen = 0;
  int64_t id_bound = 0;   // upper bound on the number of tracks so far
  uint64_t gen = 0;       // the context's forest / arithmetic generation the carried codes were hashed under
};

struct TrsPush {
  int k = 0;              // pairs the push produces
  int carry = 0;          // 1: a carried pair precedes them in the window
  int64_t bound_after = 0;
};

const int64_t kTrsMaxId = 0x7FFFFFFFll;

// the limits of gpc_hip_track_records_device on width, height and capacity; the table's size
inline int trs_create_check(int W, int H, int cap, int track_cap) {
  if (W <= 0 || H <= 0 || cap <= 0 || track_cap < 0) return GPC_E_INVALID;
  if ((int64_t)W * H > (1ll << 30) || cap > (1 << 30)) return GPC_E_UNSUPPORTED;
  return GPC_OK;
}

// A push of n frames (form TRS_FRAMES) or n pairs of records (TRS_RECORDS) under the context's generation ctx_gen: the
// status it must return before anything is touched, and on GPC_OK what it produces.  The book is not changed.
inline int trs_plan(const TrsBook& b, int form, int n, uint64_t ctx_gen, TrsPush* out) {
  if (!out || n < 1 || (form != TRS_FRAMES && form != TRS_RECORDS)) return GPC_E_INVALID;
  if (b.form != TRS_NONE && b.form != form) return GPC_E_INVALID;
  if (form == TRS_FRAMES && b.frames_seen > 0 && b.gen != ctx_gen) return GPC_E_INVALID;
  TrsPush p;
  p.k = (form == TRS_RECORDS || b.frames_seen > 0) ? n : n - 1;
  p.carry = b.pairs_seen > 0 ? 1 : 0;
  // (a launch has one grid row per pair of the window, the carried one included)
  if (p.k + p.carry > 65535 || (int64_t)p.k * b.cap > kTrsMaxId) return GPC_E_UNSUPPORTED;
  if ((int64_t)b.pairs_seen + p.k > kTrsMaxId || (int64_t)b.frames_seen + n > kTrsMaxId) return GPC_E_UNSUPPORTED;
  const int64_t px = (int64_t)b.W * b.H, per = b.cap < px ? b.cap : px;
  p.bound_after = b.id_bound + (int64_t)p.k * per;
  if (p.bound_after > kTrsMaxId) return GPC_E_UNSUPPORTED;
  *out = p;
  return GPC_OK;
}

inline void trs_commit(TrsBook& b, int form, int n, uint64_t ctx_gen, const TrsPush& p) {
  b.form = form;
  if (form == TRS_FRAMES) {
    b.frames_seen += n;
    b.gen = ctx_gen;
  }
  b.pairs_seen += p.k;
  b.id_bound = p.bound_after;
}

// a call has read the true total back
inline void trs_tighten(TrsBook& b, int32_t total) {
  if (total >= 0 && total < b.id_bound) b.id_bound = total;
}

inline void trs_reset(TrsBook& b) {
  b.form = TRS_NONE;
  b.frames_seen = b.pairs_seen = 0;
  b.id_bound = 0;
  b.gen = 0;
}

// rows [first, first + n) of a table of track_cap rows
inline int trs_read_check(const TrsBook& b, int first, int n) {
  if (first < 0 || n < 0) return GPC_E_INVALID;
  if ((int64_t)first + n > b.track_cap) return GPC_E_CAPACITY;
  return GPC_OK;
}

}  // namespace gpc
