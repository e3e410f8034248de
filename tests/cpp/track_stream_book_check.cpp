// track_stream_book_check -- the host-side bookkeeping of a track stream (opengpc_amd/csrc/track_stream_host.h), by a
// host-only compile of that very header: no device, no library.  Built and run by tests/test_track_stream.py with
// -fsanitize=address,undefined.  Checked: the argument refusals, pairs per push, the form a stream is bound to, the
// generation of the carried codes, the per-push limits, and the 31-bit bound on the track ids -- when a push is refused,
// that a refused push changes nothing, and that reading the true total back tightens the bound.
#include <cstdio>
#include <cstring>
#include <vector>

#include "track_stream_host.h"

using namespace gpc;

static int fails = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                      \
    }                                                               \
  } while (0)

static TrsBook book(int W, int H, int cap, int track_cap) {
  TrsBook b;
  b.W = W, b.H = H, b.cap = cap, b.track_cap = track_cap;
  return b;
}

static bool same(const TrsBook& a, const TrsBook& b) {
  return a.W == b.W && a.H == b.H && a.cap == b.cap && a.track_cap == b.track_cap && a.form == b.form &&
         a.frames_seen == b.frames_seen && a.pairs_seen == b.pairs_seen && a.id_bound == b.id_bound && a.gen == b.gen;
}

// plan, and commit on GPC_OK, as the library does
static int push(TrsBook& b, int form, int n, uint64_t gen, int* k = nullptr) {
  TrsPush p;
  const TrsBook before = b;
  const int st = trs_plan(b, form, n, gen, &p);
  if (st != GPC_OK) {
    EXPECT(same(before, b));
    return st;
  }
  trs_commit(b, form, n, gen, p);
  if (k) *k = p.k;
  return st;
}

int main() {
  // creation
  EXPECT(trs_create_check(48, 41, 400, 0) == GPC_OK);
  EXPECT(trs_create_check(0, 41, 400, 0) == GPC_E_INVALID && trs_create_check(48, -1, 400, 0) == GPC_E_INVALID);
  EXPECT(trs_create_check(48, 41, 0, 0) == GPC_E_INVALID && trs_create_check(48, 41, 400, -1) == GPC_E_INVALID);
  EXPECT(trs_create_check(1 << 16, 1 << 15, 400, 0) == GPC_E_UNSUPPORTED);
  EXPECT(trs_create_check(1 << 15, 1 << 15, 1 << 30, 0) == GPC_OK && trs_create_check(48, 41, (1 << 30) + 1, 0) == GPC_E_UNSUPPORTED);

  // pairs per push, frames: n - 1 for the first frames, n afterwards; one frame first is valid
  {
    TrsBook b = book(160, 101, 10050, 100);
    int k = -1;
    TrsPush p;
    EXPECT(trs_plan(b, TRS_FRAMES, 0, 1, &p) == GPC_E_INVALID && trs_plan(b, TRS_FRAMES, 1, 1, nullptr) == GPC_E_INVALID);
    EXPECT(trs_plan(b, 0, 1, 1, &p) == GPC_E_INVALID && trs_plan(b, 3, 1, 1, &p) == GPC_E_INVALID);
    EXPECT(push(b, TRS_FRAMES, 1, 1, &k) == GPC_OK && k == 0 && b.frames_seen == 1 && b.pairs_seen == 0 && b.id_bound == 0);
    EXPECT(push(b, TRS_FRAMES, 1, 1, &k) == GPC_OK && k == 1 && b.pairs_seen == 1 && b.id_bound == 10050);
    EXPECT(trs_plan(b, TRS_FRAMES, 3, 1, &p) == GPC_OK && p.k == 3 && p.carry == 1);
    EXPECT(push(b, TRS_FRAMES, 3, 1, &k) == GPC_OK && k == 3 && b.frames_seen == 5 && b.pairs_seen == 4);
    // records into a stream of frames; another generation; both leave the book alone (push() checks that)
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_E_INVALID);
    EXPECT(push(b, TRS_FRAMES, 1, 2) == GPC_E_INVALID);
    trs_reset(b);
    EXPECT(b.form == TRS_NONE && b.frames_seen == 0 && b.pairs_seen == 0 && b.id_bound == 0);
    EXPECT(push(b, TRS_FRAMES, 4, 2, &k) == GPC_OK && k == 3);
    trs_reset(b);
    EXPECT(trs_plan(b, TRS_FRAMES, 2, 7, &p) == GPC_OK && p.k == 1 && p.carry == 0);
    // records: n pairs from the start, no generation
    EXPECT(push(b, TRS_RECORDS, 2, 1, &k) == GPC_OK && k == 2);
    EXPECT(push(b, TRS_RECORDS, 1, 99, &k) == GPC_OK && k == 1 && b.pairs_seen == 3);
    EXPECT(push(b, TRS_FRAMES, 1, 99) == GPC_E_INVALID);
  }
  // the per-push limits of the offline form
  {
    TrsBook b = book(48, 41, 400, 0);
    EXPECT(push(b, TRS_RECORDS, 65536, 1) == GPC_E_UNSUPPORTED);
    EXPECT(push(b, TRS_RECORDS, 65535, 1) == GPC_OK);
    EXPECT(push(b, TRS_RECORDS, 65535, 1) == GPC_E_UNSUPPORTED);   // a pair is carried now: the window would have 65536
    EXPECT(push(b, TRS_RECORDS, 65534, 1) == GPC_OK);
    TrsBook c = book(1 << 15, 1 << 15, 1 << 30, 0);
    EXPECT(push(c, TRS_RECORDS, 2, 1) == GPC_E_UNSUPPORTED);   // 2 * 2^30 > 2^31 - 1
  }
  // the id bound: += k * min(cap, W * H); a push that could pass 2^31 - 1 is refused and changes nothing
  {
    TrsBook b = book(1 << 15, 1 << 15, 1 << 30, 0);   // min(cap, W * H) = 2^30
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_OK && b.id_bound == (1ll << 30));
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_E_UNSUPPORTED && b.id_bound == (1ll << 30) && b.pairs_seen == 1);
    trs_tighten(b, 12);                                 // the true total, read back
    EXPECT(b.id_bound == 12);
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_OK && b.id_bound == (1ll << 30) + 12);
    trs_tighten(b, 0x7FFFFFFF - (1 << 30));             // exactly room for one more pair
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_OK && b.id_bound == 0x7FFFFFFFll);
    trs_tighten(b, 0x7FFFFFFF - (1 << 30) + 1);
    EXPECT(push(b, TRS_RECORDS, 1, 1) == GPC_E_UNSUPPORTED);
    trs_tighten(b, -5);                                 // (never a negative total)
    EXPECT(b.id_bound == 0x7FFFFFFFll - (1 << 30) + 1);
    // cap below the pixels: cap counts
    TrsBook c = book(160, 101, 5000, 0);
    EXPECT(push(c, TRS_RECORDS, 7, 1) == GPC_OK && c.id_bound == 35000);
    // pixels below cap: the pixels count; many small pushes reach the bound without overflow of the 64-bit sum
    TrsBook d = book(48, 41, 30000, 0);
    long pushes = 0;
    while (push(d, TRS_RECORDS, 65534, 1) == GPC_OK) ++pushes;
    EXPECT(pushes == 0x7FFFFFFFll / (65534ll * 48 * 41) && d.id_bound <= 0x7FFFFFFFll);
  }
  // read_tracks
  {
    TrsBook b = book(48, 41, 400, 10);
    EXPECT(trs_read_check(b, 0, 10) == GPC_OK && trs_read_check(b, 10, 0) == GPC_OK && trs_read_check(b, 9, 2) == GPC_E_CAPACITY);
    EXPECT(trs_read_check(b, -1, 2) == GPC_E_INVALID && trs_read_check(b, 0, -2) == GPC_E_INVALID);
    EXPECT(trs_read_check(b, 0x7FFFFFFF, 0x7FFFFFFF) == GPC_E_CAPACITY);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
