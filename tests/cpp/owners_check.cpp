// owners_check.cpp -- opengpc_amd/csrc/owners.h driven by a fake backend that records every allocate and release.
// Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_owners.py: a double release is a double
// free of the fake's malloc'ed memory, a lost one a leak at exit.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "owners.h"

namespace {

int g_allocs = 0, g_releases = 0, g_creates = 0, g_destroys = 0;
size_t g_bytes = 0;
unsigned g_last_flags = 0;
bool g_fail = false;  // the next allocate / create fails

struct FakeMem {
  using status = int;
  static int alloc(void** p, size_t bytes, unsigned flags) {
    if (g_fail) return 7;
    *p = malloc(bytes);
    ++g_allocs, g_bytes += bytes, g_last_flags = flags;
    return 0;
  }
  static int release(void* p, size_t bytes) {
    free(p);
    ++g_releases, g_bytes -= bytes;
    return 0;
  }
};
struct FakeHandles {
  using handle = int*;
  using status = int;
  static int create(int** h, unsigned flags) {
    if (g_fail) return 7;
    *h = new int((int)flags);
    ++g_creates;
    return 0;
  }
  static int destroy(int* h) {
    delete h;
    ++g_destroys;
    return 0;
  }
};
using Buf = gpc::Block<FakeMem>;
using Words = gpc::Block<FakeMem, int>;
using Hnd = gpc::Handle<FakeHandles>;

#define REQUIRE(cond)                                             \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      return 1;                                                   \
    }                                                             \
  } while (0)

int check_blocks() {
  {  // freed exactly once on destruction, with the size it was allocated with
    Buf b;
    REQUIRE(b.alloc(100, 5) == 0 && b.p && b.cap == 100 && g_last_flags == 5);
    REQUIRE(g_allocs == 1 && g_releases == 0 && g_bytes == 100);
  }
  REQUIRE(g_allocs == 1 && g_releases == 1 && g_bytes == 0);
  {  // a move leaves the source empty and frees nothing
    Buf a;
    REQUIRE(a.alloc(64) == 0);
    void* was = a.p;
    Buf b(std::move(a));
    REQUIRE(!a.p && a.cap == 0 && b.p == was && b.cap == 64 && g_releases == 1);
    // move-assignment frees the old target once
    Buf d;
    REQUIRE(d.alloc(32) == 0);
    d = std::move(b);
    REQUIRE(g_releases == 2 && d.p == was && d.cap == 64 && !b.p && b.cap == 0);
    // self-move is harmless
    Buf& alias = d;
    d = std::move(alias);
    REQUIRE(g_releases == 2 && d.p == was && d.cap == 64);
    // std::swap frees nothing (full against full, full against empty)
    Buf e;
    REQUIRE(e.alloc(16) == 0);
    void* was_e = e.p;
    std::swap(d, e);
    REQUIRE(g_releases == 2 && d.p == was_e && d.cap == 16 && e.p == was && e.cap == 64);
    Buf none;
    std::swap(d, none);
    REQUIRE(g_releases == 2 && !d.p && d.cap == 0 && none.p == was_e && none.cap == 16);
    // alloc over a full owner releases the old block first
    REQUIRE(e.alloc(8) == 0 && g_releases == 3 && e.cap == 8);
    // reset releases once, and on an empty owner calls nothing
    REQUIRE(e.reset() == 0 && g_releases == 4 && !e.p && e.cap == 0);
    REQUIRE(e.reset() == 0 && g_releases == 4);
    REQUIRE(d.reset() == 0 && g_releases == 4);
  }
  REQUIRE(g_allocs == 5 && g_releases == 5 && g_bytes == 0);
  {  // a failed allocation leaves the owner empty, over an empty owner and over a full one
    Words w;
    g_fail = true;
    REQUIRE(w.alloc(40) == 7 && !w.p && w.cap == 0);
    g_fail = false;
    REQUIRE(w.alloc(40) == 0 && w.cap == 40);
    w.p[9] = 3;  // (typed: 40 bytes are ten ints)
    g_fail = true;
    REQUIRE(w.alloc(80) == 7 && !w.p && w.cap == 0);
    g_fail = false;
  }
  REQUIRE(g_allocs == 6 && g_releases == 6 && g_bytes == 0);
  return 0;
}

int check_handles() {
  {
    Hnd h;
    REQUIRE(!h && h.create(2) == 0 && h && *h.h == 2);
  }
  REQUIRE(g_creates == 1 && g_destroys == 1);
  {
    Hnd a;
    REQUIRE(a.create(0) == 0);
    int* was = a;
    Hnd b(std::move(a));
    REQUIRE(!a.h && b.h == was && g_destroys == 1);
    Hnd d;
    REQUIRE(d.create(0) == 0);
    d = std::move(b);
    REQUIRE(g_destroys == 2 && d.h == was && !b.h);
    Hnd& alias = d;
    d = std::move(alias);
    REQUIRE(g_destroys == 2 && d.h == was);
    Hnd e;
    REQUIRE(e.create(0) == 0);
    int* was_e = e;
    std::swap(d, e);
    REQUIRE(g_destroys == 2 && d.h == was_e && e.h == was);
    REQUIRE(e.reset() == 0 && g_destroys == 3 && !e.h);
    REQUIRE(e.reset() == 0 && g_destroys == 3);
    g_fail = true;
    REQUIRE(e.create(0) == 7 && !e.h);
    REQUIRE(d.create(0) == 7 && !d.h && g_destroys == 4);  // (the old handle goes first, as a block's does)
    g_fail = false;
  }
  REQUIRE(g_creates == 4 && g_destroys == 4);
  return 0;
}

}  // namespace

int main() {
  if (check_blocks() || check_handles()) return 1;
  if (g_allocs != g_releases || g_creates != g_destroys || g_bytes != 0) {
    printf("at exit: %d allocations, %d releases, %d creates, %d destroys\n", g_allocs, g_releases, g_creates, g_destroys);
    return 1;
  }
  printf("ok\n");
  return 0;
}
