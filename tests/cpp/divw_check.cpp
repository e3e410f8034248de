// divw_check -- the host-made multiply-high divisors (make_divw) and the fused join's shard split (join_shards_auto,
// make_join_split) of opengpc_amd/csrc/gpc_device.h, checked by a host-only compile of that very header: no device, no
// library.  Built and run by tests/test_divw.py (with -fsanitize=address,undefined, as the other host programs are).
//
//   divw    for every divisor d in 2 .. 65536, every 251st d up to 2^24 and every power of two (and its neighbours) up to
//           2^24: umulhi(k, magic) >> sh == k / d at k = m - 1, m, m + 1 for EVERY multiple m of d below 2^31, at
//           k = 2^31 - 1, and at four million random (d, k).  (The quotient of k by d only steps at a multiple, and the
//           multiply-high is monotone in k: right at m - 1 and m for every m is right everywhere.)
//   shards  for every batch size 1 .. 4096: 1 <= shards <= min(B, 13), never a multiple of 8 above 3 pairs, and the split the
//           launch makes of it (n_hi shards of ps[0] pairs, the others ps[1]) adds up to B -- for the chosen count and for
//           every forced count 1 .. 64 as the launch clamps it.
// Prints "OK <what>" lines; the first wrong value is printed and the exit status is 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "gpc_device.h"

// what divw() does on the device (__umulhi): the high half of the 64-bit product
static inline uint32_t divw_host(uint32_t k, const GpcDivW& d) {
  return (uint32_t)(((unsigned long long)k * d.magic) >> 32) >> d.sh;
}

struct Task {
  uint32_t d, q0, q1;  // multiples q * d for q in [q0, q1)
};

static std::atomic<int> g_bad(0);

static void fail(uint32_t d, uint32_t k, uint32_t got, uint32_t want) {
  if (g_bad.fetch_add(1) == 0) fprintf(stderr, "divw: %u / %u = %u, make_divw gives %u\n", k, d, want, got);
}

// every multiple m = q * d of the task and its two neighbours: m - 1 -> q - 1, m -> q, m + 1 -> q (d >= 2)
static void run_task(const Task& t) {
  const GpcDivW dv = make_divw((int)t.d);
  const unsigned long long lim = 1ull << 31;
  for (uint32_t q = t.q0; q < t.q1; ++q) {
    const unsigned long long m = (unsigned long long)q * t.d;
    if (m > 0) {
      const uint32_t k = (uint32_t)(m - 1);
      const uint32_t g = divw_host(k, dv);
      if (g != q - 1) fail(t.d, k, g, q - 1);
    }
    if (m < lim) {
      const uint32_t g = divw_host((uint32_t)m, dv);
      if (g != q) fail(t.d, (uint32_t)m, g, q);
    }
    if (m + 1 < lim) {
      const uint32_t g = divw_host((uint32_t)(m + 1), dv);
      if (g != q) fail(t.d, (uint32_t)(m + 1), g, q);
    }
  }
}

static int cmd_divw() {
  std::vector<uint32_t> ds;
  for (uint32_t d = 2; d <= 65536u; ++d) ds.push_back(d);
  for (uint32_t d = 65536u + 251u; d <= (1u << 24); d += 251u) ds.push_back(d);
  for (int p = 17; p <= 24; ++p) {
    ds.push_back((1u << p) - 1u);
    ds.push_back(1u << p);
    if (p < 24) ds.push_back((1u << p) + 1u);
  }
  std::vector<Task> tasks;
  const uint32_t chunk = 1u << 22;
  unsigned long long multiples = 0;
  for (uint32_t d : ds) {
    // q * d - 1 < 2^31  <=>  q <= 2^31 / d: the last multiple may be 2^31 itself, whose lower neighbour is 2^31 - 1
    const uint32_t nq = (uint32_t)((1ull << 31) / d) + 1u;
    multiples += nq;
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) tasks.push_back(Task{d, q0, q0 + chunk < nq ? q0 + chunk : nq});
  }
  unsigned nt = std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;
  std::atomic<size_t> next(0);
  std::vector<std::thread> pool;
  for (unsigned i = 0; i < nt; ++i)
    pool.emplace_back([&] {
      for (size_t j; (j = next.fetch_add(1)) < tasks.size() && !g_bad.load();) run_task(tasks[j]);
    });
  for (auto& th : pool) th.join();
  if (g_bad.load()) return 1;
  printf("OK divw %zu divisors, %llu multiples each with both neighbours\n", ds.size(), multiples);

  // the largest dividend the kernels may form, and random (d, k) against the machine's own division
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() -> uint32_t {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)(s >> 16);
  };
  for (uint32_t d : ds) {
    const uint32_t k = 0x7FFFFFFFu, g = divw_host(k, make_divw((int)d));
    if (g != k / d) return fail(d, k, g, k / d), 1;
  }
  for (uint32_t d = 2; d <= (1u << 24); d += 1u + rnd() % 7u) {  // ~4 million divisors, one random dividend each
    const uint32_t k = rnd() & 0x7FFFFFFFu, g = divw_host(k, make_divw((int)d));
    if (g != k / d) return fail(d, k, g, k / d), 1;
  }
  printf("OK divw 2^31 - 1 and random dividends\n");
  return 0;
}

static int check_split(int B, int nsh) {
  const GpcJoinSplit sp = make_join_split(B, nsh);
  const long total = (long)sp.n_hi * sp.ps[0] + (long)(nsh - sp.n_hi) * sp.ps[1];
  const bool ok = total == B && sp.n_hi >= 0 && sp.n_hi < nsh && sp.ps[1] >= 1 && sp.ps[0] - sp.ps[1] == (sp.n_hi ? 1 : 0);
  if (!ok) {
    fprintf(stderr, "split: %d pairs over %d shards: n_hi %d, ps %d / %d\n", B, nsh, sp.n_hi, sp.ps[0], sp.ps[1]);
    return 1;
  }
  for (int k = 0; k < 2; ++k) {  // the divisor that goes with a shard size is that size's (a shard of one pair: 2's, unused)
    const GpcDivW dv = make_divw(sp.ps[k] > 1 ? sp.ps[k] : 2);
    if (sp.ps_magic[k] != dv.magic || sp.ps_sh[k] != dv.sh) {
      fprintf(stderr, "split: %d pairs over %d shards: the divisor of ps[%d] = %d is another size's\n", B, nsh, k, sp.ps[k]);
      return 1;
    }
  }
  return 0;
}

static int cmd_shards() {
  for (int B = 1; B <= 4096; ++B) {
    const int n = join_shards_auto(B);
    const int most = B < 13 ? B : 13;
    if (n < 1 || n > most || (B > 3 && n % 8 == 0)) {
      fprintf(stderr, "shards: %d pairs over %d shards\n", B, n);
      return 1;
    }
    if (check_split(B, n)) return 1;
    for (int forced = 1; forced <= 64; ++forced)
      if (check_split(B, B < forced ? B : forced)) return 1;
  }
  printf("OK shards 4096 batch sizes\n");
  return 0;
}

int main(int argc, char** argv) {
  const char* cmd = argc > 1 ? argv[1] : "all";
  int rc = 0;
  if (!strcmp(cmd, "divw") || !strcmp(cmd, "all")) rc |= cmd_divw();
  if (!strcmp(cmd, "shards") || !strcmp(cmd, "all")) rc |= cmd_shards();
  return rc;
}
