// Stand-alone check of the guided completion's CPU side (no HIP, no library): the parameter and size checks of
// opengpc_amd/csrc/inpaint_host.h, then gpc/inpaint.hpp's restatement of the rule over cases read from a file:
//   inpaint_check cases.bin results.bin
// cases.bin: int32 count, then per case int32 {C, W, H, radius, range_shift, min_weight, passes}, the field [C][H][W] int32 and
// the guide [H][W] uint8.  results.bin: per case out [C][H][W] int32, pass [H][W] uint8, stats [2] int32.  Built by
// tests/test_inpaint.py, plainly and with -fsanitize=address,undefined; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#define GPC_INPAINT_RULE_ONLY
#include "gpc/inpaint.hpp"
#include "inpaint_host.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int host_checks() {
  using namespace gpc;
  const gpc_inpaint def = {4, 3, 512, 32};
  EXPECT(sizeof(gpc_inpaint) == 16 && IP_TILE == 32);
  EXPECT(ip_params(&def) == GPC_OK && ip_params(nullptr) == GPC_E_INVALID);
  const gpc_inpaint bad[] = {{0, 3, 512, 32},         {9, 3, 512, 32},  {4, -1, 512, 32},        {4, 9, 512, 32},
                             {4, 3, 0, 32},           {4, 3, (1 << 24) + 1, 32}, {4, 3, 512, 0}, {4, 3, 512, 255},
                             {INT32_MIN, 3, 512, 32}, {4, INT32_MAX, 512, 32},   {4, 3, INT32_MAX, 32}, {4, 3, 512, INT32_MAX}};
  for (const gpc_inpaint& b : bad) EXPECT(ip_params(&b) == GPC_E_INVALID);
  const gpc_inpaint edge[] = {{1, 0, 1, 1}, {8, 8, 1 << 24, 254}};
  for (const gpc_inpaint& e : edge) EXPECT(ip_params(&e) == GPC_OK);
  EXPECT(ip_limits(1, 1, 1, 1) == GPC_OK && ip_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(ip_limits(0, 4, 4, 1) == GPC_E_INVALID && ip_limits(3, 4, 4, 1) == GPC_E_INVALID && ip_limits(1, 0, 4, 1) == GPC_E_INVALID);
  EXPECT(ip_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && ip_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);
  EXPECT(ip_limits(1, 0x7FFFFFFF, 0x7FFFFFFF, 1) == GPC_E_UNSUPPORTED);
  std::vector<int32_t> a(64);
  const uintptr_t p = (uintptr_t)a.data();
  EXPECT(ip_alias_ok(p, p, 64) && ip_alias_ok(p, p + 64, 64) && ip_alias_ok(p + 64, p, 64));
  EXPECT(!ip_alias_ok(p, p + 4, 64) && !ip_alias_ok(p + 63, p, 64));
  for (int shift = 0; shift <= 8; ++shift)
    for (int d = 0; d < 256; ++d) {
      EXPECT(ip_weight(d, shift) == inpaint::weight(d, 0, shift) && ip_weight(d, shift) == inpaint::weight(0, d, shift));
      EXPECT(ip_weight(d, shift) >= 1 && ip_weight(d, shift) <= 256);
    }
  EXPECT(ip_weight(255, 8) == 256 && ip_weight(0, 0) == 256 && ip_weight(1, 0) == 128 && ip_weight(8, 0) == 1 && ip_weight(255, 0) == 1);
  EXPECT(ip_weight(7, 3) == 256 && ip_weight(8, 3) == 128 && ip_weight(64, 3) == 1);
  // the mean: ties away from zero, the extremes of the sums (289 neighbours of weight 256 at either end of int32)
  EXPECT(ip_mean(-3 * 256, 2 * 256) == -2 && ip_mean(3 * 256, 2 * 256) == 2 && ip_mean(0, 256) == 0 && ip_mean(-1, 3) == 0);
  EXPECT(ip_mean(4, 3) == 1 && ip_mean(5, 3) == 2 && ip_mean(-5, 3) == -2 && inpaint::mean(-3, 2) == -2 && inpaint::mean(3, 2) == 2);
  const int64_t Wt = (int64_t)289 * 256;
  EXPECT(ip_mean(Wt * INT32_MAX, Wt) == INT32_MAX && ip_mean(Wt * (INT32_MIN + 1), Wt) == INT32_MIN + 1);
  EXPECT(inpaint::mean(Wt * INT32_MAX, Wt) == INT32_MAX && inpaint::mean(Wt * (int64_t)INT32_MIN, Wt) == INT32_MIN);
  EXPECT(ip_tiles(1) == 1 && ip_tiles(32) == 1 && ip_tiles(33) == 2 && ip_tiles(32768) == 1024);
  EXPECT(ip_ctl_stats_at() == 256 && ip_ctl_tiles_at(3) == 262 && ip_ctl_bytes(70, 45, 3) == 4 * (262 + 3 * 2 * 3));
  EXPECT(ip_ctl_bytes(32768, 32768, 65535) == 4 * (256 + (int64_t)2 * 65535 + (int64_t)1024 * 1024 * 65535));
  EXPECT(ip_pass_bytes(1024, 436, 16) == (int64_t)1024 * 436 * 16);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks()) return 1;
  if (argc == 3) {
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    EXPECT(in && res);
    int32_t count = 0;
    EXPECT(fread(&count, 4, 1, in) == 1 && count >= 0);
    for (int i = 0; i < count; ++i) {
      int32_t h[7];
      EXPECT(fread(h, 4, 7, in) == 7);
      const int C = h[0], W = h[1], H = h[2];
      EXPECT((C == 1 || C == 2) && W >= 1 && H >= 1 && W <= 4096 && H <= 4096);
      gpc::inpaint::Params p;
      p.radius = h[3], p.rangeShift = h[4], p.minWeight = h[5], p.passes = h[6];
      const gpc_inpaint c = p.toC();
      EXPECT(gpc::ip_params(&c) == GPC_OK);
      const size_t n = (size_t)W * H;
      std::vector<int32_t> field((size_t)C * n), out((size_t)C * n);
      std::vector<uint8_t> guide(n), pass(n);
      int32_t stats[2];
      EXPECT(fread(field.data(), 4, field.size(), in) == field.size() && fread(guide.data(), 1, n, in) == n);
      gpc::inpaint::reference(field.data(), guide.data(), C, W, H, p, out.data(), pass.data(), stats);
      EXPECT(fwrite(out.data(), 4, out.size(), res) == out.size() && fwrite(pass.data(), 1, n, res) == n && fwrite(stats, 4, 2, res) == 2);
    }
    fclose(in);
    EXPECT(fclose(res) == 0);
  }
  puts("ok");
  return 0;
}
