// Stand-alone check of the dense field scorer's host side.  Without arguments: opengpc_amd/csrc/field_score_host.h (no HIP)
// against the C ABI's structs -- the parameter and size checks, the squares the kernel compares against, the launch
// geometry, the integer square root; built plainly and with -fsanitize=address,undefined.  Built with
// -DFIELD_SCORE_WITH_LIBRARY against libgpc_hip.so and given a file, it scores the case the file holds through
// gpc::evaluation::scoreField (include/gpc/dense_evaluation.hpp) and compares with the words and the error plane the Python
// model wrote there (tests/test_field_score_cpp.py has the layout).  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "field_score_host.h"
#ifdef FIELD_SCORE_WITH_LIBRARY
#include "gpc/dense_evaluation.hpp"
#endif

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static gpc_field_score_prm make(int n_thr, int t0, int t1, int abs_q8, int rel, int n_speed, int s0, int s1, int s2, int reserved) {
  gpc_field_score_prm p;
  memset(&p, 0, sizeof p);
  p.n_thr = n_thr, p.thr_q8[0] = t0, p.thr_q8[1] = t1, p.out_abs_q8 = abs_q8, p.out_rel_pm = rel;
  p.n_speed = n_speed, p.speed_q8[0] = s0, p.speed_q8[1] = s1, p.speed_q8[2] = s2, p.reserved = reserved;
  return p;
}

static int host_checks() {
  using namespace gpc;
  EXPECT(sizeof(gpc_field_score_prm) == 64 && sizeof(gpc_field_tally) == 96 && sizeof(gpc_field_score) == 512);
  const gpc_field_score_prm def = make(2, 256, 768, 768, 50, 0, 0, 0, 0, 0);
  EXPECT(fs_params(&def) == GPC_OK && fs_params(nullptr) == GPC_E_INVALID);
  const gpc_field_score_prm bad[] = {make(9, 0, 0, 0, 0, 0, 0, 0, 0, 0),        make(-1, 0, 0, 0, 0, 0, 0, 0, 0, 0),
                                     make(2, 256, 65536, 0, 0, 0, 0, 0, 0, 0),  make(1, -1, 0, 0, 0, 0, 0, 0, 0, 0),
                                     make(0, 0, 0, 65536, 0, 0, 0, 0, 0, 0),    make(0, 0, 0, -1, 0, 0, 0, 0, 0, 0),
                                     make(0, 0, 0, 0, 256, 0, 0, 0, 0, 0),      make(0, 0, 0, 0, -1, 0, 0, 0, 0, 0),
                                     make(0, 0, 0, 0, 0, 4, 0, 0, 0, 0),        make(0, 0, 0, 0, 0, -1, 0, 0, 0, 0),
                                     make(0, 0, 0, 0, 0, 1, (1 << 23) + 1, 0, 0, 0), make(0, 0, 0, 0, 0, 1, -1, 0, 0, 0),
                                     make(0, 0, 0, 0, 0, 2, 10, 9, 0, 0),       make(0, 0, 0, 0, 0, 3, 1, 2, 1, 0),
                                     make(0, 0, 0, 0, 0, 0, 0, 0, 0, 1),        make(INT32_MAX, 0, 0, 0, 0, 0, 0, 0, 0, 0),
                                     make(0, 0, 0, INT32_MIN, 0, 0, 0, 0, 0, 0), make(0, 0, 0, 0, 0, INT32_MAX, 0, 0, 0, 0)};
  for (const gpc_field_score_prm& b : bad) EXPECT(fs_params(&b) == GPC_E_INVALID);
  const gpc_field_score_prm edge[] = {make(0, 0, 0, 0, 0, 0, 0, 0, 0, 0), make(2, 0, 65535, 65535, 255, 3, 0, 1 << 23, 1 << 23, 0),
                                      make(1, 5, -7, 0, 0, 1, 3, -1, INT32_MAX, 0)};  // (entries beyond those in use are not looked at)
  for (const gpc_field_score_prm& e : edge) EXPECT(fs_params(&e) == GPC_OK);
  const FsPrm q = fs_squares(edge[1]);
  EXPECT(q.thr2[0] == 0 && q.thr2[1] == 4294836225u && q.abs2 == 4294836225u && q.rel2 == 65025 && q.sp2[2] == (1ull << 46));
  EXPECT(q.n_thr == 2 && q.n_speed == 3 && q.thr2[1] < 0xFFFFFFFFu);

  EXPECT(fs_limits(1, 1, 1, 1) == GPC_OK && fs_limits(2, 32768, 32768, 65535) == GPC_OK);
  EXPECT(fs_limits(0, 4, 4, 1) == GPC_E_INVALID && fs_limits(3, 4, 4, 1) == GPC_E_INVALID && fs_limits(1, 0, 4, 1) == GPC_E_INVALID);
  EXPECT(fs_limits(1, 32769, 1, 1) == GPC_E_UNSUPPORTED && fs_limits(1, 4, 4, 65536) == GPC_E_UNSUPPORTED);
  const float plane[4] = {0, 0, 0, 0};
  const gpc_truth none = {nullptr, nullptr, nullptr}, stereo = {plane, nullptr, nullptr}, flow = {plane, plane, nullptr};
  EXPECT(fs_truth(nullptr, 1) == GPC_E_INVALID && fs_truth(&none, 1) == GPC_E_INVALID);
  EXPECT(fs_truth(&stereo, 1) == GPC_OK && fs_truth(&stereo, 2) == GPC_E_INVALID);
  EXPECT(fs_truth(&flow, 2) == GPC_OK && fs_truth(&flow, 1) == GPC_E_INVALID);

  // the launch: a pair's slots may start 3 pixels before it; every pixel lies in a chunk
  EXPECT(fs_chunks(1, 1) == 1 && fs_chunks(2045, 1) == 1 && fs_chunks(2046, 1) == 2 && fs_chunks(32768, 32768) == (1 << 19) + 1);
  EXPECT(fs_groups(1, 1, 1) == 1 && fs_groups(1, 1, 65535) == FS_MAX_GROUPS && fs_groups(512, 260, 2) == 132);
  for (int n = 1; n < 5000; n += 7)
    for (int ph = 0; ph < 4; ++ph) EXPECT((int64_t)fs_chunks(n, 1) * FS_SLOTS * FS_PX - ph >= n);

  for (uint64_t k : {0ull, 1ull, 2ull, 3ull, 255ull, 46340ull, 46341ull, 65534ull, 65535ull, 65536ull}) {
    EXPECT(fs_isqrt(k * k) == k && (k == 0 || fs_isqrt(k * k - 1) == k - 1));
    if (k < 65536) EXPECT(fs_isqrt(k * k + 1) == (k == 0 ? 1 : k) && fs_isqrt(k * k + 2 * k) == k);
  }
  return 0;
}

#ifdef FIELD_SCORE_WITH_LIBRARY
// the file: int32 W, H, C, with_cls, n_thr, thr[8], out_abs, out_rel, n_speed, speed[3]; field [C][H][W] int32; u, v (C == 2)
// [H][W] float; ignore, cls [H][W] uint8; the model's 64 int64 words; its error plane [H][W] uint16
static int library_check(const char* path) {
  FILE* f = fopen(path, "rb");
  EXPECT(f != nullptr);
  int32_t head[19];
  EXPECT(fread(head, 4, 19, f) == 19);
  const int W = head[0], H = head[1], C = head[2];
  const size_t n = (size_t)W * H;
  std::vector<int32_t> field(C * n);
  std::vector<float> u(n), v(C == 2 ? n : 0);
  std::vector<uint8_t> ign(n), cls(n);
  std::vector<uint16_t> err(n);
  int64_t words[64];
  EXPECT(fread(field.data(), 4, C * n, f) == C * n && fread(u.data(), 4, n, f) == n);
  if (C == 2) EXPECT(fread(v.data(), 4, n, f) == n);
  EXPECT(fread(ign.data(), 1, n, f) == n && fread(cls.data(), 1, n, f) == n);
  EXPECT(fread(words, 8, 64, f) == 64 && fread(err.data(), 2, n, f) == n);
  fclose(f);

  gpc::dense::Field fld;
  fld.width = W, fld.height = H, fld.channels = C;
  for (int c = 0; c < C; ++c) fld.value.emplace_back(H, W);
  ndb::Buffer<uint8_t> classes(H, W);
  gpc::evaluation::Truth truth;
  truth.width = W, truth.height = H, truth.u = u, truth.v = v, truth.ignore = ign;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      for (int c = 0; c < C; ++c) fld.value[(size_t)c](y, x) = field[c * n + (size_t)y * W + x];
      classes(y, x) = cls[(size_t)y * W + x];
    }
  gpc::evaluation::FieldParams p;
  p.thresholdsQ8.assign(head + 5, head + 5 + head[4]);
  p.outlierAbsQ8 = head[13], p.outlierRelPm = head[14];
  p.speedsQ8.assign(head + 16, head + 16 + head[15]);
  p.wantError = true;
  const gpc::evaluation::FieldScore s = gpc::evaluation::scoreField(fld, truth, p, head[3] ? &classes : nullptr);
  EXPECT(!s.empty() && gpc::inference::lastStatus() == GPC_OK);
  EXPECT(memcmp(&s.counts, words, sizeof words) == 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) EXPECT(s.error(y, x) == err[(size_t)y * W + x]);
  const gpc_field_tally& a = s.counts.all;
  EXPECT(a.n_judged > 0 && s.epe() == (double)a.sum_e_q8 / (256.0 * (double)a.n_judged));
  EXPECT(s.within(0) == (double)a.n_within[0] / (double)a.n_judged && s.outlierRate() == (double)a.n_outlier / (double)a.n_judged);
  EXPECT(s.density() == (double)a.n_judged / (double)(a.n_judged + s.counts.n_hole) && s.rms() >= s.epe());
  EXPECT(s.density(0) + s.density(1) + s.density(2) + s.density(3) > s.density() - 1e-12);
  // a truth of another size is refused before the library is asked
  truth.width = W + 1;
  EXPECT(gpc::evaluation::scoreField(fld, truth, p).empty() && gpc::inference::lastStatus() == GPC_E_INVALID);
  return 0;
}
#endif

int main(int argc, char** argv) {
  if (host_checks()) return 1;
#ifdef FIELD_SCORE_WITH_LIBRARY
  if (argc > 1 && library_check(argv[1])) return 1;
#else
  (void)argc, (void)argv;
#endif
  puts("ok");
  return 0;
}
