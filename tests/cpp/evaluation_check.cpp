// evaluation_check <sintel root>/ : gpc::evaluation::Truth built from the datasources' files of alley_1 frame 1, printed as
// FNV-1a hashes of its planes (tests/test_score.py compares them with numpy), and Score's ratios.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <string>

#include "gpc/evaluation.hpp"

static uint64_t fnv(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using gpc::evaluation::Truth;
  gpc::datasource::SintelOpticalFlow flow(argv[1]);
  gpc::datasource::FlowField f;
  ndb::Buffer<uint8_t> oS, oT, iS, iT;
  if (flow.getFlow(1, f) | flow.getOcclusion(1, oS) | flow.getOcclusion(2, oT) | flow.getInvalid(1, iS) | flow.getInvalid(2, iT)) return 3;
  const Truth tf = Truth::fromFlow(f, oS, oT, iS, iT);
  printf("FLOW %d %d %llu %llu %llu\n", tf.width, tf.height, (unsigned long long)fnv(tf.u.data(), 4 * tf.u.size()),
         (unsigned long long)fnv(tf.v.data(), 4 * tf.v.size()), (unsigned long long)fnv(tf.ignore.data(), tf.ignore.size()));
  gpc::datasource::SintelStereo stereo(argv[1]);
  ndb::RGBBuffer d;
  ndb::Buffer<uint8_t> oc, oof;
  if (stereo.getDisparity(1, d) | stereo.getOcclusion(1, oc) | stereo.getInvalid(1, oof)) return 4;
  const Truth ts = Truth::fromDisparity(d, oc, oof);
  // (readPNG pads columns to a multiple of 16: the test's images are 64 wide, so the planes are the files')
  printf("STEREO %d %d %llu %llu\n", ts.width, ts.height, (unsigned long long)fnv(ts.u.data(), 4 * ts.u.size()),
         (unsigned long long)fnv(ts.ignore.data(), ts.ignore.size()));
  const Truth sub = Truth::fromDisparitySubpixel(d, oc, oof);
  printf("SUBPIX %llu\n", (unsigned long long)fnv(sub.u.data(), 4 * sub.u.size()));
  gpc::evaluation::Score s;
  s.n_judged = 4;
  s.n_within[0] = 3;
  s.n_matchable = 6;
  printf("SCORE %g %g\n", s.precision(0), s.recall(0));
  return ts.flow() || !tf.flow() || tf.resized(80, 50).ignore[79] != 1;
}
