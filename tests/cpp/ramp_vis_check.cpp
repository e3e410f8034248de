// ramp_vis_check -- getDisparityVisualization of include/gpc/buffer.hpp for pytest.
//   ramp_vis_check <w> <h> <in.bin> <out.raw>
// in.bin: w*h gray bytes, then an int32 count n, then n records of (int32 x, int32 y, float d).
// out.raw: w*h RGB triples in row order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpc/buffer.hpp"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  FILE* f = fopen(argv[3], "rb");
  if (!f) return 3;
  ndb::Buffer<uint8_t> img(h, w);
  std::vector<uint8_t> px((size_t)w * h);
  if (fread(px.data(), 1, px.size(), f) != px.size()) return 4;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) img.setPixel(x, y, px[(size_t)y * w + x]);
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 4;
  std::vector<ndb::Support> supp;
  for (int i = 0; i < n; ++i) {
    int32_t xy[2];
    float d;
    if (fread(xy, 4, 2, f) != 2 || fread(&d, 4, 1, f) != 1) return 4;
    supp.push_back(ndb::Support(xy[0], xy[1], d));
  }
  fclose(f);
  ndb::Buffer<ndb::RGBColor> vis = ndb::getDisparityVisualization(img, supp);
  if (vis.cols() < w || vis.rows() != h) return 5;
  FILE* o = fopen(argv[4], "wb");
  if (!o) return 3;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const ndb::RGBColor c = vis.getPixel(x, y);
      const uint8_t rgb[3] = {c.r, c.g, c.b};
      fwrite(rgb, 1, 3, o);
    }
  fclose(o);
  return 0;
}
