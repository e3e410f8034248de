// evaluation_gpu_check <W> <H> <records.bin> <n> <supports|corr> <u.bin> <v.bin|-> <ignore.bin|-> thr...
// gpc::evaluation::scoreSupports / scoreCorrespondences on records and truth planes read from raw files; prints the fifteen
// counters of the Score (tests/test_gpu_score.py compares them with the Python records form).  Then the refusals: a Truth
// whose planes do not hold width x height values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gpc/evaluation.hpp"

template <class T>
static std::vector<T> slurp(const char* path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]);
  const size_t n = (size_t)atol(argv[4]), npx = (size_t)W * H;
  const bool corr = !strcmp(argv[5], "corr");
  gpc::evaluation::Truth t;
  t.width = W;
  t.height = H;
  t.u = slurp<float>(argv[6], npx);
  if (corr) t.v = slurp<float>(argv[7], npx);
  if (strcmp(argv[8], "-")) t.ignore = slurp<uint8_t>(argv[8], npx);
  std::vector<float> thr;
  for (int i = 9; i < argc; ++i) thr.push_back((float)atof(argv[i]));
  gpc::evaluation::Score s;
  if (corr) {
    std::vector<ndb::Correspondence> r = slurp<ndb::Correspondence>(argv[3], n);
    s = gpc::evaluation::scoreCorrespondences(r, t, thr);
  } else {
    std::vector<ndb::Support> r = slurp<ndb::Support>(argv[3], n);
    s = gpc::evaluation::scoreSupports(r, t, thr);
  }
  if (gpc::inference::lastStatus() != GPC_OK) return 3;
  const int64_t* w = reinterpret_cast<const int64_t*>(static_cast<const gpc_score*>(&s));
  printf("SCORE");
  for (int i = 0; i < 15; ++i) printf(" %lld", (long long)w[i]);
  printf("\n");
  // no records at all
  std::vector<ndb::Support> none;
  std::vector<ndb::Correspondence> nonec;
  const gpc::evaluation::Score z = corr ? gpc::evaluation::scoreCorrespondences(nonec, t, thr) : gpc::evaluation::scoreSupports(none, t, thr);
  printf("EMPTY %d %lld %lld\n", gpc::inference::lastStatus(), (long long)z.n_records, (long long)z.n_judged);
  // planes of the wrong size, and the wrong kind of truth, are refused before the library reads them
  gpc::evaluation::Truth bad = t;
  bad.u.resize(npx - 1);
  gpc::inference::clearStatus();
  (void)(corr ? gpc::evaluation::scoreCorrespondences(nonec, bad, thr) : gpc::evaluation::scoreSupports(none, bad, thr));
  const int st1 = gpc::inference::lastStatus();
  bad = t;
  bad.ignore.resize(5);
  gpc::inference::clearStatus();
  (void)(corr ? gpc::evaluation::scoreCorrespondences(nonec, bad, thr) : gpc::evaluation::scoreSupports(none, bad, thr));
  const int st2 = gpc::inference::lastStatus();
  gpc::inference::clearStatus();
  (void)(corr ? gpc::evaluation::scoreSupports(none, t, thr) : gpc::evaluation::scoreCorrespondences(nonec, t, thr));
  printf("REFUSED %d %d %d\n", st1, st2, gpc::inference::lastStatus());
  return 0;
}
