// track_check -- gpc::tracking::assemble of include/gpc/tracking.hpp on hand-made records and links, for pytest.  Host only:
// no device is touched.  Returns 0 and prints "ok" when every case gives the tracks written out below.
#include <cstdio>
#include <vector>

#include "gpc/tracking.hpp"

typedef std::vector<std::vector<ndb::Correspondence>> Records;
typedef std::vector<std::vector<int32_t>> Links;

static ndb::Correspondence rec(int sx, int sy, int tx, int ty) { return ndb::Correspondence(ndb::Point(sx, sy), ndb::Point(tx, ty)); }

static bool is(const gpc::tracking::Track& t, int first, std::vector<std::pair<int, int>> pts) {
  if (t.firstFrame != first || t.points.size() != pts.size()) return false;
  for (size_t k = 0; k < pts.size(); ++k)
    if (t.points[k].x != pts[k].first || t.points[k].y != pts[k].second) return false;
  return true;
}

int main() {
  Records r = {{rec(1, 1, 2, 2), rec(5, 5, 6, 6)}, {rec(6, 6, 7, 7), rec(2, 2, 3, 3), rec(9, 9, 9, 8)}, {rec(3, 3, 4, 4)}};
  Links next = {{1, 0}, {-1, 0, -1}, {-1}};
  std::vector<gpc::tracking::Track> t = gpc::tracking::assemble(r, next);
  if (t.size() != 3) return 1;
  if (!is(t[0], 0, {{1, 1}, {2, 2}, {3, 3}, {4, 4}})) return 2;   // through all pairs
  if (!is(t[1], 0, {{5, 5}, {6, 6}, {7, 7}})) return 3;           // ends early
  if (!is(t[2], 1, {{9, 9}, {9, 8}})) return 4;                   // starts late, one record
  t = gpc::tracking::assemble(r, next, 2);
  if (t.size() != 2 || !is(t[0], 0, {{1, 1}, {2, 2}, {3, 3}, {4, 4}}) || !is(t[1], 0, {{5, 5}, {6, 6}, {7, 7}})) return 5;
  t = gpc::tracking::assemble(r, next, 3);
  if (t.size() != 1 || t[0].points.size() != 4) return 6;
  if (!gpc::tracking::assemble(r, next, 4).empty()) return 7;
  // an empty middle pair: nothing crosses it
  Records e = {{rec(1, 1, 2, 2)}, {}, {rec(2, 2, 3, 3)}};
  Links en = {{-1}, {}, {-1}};
  t = gpc::tracking::assemble(e, en);
  if (t.size() != 2 || !is(t[0], 0, {{1, 1}, {2, 2}}) || !is(t[1], 2, {{2, 2}, {3, 3}})) return 8;
  // one pair
  Records one = {{rec(4, 4, 5, 5), rec(6, 6, 7, 7)}};
  t = gpc::tracking::assemble(one, Links{{-1, -1}});
  if (t.size() != 2 || !is(t[1], 0, {{6, 6}, {7, 7}})) return 9;
  // links that point outside the next pair, and missing link rows, end the chain instead of being followed
  Links bad = {{7, 0}, {-1, 0, -1}};
  t = gpc::tracking::assemble(r, bad);
  if (t.size() != 4 || !is(t[0], 0, {{1, 1}, {2, 2}}) || !is(t[1], 0, {{5, 5}, {6, 6}, {7, 7}}) || !is(t[2], 1, {{2, 2}, {3, 3}, {4, 4}}) ||
      !is(t[3], 1, {{9, 9}, {9, 8}}))
    return 10;
  if (!gpc::tracking::assemble(Records(), Links()).empty()) return 11;
  printf("ok\n");
  return 0;
}
