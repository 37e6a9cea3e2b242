// ASan/UBSan run of ms_perimeter_tables_host (host code only, no context, no GPU): perimeter's entries, distinct vertices
// per loop and signed vertex -> entry CSR over empty, duplicate-edge, self-edge, shared-vertex, permuted and out-of-range
// inputs.  The output arrays are allocated at exactly the documented sizes, so a write past them is reported.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "membrane_hip.h"

static int run(const char* what, int nv, const std::vector<int32_t>& iperm, const std::vector<int32_t>& loop_off,
               const std::vector<int32_t>& tail, const std::vector<int32_t>& head, int want_rc) {
  const int n = (int)tail.size(), nl = (int)loop_off.size() - 1;
  int32_t counts[2] = {-1, -1};
  // heap blocks of exactly the documented room (new[] so the redzones sit right behind them)
  int32_t* et = new int32_t[n + 1];
  int32_t* eh = new int32_t[n + 1];
  int32_t* vo = new int32_t[nl + 1];
  int32_t* vrow = new int32_t[2 * n + 1];
  int32_t* co = new int32_t[2 * n + 2];
  int32_t* ce = new int32_t[2 * n + 1];
  static const int32_t none_i[1] = {0};
  const int rc = ms_perimeter_tables_host(nv, iperm.empty() ? none_i : iperm.data(), nl, loop_off.data(), n ? tail.data() : none_i,
                                          n ? head.data() : none_i, counts, et, eh, vo, vrow, co, ce);
  int bad = rc != want_rc;
  if (rc == MS_OK) {
    const int ne = counts[0], nd = counts[1];
    bad |= ne != n || nd > 2 * n || vo[0] != 0 || vo[nl] != nd || co[0] != 0 || co[nd] != 2 * ne;
    std::vector<int> seen(n > 0 ? 2 * n + 2 : 2, 0);  // every +-(entry + 1) appears exactly once
    for (int l = 0; l < nl && !bad; ++l) {
      bad |= vo[l + 1] < vo[l];
      for (int j = vo[l]; j < vo[l + 1] && !bad; ++j) {
        bad |= vrow[j] < 0 || vrow[j] >= nv || co[j + 1] <= co[j];
        for (int k = co[j]; k < co[j + 1] && !bad; ++k) {
          const int s = ce[k], e = (s < 0 ? -s : s) - 1;
          bad |= s == 0 || e < loop_off[l] || e >= loop_off[l + 1] || (k > co[j] && e < (ce[k - 1] < 0 ? -ce[k - 1] : ce[k - 1]) - 1);
          if (!bad) {
            bad |= (s < 0 ? et[e] : eh[e]) != vrow[j];
            bad |= seen[2 * e + (s > 0)]++ != 0;
          }
        }
      }
    }
  }
  printf("%-30s loops=%d n=%d rc=%d (want %d) entries=%d vertices=%d %s\n", what, nl, n, rc, want_rc, counts[0], counts[1],
         bad ? "BAD" : "ok");
  delete[] et;
  delete[] eh;
  delete[] vo;
  delete[] vrow;
  delete[] co;
  delete[] ce;
  return bad;
}

int main() {
  int bad = 0;
  const int nv = 9;
  std::vector<int32_t> id(nv), rev(nv);
  for (int i = 0; i < nv; ++i) {
    id[i] = i;
    rev[i] = nv - 1 - i;
  }
  bad |= run("no loop", nv, id, {0}, {}, {}, MS_OK);
  bad |= run("no loop, nv = 0", 0, {}, {0}, {}, {}, MS_OK);
  bad |= run("one empty loop", nv, id, {0, 0}, {}, {}, MS_OK);
  bad |= run("ring", nv, id, {0, 4}, {0, 1, 2, 3}, {1, 2, 3, 0}, MS_OK);
  bad |= run("ring, reversed rows", nv, rev, {0, 4}, {0, 1, 2, 3}, {1, 2, 3, 0}, MS_OK);
  bad |= run("two loops sharing vertices", nv, id, {0, 4, 7}, {0, 1, 2, 3, 0, 4, 5}, {1, 2, 3, 0, 4, 5, 1}, MS_OK);
  bad |= run("empty loop between two", nv, id, {0, 2, 2, 3}, {0, 1, 4}, {1, 2, 5}, MS_OK);
  bad |= run("duplicate and reversed edges", nv, id, {0, 4}, {4, 4, 5, 4}, {5, 5, 4, 5}, MS_OK);
  bad |= run("self edge", nv, id, {0, 1}, {7}, {7}, MS_OK);
  bad |= run("tail out of range", nv, id, {0, 2}, {0, 9}, {1, 2}, MS_ERR_INVALID);
  bad |= run("head negative", nv, id, {0, 2}, {0, 1}, {1, -1}, MS_ERR_INVALID);
  bad |= run("loop_off[0] != 0", nv, id, {1, 2}, {0, 1}, {1, 2}, MS_ERR_INVALID);
  bad |= run("loop offsets decrease", nv, id, {0, 2, 1}, {0, 1}, {1, 2}, MS_ERR_INVALID);
  std::vector<int32_t> badperm = id;
  badperm[2] = 40;
  bad |= run("permutation out of range", nv, badperm, {0, 2}, {1, 2}, {2, 3}, MS_ERR_INVALID);
  {
    int32_t counts[2];
    bad |= ms_perimeter_tables_host(nv, nullptr, 0, nullptr, nullptr, nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr) != MS_ERR_INVALID;
    bad |= ms_perimeter_tables_host(-1, id.data(), 0, id.data(), id.data(), id.data(), counts, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr) != MS_ERR_INVALID;
  }
  printf(bad ? "FAILED\n" : "all clean\n");
  return bad;
}
