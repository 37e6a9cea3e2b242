// ASan/UBSan run of ms_rim_source_tables_host (host code only, no context, no GPU): the row -> rim edge CSR of
// tilt_rim_source_in/out over empty, duplicate-edge, gamma == 0, permuted and out-of-range inputs.  The output arrays
// are allocated at exactly the documented sizes, so a write past them is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "membrane_hip.h"

static int run(const char* what, int nv, const std::vector<int32_t>& iperm, const std::vector<int32_t>& tail,
               const std::vector<int32_t>& head, const std::vector<double>& gamma, int want_rc) {
  const int n = (int)tail.size();
  int32_t counts[2] = {-1, -1};
  // heap blocks of exactly the documented room (new[] so the redzones sit right behind them)
  int32_t* vrow = new int32_t[2 * n + 1];
  int32_t* off = new int32_t[2 * n + 2];
  int32_t* other = new int32_t[2 * n + 1];
  double* cg = new double[2 * n + 1];
  static const int32_t none_i[1] = {0};
  static const double none_d[1] = {0.0};
  const int rc = ms_rim_source_tables_host(nv, iperm.empty() ? none_i : iperm.data(), n, n ? tail.data() : none_i,
                                           n ? head.data() : none_i, n ? gamma.data() : none_d, counts, vrow, off, other, cg);
  int bad = rc != want_rc;
  if (rc == MS_OK) {
    const int ne = counts[0], nt = counts[1];
    bad |= ne != n || nt > 2 * n || off[0] != 0 || off[nt] != 2 * ne;
    for (int i = 0; i < nt && !bad; ++i) {
      bad |= vrow[i] < 0 || vrow[i] >= nv || (i > 0 && vrow[i] <= vrow[i - 1]) || off[i + 1] <= off[i];
      for (int k = off[i]; k < off[i + 1]; ++k) bad |= other[k] < 0 || other[k] >= nv || !std::isfinite(cg[k]);
    }
  }
  printf("%-28s n=%d rc=%d (want %d) edges=%d rim rows=%d %s\n", what, n, rc, want_rc, counts[0], counts[1], bad ? "BAD" : "ok");
  delete[] vrow;
  delete[] off;
  delete[] other;
  delete[] cg;
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
  bad |= run("empty", nv, id, {}, {}, {}, MS_OK);
  bad |= run("empty, nv = 0", 0, {}, {}, {}, {}, MS_OK);
  bad |= run("ring", nv, id, {0, 1, 2, 3}, {1, 2, 3, 0}, {1.0, 2.0, 0.0, -1.5}, MS_OK);
  bad |= run("ring, reversed rows", nv, rev, {0, 1, 2, 3}, {1, 2, 3, 0}, {1.0, 2.0, 0.0, -1.5}, MS_OK);
  bad |= run("duplicate edges", nv, id, {4, 4, 5, 4}, {5, 5, 4, 5}, {1.0, 1.0, 2.0, 0.0}, MS_OK);
  bad |= run("self edge", nv, id, {7}, {7}, {1.0}, MS_OK);
  bad |= run("every gamma 0", nv, id, {0, 1}, {1, 2}, {0.0, 0.0}, MS_OK);
  bad |= run("tail out of range", nv, id, {0, 9}, {1, 2}, {1.0, 1.0}, MS_ERR_INVALID);
  bad |= run("head negative", nv, id, {0, 1}, {1, -1}, {1.0, 1.0}, MS_ERR_INVALID);
  bad |= run("gamma NaN", nv, id, {0, 1}, {1, 2}, {1.0, NAN}, MS_ERR_INVALID);
  bad |= run("gamma inf", nv, id, {0}, {1}, {INFINITY}, MS_ERR_INVALID);
  std::vector<int32_t> badperm = id;
  badperm[2] = 40;
  bad |= run("permutation out of range", nv, badperm, {1, 2}, {2, 3}, {1.0, 1.0}, MS_ERR_INVALID);
  {
    int32_t counts[2];
    bad |= ms_rim_source_tables_host(nv, nullptr, 0, nullptr, nullptr, nullptr, counts, nullptr, nullptr, nullptr, nullptr) !=
           MS_ERR_INVALID;
    bad |= ms_rim_source_tables_host(-1, id.data(), 0, id.data(), id.data(), nullptr, counts, nullptr, nullptr, nullptr, nullptr) !=
           MS_ERR_INVALID;
  }
  printf(bad ? "FAILED\n" : "all clean\n");
  return bad;
}
