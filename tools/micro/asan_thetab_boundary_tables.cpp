// ASan/UBSan run of ms_thetab_boundary_tables_host (host code only, no context, no GPU): the ring row -> incident facet
// CSR of tilt_thetaB_boundary_in on a triangulated hexagonal patch, over the 1-row, the 257-row and the empty ring, a
// permuted row numbering, facets with a row out of range and refused inputs.  The output arrays are allocated at exactly
// the documented sizes, so a write past them is reported.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "membrane_hip.h"

// a strip of 2 (n - 1) x (m - 1) triangles on an n x m grid
static void grid(int n, int m, std::vector<int32_t>& tri) {
  for (int j = 0; j + 1 < m; ++j)
    for (int i = 0; i + 1 < n; ++i) {
      const int a = j * n + i, b = a + 1, c = a + n, d = c + 1;
      const int32_t t[6] = {a, b, c, b, d, c};
      tri.insert(tri.end(), t, t + 6);
    }
}

static int run(const char* what, int nv, const std::vector<int32_t>& iperm, const std::vector<int32_t>& tri,
               const std::vector<int32_t>& rows, int want_rc) {
  const int nf = (int)tri.size() / 3, n = (int)rows.size();
  static const int32_t none[1] = {0};
  int32_t* off = new int32_t[n + 1];
  int rc = ms_thetab_boundary_tables_host(nv, iperm.empty() ? none : iperm.data(), nf, nf ? tri.data() : none, n,
                                          n ? rows.data() : none, off, nullptr);
  int bad = rc != want_rc, entries = -1;
  if (rc == MS_OK) {
    entries = off[n];
    int32_t* fv = new int32_t[3 * entries > 0 ? 3 * entries : 1];
    int32_t* off2 = new int32_t[n + 1];
    rc = ms_thetab_boundary_tables_host(nv, iperm.data(), nf, nf ? tri.data() : none, n, n ? rows.data() : none, off2, fv);
    bad |= rc != MS_OK || off[0] != 0;
    for (int i = 0; i < n && !bad; ++i) {
      bad |= off2[i + 1] != off[i + 1] || off[i + 1] < off[i];
      for (int k = off[i]; k < off[i + 1] && !bad; ++k) {
        bool has = false;
        for (int j = 0; j < 3; ++j) {
          bad |= fv[3 * k + j] < 0 || fv[3 * k + j] >= nv;
          has |= fv[3 * k + j] == iperm[rows[i]];
        }
        bad |= !has;  // every entry is a facet of its row
      }
    }
    delete[] fv;
    delete[] off2;
  }
  printf("%-34s rows=%d rc=%d (want %d) entries=%d %s\n", what, n, rc, want_rc, entries, bad ? "BAD" : "ok");
  delete[] off;
  return bad;
}

int main() {
  int bad = 0;
  const int n = 24, m = 24, nv = n * m;
  std::vector<int32_t> tri, id(nv), rev(nv), ring257(257);
  grid(n, m, tri);
  std::iota(id.begin(), id.end(), 0);
  for (int i = 0; i < nv; ++i) rev[i] = nv - 1 - i;
  for (int i = 0; i < 257; ++i) ring257[i] = (i * 2 + 1) % nv;  // distinct: 2 i + 1 < 576
  bad |= run("one row", nv, id, tri, {n + 1}, MS_OK);
  bad |= run("one row, reversed numbering", nv, rev, tri, {n + 1}, MS_OK);
  bad |= run("257 rows", nv, id, tri, ring257, MS_OK);
  bad |= run("257 rows, reversed numbering", nv, rev, tri, ring257, MS_OK);
  bad |= run("empty ring", nv, id, tri, {}, MS_OK);
  bad |= run("empty ring, no facets", nv, id, {}, {}, MS_OK);
  bad |= run("a row without a facet", nv + 1, [&] { auto p = id; p.push_back(nv); return p; }(), tri, {nv}, MS_OK);
  {
    std::vector<int32_t> t2 = tri;
    t2[4] = nv + 7;  // the facet is skipped
    t2[10] = -3;
    bad |= run("facets with a row out of range", nv, id, t2, ring257, MS_OK);
  }
  bad |= run("ring row out of range", nv, id, tri, {0, nv}, MS_ERR_INVALID);
  bad |= run("ring row negative", nv, id, tri, {-1}, MS_ERR_INVALID);
  bad |= run("ring row listed twice", nv, id, tri, {5, 9, 5}, MS_ERR_INVALID);
  {
    std::vector<int32_t> p = id;
    p[2] = nv + 40;
    bad |= run("permutation out of range", nv, p, tri, {1, 2}, MS_ERR_INVALID);
  }
  {
    int32_t off[2];
    bad |= ms_thetab_boundary_tables_host(nv, nullptr, 0, nullptr, 0, nullptr, off, nullptr) != MS_ERR_INVALID;
    bad |= ms_thetab_boundary_tables_host(-1, id.data(), 0, id.data(), 0, id.data(), off, nullptr) != MS_ERR_INVALID;
  }
  printf(bad ? "FAILED\n" : "all clean\n");
  return bad;
}
