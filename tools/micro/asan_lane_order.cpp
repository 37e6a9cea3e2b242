// ASan/UBSan run of the lean lane-order pass of the tile builder (host code only, CPU only): build_tiling's step 4 and
// lane_order_model on icospheres, a jittered disk, a tile with a valence-32 vertex and a mesh with bad indices; every
// tile's lean records must be a permutation of the common ones, for 1 and 4 threads alike.
//   hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//     -std=c++17 -Imembrane_solver_amd/csrc -Iinclude tools/micro/asan_lane_order.cpp membrane_solver_amd/csrc/ms_tiles.cpp
#include "ms_internal.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
using namespace ms;

// class-I icosphere of frequency f (vertices shared along edges through a map keyed by rounded coordinates)
static void icosphere(int f, std::vector<double>& P, std::vector<int32_t>& T) {
  const double t = (1.0 + std::sqrt(5.0)) / 2.0;
  const double V[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                           {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  const int F[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                        {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  std::map<std::array<long, 3>, int> ids;
  auto vid = [&](double x, double y, double z) {
    const double n = std::sqrt(x * x + y * y + z * z);
    x /= n; y /= n; z /= n;
    const std::array<long, 3> k = {std::lround(x * 1e9), std::lround(y * 1e9), std::lround(z * 1e9)};
    auto it = ids.find(k);
    if (it != ids.end()) return it->second;
    const int id = (int)(P.size() / 3);
    // a smooth displacement, so that the surface is not a perfect sphere
    const double s = 1.0 + 0.05 * std::sin(3 * x) * std::cos(2 * y + z);
    P.push_back(s * x); P.push_back(s * y); P.push_back(s * z);
    ids[k] = id;
    return id;
  };
  for (const auto& fc : F) {
    const double *a = V[fc[0]], *b = V[fc[1]], *c = V[fc[2]];
    auto at = [&](int i, int j) {
      const double u = (double)i / f, v = (double)j / f, w = 1.0 - u - v;
      return vid(w * a[0] + u * b[0] + v * c[0], w * a[1] + u * b[1] + v * c[1], w * a[2] + u * b[2] + v * c[2]);
    };
    for (int i = 0; i < f; ++i)
      for (int j = 0; j < f - i; ++j) {
        T.push_back(at(i, j)); T.push_back(at(i + 1, j)); T.push_back(at(i, j + 1));
        if (j < f - i - 1) { T.push_back(at(i + 1, j)); T.push_back(at(i + 1, j + 1)); T.push_back(at(i, j + 1)); }
      }
  }
}

// rings of a disk; ring 1 has `hub` vertices, so the centre has valence `hub`
static void disk(int rings, int hub, double jitter, std::vector<double>& P, std::vector<int32_t>& T) {
  P = {0.0, 0.0, 0.3};
  std::vector<int> start = {0}, count = {1};
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65535.0 - 0.5; };
  for (int r = 1; r <= rings; ++r) {
    const int n = hub * r;
    start.push_back((int)P.size() / 3);
    count.push_back(n);
    for (int j = 0; j < n; ++j) {
      const double rad = (double)r / rings + jitter * rnd() / rings, ph = 2 * M_PI * (j + jitter * rnd()) / n;
      P.push_back(rad * std::cos(ph)); P.push_back(rad * std::sin(ph)); P.push_back(0.3 * (1 - rad * rad));
    }
  }
  for (int j = 0; j < hub; ++j) { T.push_back(0); T.push_back(start[1] + j); T.push_back(start[1] + (j + 1) % hub); }
  for (int r = 1; r < rings; ++r) {
    const int n0 = count[r], n1 = count[r + 1];
    int i = 0, j = 0;  // walk both rings by angle
    while (i < n0 || j < n1) {
      const int a = start[r] + i % n0, b = start[r + 1] + j % n1;
      if (j < n1 && (i >= n0 || (double)(j + 1) / n1 <= (double)(i + 1) / n0 + 1e-12)) {
        T.push_back(a); T.push_back(b); T.push_back(start[r + 1] + (j + 1) % n1);
        ++j;
      } else {
        T.push_back(a); T.push_back(b); T.push_back(start[r] + (i + 1) % n0);
        ++i;
      }
    }
  }
}

static std::array<uint16_t, 4> canon(const TileFacet& f) { return {f.l0, f.l1, f.l2, f.flags}; }

static int check(const char* name, std::vector<double>& P, std::vector<int32_t>& T, int tile) {
  const int nv = (int)P.size() / 3, nf = (int)T.size() / 3;
  std::vector<TileFacet> first;
  for (const char* thr : {"1", "4"}) {
    setenv("MS_TILE_THREADS", thr, 1);
    Tiling t;
    std::string err;
    const int rc = build_tiling(nv, nf, P.data(), T.data(), nullptr, tile, 1, t, err);
    if (rc != 0) {
      printf("%s tile=%d threads=%s rc=%d %s\n", name, tile, thr, rc, err.c_str());
      return rc == MS_ERR_TILE_CAPACITY ? 0 : 1;
    }
    if (t.tile_facets_lean.size() != t.tile_facets.size()) return 1;
    int ordered = 0;
    for (int k = 0; k < t.n_tiles; ++k) {
      const size_t b = (size_t)t.tile_facet_off[k], e = (size_t)t.tile_facet_off[k + 1];
      std::vector<std::array<uint16_t, 4>> a, c;
      for (size_t p = b; p < e; ++p) {
        a.push_back(canon(t.tile_facets[p]));
        c.push_back(canon(t.tile_facets_lean[p]));
      }
      std::sort(a.begin(), a.end());
      std::sort(c.begin(), c.end());
      if (a != c) {
        printf("%s tile %d: the lean records are not a permutation of the common ones\n", name, k);
        return 1;
      }
      ordered += e - b >= 128;
    }
    const LaneModel mc = lane_order_model(t, t.tile_facets.data(), 0, t.n_tiles);
    const LaneModel ml = lane_order_model(t, t.tile_facets_lean.data(), 0, t.n_tiles);
    printf("%s nv=%d nf=%d tile=%d threads=%s tiles=%d (ordered %d) dropped=%ld  A16 %.3f -> %.3f  R16 %.3f -> %.3f  R32 %.3f -> %.3f\n",
           name, nv, nf, tile, thr, t.n_tiles, ordered, (long)t.dropped_facets, mc.a16_sum / std::max(1.0, mc.a16_groups),
           ml.a16_sum / std::max(1.0, ml.a16_groups), mc.r16_sum / std::max(1.0, mc.r16_groups), ml.r16_sum / std::max(1.0, ml.r16_groups),
           mc.r32_sum / std::max(1.0, mc.r32_groups), ml.r32_sum / std::max(1.0, ml.r32_groups));
    if (first.empty()) first = t.tile_facets_lean;
    else if (memcmp(first.data(), t.tile_facets_lean.data(), sizeof(TileFacet) * first.size()) != 0) {
      printf("%s: the result depends on the thread count\n", name);
      return 1;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  for (int f : {12, 13}) {
    std::vector<double> P; std::vector<int32_t> T;
    icosphere(f, P, T);
    for (int tile : {0, 64, 200, 256, 512}) bad |= check(f == 12 ? "ico12" : "ico13", P, T, tile);
  }
  {
    std::vector<double> P; std::vector<int32_t> T;
    disk(9, 6, 0.2, P, T);
    bad |= check("disk9", P, T, 256);
  }
  {
    std::vector<double> P; std::vector<int32_t> T;
    disk(6, 32, 0.0, P, T);  // the centre has valence 32
    bad |= check("valence32", P, T, 256);
    bad |= check("valence32", P, T, 64);
  }
  {
    std::vector<double> P; std::vector<int32_t> T;
    icosphere(12, P, T);
    T[4] = 100000; T[10] = -3; T[T.size() - 1] = (int32_t)(P.size() / 3);
    bad |= check("bad_indices", P, T, 256);
  }
  printf(bad ? "FAILED\n" : "all checks passed\n");
  return bad;
}
