// The hard area constraints on the device (modules/constraints/body_area.py, global_area.py and the dense KKT
// projection of runtime/constraint_projection.py:101-129).
//
//   k_area_row<ATOMIC>  one workgroup per tile: gA = dA/dx of the owned rows (body_area.py:51-63: n = (v1 - v0) x (v2 - v0),
//                       facets with |n| < 1e-12 skipped, g0 = 1/2 (v1 - v2) x n_hat and cyclic) over the facets that
//                       carry TF_BODY, or over every facet (global_area); the tile's share of the area (the facets it
//                       owns) and of <gA,gA> go to the lane's own partials.
//   k_area_dots         one workgroup per tile, one pass over G: <g,gA>, and with the volume row <g,gV>, <gV,gV>, <gV,gA>.
//   k_area_fold         ONE workgroup: every partial row summed in tile order, then lambda of the 1 x 1 system
//                       (<gA,gA> > 1e-18) or of the 2 x 2 system C C^T + 1e-18 I (Cholesky, else LU with partial
//                       pivoting, else lambda = 0: the gradient is left alone).  rows == 0 folds the area and <gA,gA>
//                       alone (the enforcer).
//   k_area_apply        g -= lambda_V gV + lambda_A gA on every row (the fixed rows are zeroed behind it, by k_direction).
//
// The sums: MS_NSCAL has one slot left, so the lane keeps AP_ROWS partial rows of n_tiles cells and AP_RES result cells
// of its own (ms_ctx::d_area_part / d_area_res); nothing of it goes through the mailbox.  Vertex sums of the row kernel:
// LDS atomics by default, the per-vertex corner CSR in facet order under ms_set_deterministic; every other sum of the
// four kernels has a fixed order in both modes (a halving tree per workgroup, tile order in the fold).
#include "ms_internal.h"

namespace ms {
namespace {

constexpr int AB = 256;  // threads of the streaming kernels

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 sub(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 crs(const D3& a, const D3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ D3 lds3(const double* px, int cap, int s) { return {px[s], px[cap + s], px[2 * cap + s]}; }

// fixed-order sum over a workgroup of n threads (any n <= 512): thread t parks v, a halving tree over the next power of
// two; every thread gets the total
__device__ __forceinline__ double wg_tree_sum(double v, double* red, int n) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  int p = 1;
  while (p < n) p <<= 1;
  for (int s = p >> 1; s > 0; s >>= 1) {
    if (t < s && t + s < n) red[t] += red[t + s];
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}

// LDS: px[3][cap] | stg (ATOMIC: [3][T] sums of the owned slots; else [9][T] one facet chunk's corner rows) | red[T]
template <bool ATOMIC>
__global__ __launch_bounds__(512) void k_area_row(AreaRowArgs a) {
  extern __shared__ double lds[];
  const DeviceMesh& m = a.m;
  const int T = m.T, cap = a.cap, tid = threadIdx.x;
  double* px = lds;
  double* stg = px + 3 * cap;
  double* red = stg + (ATOMIC ? 3 : 9) * T;
  const int tile = a.tile0 + (int)blockIdx.x;
  const int v_lo = tile * m.own;
  const int n_owned = min(m.own, m.nv - v_lo);
  const int h0 = m.tile_halo_off[tile], nh = m.tile_halo_off[tile + 1] - h0;
  const int f0 = m.tile_facet_off[tile], f1 = m.tile_facet_off[tile + 1];
  // (the tiling bounds every slot by cap = T + the largest halo: n_owned + nh <= cap)
  for (int s = tid; s < n_owned + nh; s += T) {
    const int v = s < n_owned ? v_lo + s : m.halo_ids[h0 + (s - n_owned)];
    const size_t o = 3 * (size_t)v;
    px[s] = a.x[o];
    px[cap + s] = a.x[o + 1];
    px[2 * cap + s] = a.x[o + 2];
  }
  if (ATOMIC) {
    stg[tid] = 0.0;
    stg[T + tid] = 0.0;
    stg[2 * T + tid] = 0.0;
  }
  __syncthreads();

  double area = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  int cur = 0, end = 0;
  const uint16_t* vent = m.vent + m.tile_ent_off[tile];
  if (!ATOMIC && tid < n_owned) {
    const uint16_t* voff = m.tile_voff + (size_t)tile * (T + 1);
    cur = voff[tid];
    end = voff[tid + 1];
  }
  for (int c0 = f0; c0 < f1; c0 += T) {
    const int p = c0 + tid;
    D3 G0{0, 0, 0}, G1{0, 0, 0}, G2{0, 0, 0};
    TileFacet tf{0, 0, 0, 0};
    if (p < f1) {
      tf = m.tile_facets[p];
      if (a.all_facets || (tf.flags & TF_BODY)) {
        const D3 v0 = lds3(px, cap, tf.l0), v1 = lds3(px, cap, tf.l1), v2 = lds3(px, cap, tf.l2);
        const D3 n = crs(sub(v1, v0), sub(v2, v0));
        const double A2 = sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
        if (A2 >= 1.0e-12) {
          const D3 nh3{n.x / A2, n.y / A2, n.z / A2};
          const D3 c0v = crs(sub(v1, v2), nh3), c1v = crs(sub(v2, v0), nh3), c2v = crs(sub(v0, v1), nh3);
          G0 = {0.5 * c0v.x, 0.5 * c0v.y, 0.5 * c0v.z};
          G1 = {0.5 * c1v.x, 0.5 * c1v.y, 0.5 * c1v.z};
          G2 = {0.5 * c2v.x, 0.5 * c2v.y, 0.5 * c2v.z};
          if (tf.flags & TF_OWNER) area += 0.5 * A2;
          if (ATOMIC) {
            if (tf.l0 < n_owned) { atomicAdd(&stg[tf.l0], G0.x); atomicAdd(&stg[T + tf.l0], G0.y); atomicAdd(&stg[2 * T + tf.l0], G0.z); }
            if (tf.l1 < n_owned) { atomicAdd(&stg[tf.l1], G1.x); atomicAdd(&stg[T + tf.l1], G1.y); atomicAdd(&stg[2 * T + tf.l1], G1.z); }
            if (tf.l2 < n_owned) { atomicAdd(&stg[tf.l2], G2.x); atomicAdd(&stg[T + tf.l2], G2.y); atomicAdd(&stg[2 * T + tf.l2], G2.z); }
          }
        }
      }
    }
    if (ATOMIC) continue;
    if (p < f1) {
      double* s = stg + tid;
      s[0 * T] = G0.x; s[1 * T] = G0.y; s[2 * T] = G0.z;
      s[3 * T] = G1.x; s[4 * T] = G1.y; s[5 * T] = G1.z;
      s[6 * T] = G2.x; s[7 * T] = G2.y; s[8 * T] = G2.z;
    }
    __syncthreads();
    {
      const int lo = c0 - f0, hi = min(c0 + T, f1) - f0;
      while (cur < end) {
        const int ent = vent[cur];
        const int fl = ent >> 2;
        if (fl >= hi) break;
        const int k = ent & 3;
        const double* s = stg + (fl - lo);
        gx += s[(3 * k) * T];
        gy += s[(3 * k + 1) * T];
        gz += s[(3 * k + 2) * T];
        ++cur;
      }
    }
    __syncthreads();
  }
  if (ATOMIC) {
    __syncthreads();
    if (tid < n_owned) {
      gx = stg[tid];
      gy = stg[T + tid];
      gz = stg[2 * T + tid];
    }
  }
  double gaga = 0.0;
  if (tid < n_owned) {
    const size_t o = 3 * (size_t)(v_lo + tid);
    a.ga[o] = gx;
    a.ga[o + 1] = gy;
    a.ga[o + 2] = gz;
    gaga = gx * gx + gy * gy + gz * gz;
  }
  area = wg_tree_sum(area, red, T);
  gaga = wg_tree_sum(gaga, red, T);
  if (tid == 0) {
    a.part[(size_t)AP_A * m.n_tiles + tile] = area;
    a.part[(size_t)AP_GAGA * m.n_tiles + tile] = gaga;
  }
}

__global__ __launch_bounds__(AB) void k_area_dots(AreaProjArgs a) {
  __shared__ double red[AB];
  const int tile = a.tile0 + (int)blockIdx.x;
  double ggv = 0.0, gga = 0.0, gvgv = 0.0, gvga = 0.0;
  for (int i = threadIdx.x; i < a.own; i += AB) {
    const int v = tile * a.own + i;
    if (v >= a.nv) break;
    const size_t o = 3 * (size_t)v;
    const double g0 = a.g[o], g1 = a.g[o + 1], g2 = a.g[o + 2];
    const double a0 = a.ga[o], a1 = a.ga[o + 1], a2 = a.ga[o + 2];
    gga += g0 * a0 + g1 * a1 + g2 * a2;
    if (a.gv != nullptr) {
      const double v0 = a.gv[o], v1 = a.gv[o + 1], v2 = a.gv[o + 2];
      ggv += g0 * v0 + g1 * v1 + g2 * v2;
      gvgv += v0 * v0 + v1 * v1 + v2 * v2;
      gvga += v0 * a0 + v1 * a1 + v2 * a2;
    }
  }
  gga = wg_tree_sum(gga, red, AB);
  if (a.gv != nullptr) {  // (uniform over the launch)
    ggv = wg_tree_sum(ggv, red, AB);
    gvgv = wg_tree_sum(gvgv, red, AB);
    gvga = wg_tree_sum(gvga, red, AB);
  }
  if (threadIdx.x == 0) {
    a.part[(size_t)AP_GGA * a.n_tiles + tile] = gga;
    a.part[(size_t)AP_GGV * a.n_tiles + tile] = ggv;
    a.part[(size_t)AP_GVGV * a.n_tiles + tile] = gvgv;
    a.part[(size_t)AP_GVGA * a.n_tiles + tile] = gvga;
  }
}

// rows: 0 the area and <gA,gA> alone; 1 the area row; 2 the volume row, then the area row
__global__ __launch_bounds__(AB) void k_area_fold(const double* part, double* res, int n_tiles, int tile0, int tile1, int rows) {
  __shared__ double red[AB];
  double tot[AP_ROWS];
  for (int r = 0; r < AP_ROWS; ++r) {
    double s = 0.0;
    if (rows != 0 || r == AP_A || r == AP_GAGA)
      for (int t = tile0 + (int)threadIdx.x; t < tile1; t += AB) s += part[(size_t)r * n_tiles + t];
    tot[r] = wg_tree_sum(s, red, AB);
  }
  if (threadIdx.x != 0) return;
  for (int r = 0; r < AP_ROWS; ++r) res[r] = tot[r];
  double lv = 0.0, la = 0.0;
  if (rows == 1) {
    // constraint_manager.py:293-301, one dense row: g -= (<g,gC> / <gC,gC>) gC where <gC,gC> > 1e-18
    if (tot[AP_GAGA] > 1e-18) la = tot[AP_GGA] / tot[AP_GAGA];
  } else if (rows == 2) {
    // constraint_projection.py:101-129: A = C C^T + 1e-18 I, b = C g, C = [gV; gA]
    const double a11 = tot[AP_GVGV] + 1e-18, a12 = tot[AP_GVGA], a22 = tot[AP_GAGA] + 1e-18;
    const double b1 = tot[AP_GGV], b2 = tot[AP_GGA];
    bool solved = false;
    if (a11 > 0.0) {  // Cholesky A = L L^T
      const double l11 = sqrt(a11), l21 = a12 / l11, d = a22 - l21 * l21;
      if (d > 0.0) {
        const double l22 = sqrt(d);
        const double y1 = b1 / l11, y2 = (b2 - l21 * y1) / l22;
        la = y2 / l22;
        lv = (y1 - l21 * la) / l11;
        solved = true;
      }
    }
    if (!solved) {  // LU with partial pivoting; an exactly singular system leaves the gradient alone
      double p11 = a11, p12 = a12, p21 = a12, p22 = a22, q1 = b1, q2 = b2;
      if (fabs(p21) > fabs(p11)) {
        double t = p11; p11 = p21; p21 = t;
        t = p12; p12 = p22; p22 = t;
        t = q1; q1 = q2; q2 = t;
      }
      if (p11 != 0.0) {
        const double f = p21 / p11, u22 = p22 - f * p12;
        if (u22 != 0.0) {
          la = (q2 - f * q1) / u22;
          lv = (q1 - p12 * la) / p11;
        }
      }
      if (!(isfinite(lv) && isfinite(la))) lv = la = 0.0;
    }
  }
  res[AP_LAMV] = lv;
  res[AP_LAMA] = la;
}

__global__ __launch_bounds__(AB) void k_area_apply(AreaProjArgs a) {
  const int tile = a.tile0 + (int)blockIdx.x;
  const double lv = a.gv != nullptr ? a.res[AP_LAMV] : 0.0, la = a.res[AP_LAMA];
  for (int i = threadIdx.x; i < a.own; i += AB) {
    const int v = tile * a.own + i;
    if (v >= a.nv) break;
    const size_t o = 3 * (size_t)v;
    for (int k = 0; k < 3; ++k) {
      double s = la * a.ga[o + k];
      if (a.gv != nullptr) s = lv * a.gv[o + k] + s;
      a.g[o + k] -= s;
    }
  }
}

}  // namespace

size_t area_row_lds_bytes(int T, int cap, bool atomic) {
  return sizeof(double) * (3 * (size_t)cap + (atomic ? 3 : 9) * (size_t)T + (size_t)T);
}

// (none of the four is recorded by the one-tile interpreter: the host flushes it first)
hipError_t launch_area_row(const AreaRowArgs& a, bool atomic, hipStream_t s) {
  const int nb = a.tile1 - a.tile0;
  if (nb <= 0) return hipSuccess;
  if (a.m.T > 512 || a.m.own > a.m.T) return hipErrorInvalidValue;
  const size_t lds = area_row_lds_bytes(a.m.T, a.cap, atomic);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(atomic ? reinterpret_cast<const void*>(k_area_row<true>)
                                                    : reinterpret_cast<const void*>(k_area_row<false>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (atomic) hipLaunchKernelGGL(k_area_row<true>, dim3(nb), dim3(a.m.T), lds, s, a);
  else hipLaunchKernelGGL(k_area_row<false>, dim3(nb), dim3(a.m.T), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_area_dots(const AreaProjArgs& a, hipStream_t s) {
  if (a.tile1 <= a.tile0) return hipSuccess;
  hipLaunchKernelGGL(k_area_dots, dim3(a.tile1 - a.tile0), dim3(AB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_area_fold(const double* part, double* res, int n_tiles, int tile0, int tile1, int rows, hipStream_t s) {
  hipLaunchKernelGGL(k_area_fold, dim3(1), dim3(AB), 0, s, part, res, n_tiles, tile0, tile1, rows);
  return hipGetLastError();
}

hipError_t launch_area_apply(const AreaProjArgs& a, hipStream_t s) {
  if (a.tile1 <= a.tile0) return hipSuccess;
  hipLaunchKernelGGL(k_area_apply, dim3(a.tile1 - a.tile0), dim3(AB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
