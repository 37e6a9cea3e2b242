// Device bodies of the two pin kernels (ms_pins.hip: k_pin_enforce, k_pin_grad), shared with the one-workgroup
// interpreter (ms_exec.inc: CK_PIN_ENFORCE, CK_PIN_GRAD).  Both are one workgroup of PB threads with fixed-order LDS
// trees; the caller hands them their LDS (3 * PB doubles).
#pragma once
#include "ms_internal.h"

namespace ms {
namespace pin_dev {

constexpr int PB = 256;

struct P3 {
  double x, y, z;
};
__device__ __forceinline__ P3 ld3(const double* p) { return P3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(double* p, P3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}
__device__ __forceinline__ double dot3(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ P3 sub3(P3 a, P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3 axpy3(double s, P3 a, P3 b) { return P3{b.x + s * a.x, b.y + s * a.y, b.z + s * a.z}; }

// the reference's _default_tangent: e_x (or e_y when the normal is within 0.9 of e_x) minus its normal part
__device__ inline P3 default_tangent(P3 n) {
  P3 t = fabs(n.x) > 0.9 ? P3{0.0, 1.0, 0.0} : P3{1.0, 0.0, 0.0};
  t = axpy3(-dot3(t, n), n, t);
  const double nrm = sqrt(dot3(t, t));
  return nrm < 1e-15 ? P3{1.0, 0.0, 0.0} : P3{t.x / nrm, t.y / nrm, t.z / nrm};
}
// unit in-plane radial direction of x about centre c (the reference's r-hat; the default tangent at the centre)
__device__ inline P3 radial_hat(P3 x, P3 n, P3 c) {
  const P3 pp = axpy3(-dot3(sub3(x, c), n), n, x);
  const P3 off = sub3(pp, c);
  const double nrm = sqrt(dot3(off, off));
  return nrm < 1e-15 ? default_tangent(n) : P3{off.x / nrm, off.y / nrm, off.z / nrm};
}
__device__ inline P3 onto_circle(P3 x, P3 n, P3 c, double r) {
  const P3 t = radial_hat(x, n, c);
  return P3{c.x + r * t.x, c.y + r * t.y, c.z + r * t.z};
}

// fixed-order sum of NV values per thread over the workgroup; every thread gets the totals
template <int NV>
__device__ inline void tree_sum(double (&v)[NV], double (*red)[PB]) {
  const int t = threadIdx.x;
  for (int k = 0; k < NV; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = PB / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < NV; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
  for (int k = 0; k < NV; ++k) v[k] = red[k][0];
  __syncthreads();
}

// the enforcement program on a.x; red: 3 * PB doubles of LDS
__device__ __forceinline__ void pin_enforce_body(const PinEnforceArgs& a, double (*red)[PB]) {
  double* const X = a.x;
  for (int s = 0; s < a.n_stages; ++s) {
    const int i0 = a.stage_off[s], i1 = a.stage_off[s + 1];
    const int kind = a.stage_kind[s];
    if (kind == MS_PIN_STAGE_FIXED) {
      for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
        const int arg = a.item_arg[i];
        const double* p = a.params + 7 * (size_t)(arg & 0xffffff);
        const P3 n = ld3(p), q = ld3(p + 3);
        double* xr = X + 3 * (size_t)a.item_row[i];
        const P3 x = ld3(xr);
        st3(xr, (arg >> 24) == MS_PIN_OP_PLANE ? axpy3(-dot3(sub3(x, q), n), n, x) : onto_circle(x, n, q, p[6]));
      }
    } else {
      const double* p = a.params + 7 * (size_t)a.stage_param[s];
      const P3 n = ld3(p), base = ld3(p + 3);
      const double inv = 1.0 / (double)(i1 - i0);
      if (kind == MS_PIN_STAGE_PLANE_GROUP) {
        // the centroid of ALL members (before any is moved); members flagged fixed keep their place
        double v[3] = {0.0, 0.0, 0.0};
        for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
          const P3 x = ld3(X + 3 * (size_t)a.item_row[i]);
          v[0] += x.x;
          v[1] += x.y;
          v[2] += x.z;
        }
        tree_sum<3>(v, red);
        const P3 cen{v[0] * inv, v[1] * inv, v[2] * inv};
        for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
          if (a.item_arg[i]) continue;
          double* xr = X + 3 * (size_t)a.item_row[i];
          const P3 x = ld3(xr);
          st3(xr, axpy3(-dot3(sub3(x, cen), n), n, x));
        }
      } else {
        // slide circle: centre = base + t n with t the mean normal offset; radius given or the mean radial distance
        double v[1] = {0.0};
        for (int i = i0 + (int)threadIdx.x; i < i1; i += PB)
          v[0] += dot3(sub3(ld3(X + 3 * (size_t)a.item_row[i]), base), n);
        tree_sum<1>(v, red);
        const P3 c = axpy3(v[0] * inv, n, base);
        double r = p[6];
        if (r < 0.0) {
          double w[1] = {0.0};
          for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
            const P3 x = ld3(X + 3 * (size_t)a.item_row[i]);
            const P3 pp = axpy3(-dot3(sub3(x, c), n), n, x);
            P3 rad = sub3(pp, c);
            rad = axpy3(-dot3(rad, n), n, rad);
            w[0] += sqrt(dot3(rad, rad));
          }
          tree_sum<1>(w, red);
          r = w[0] * inv;
        }
        if (isfinite(r) && r > 0.0) {
          for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
            double* xr = X + 3 * (size_t)a.item_row[i];
            st3(xr, onto_circle(ld3(xr), n, c, r));
          }
        }
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// remove the rows' directions from v at row `row` (kind: plane n; fixed circle n then r-hat about its centre;
// slide-circle member r-hat about the group's base point -- the mean normal offset cancels out of r-hat)
__device__ inline P3 pin_row_project(const PinGradArgs& a, int k, P3 v) {
  const int row = a.grad_row[k], kind = a.grad_kind[k];
  const double* p = a.params + 7 * (size_t)a.grad_param[k];
  const P3 n = ld3(p), c = ld3(p + 3);
  if (kind != MS_PIN_GRAD_RADIAL) v = axpy3(-dot3(v, n), n, v);
  if (kind != MS_PIN_GRAD_PLANE) {
    const P3 rh = radial_hat(ld3(a.x + 3 * (size_t)row), n, c);
    v = axpy3(-dot3(v, rh), rh, v);
  }
  return v;
}

// the project lane's pass on a.g (and a.gc); red: 3 * PB doubles of LDS
__device__ __forceinline__ void pin_grad_body(const PinGradArgs& a, double (*red)[PB]) {
  double* const G = a.g;
  double* const C = a.gc;  // (nullptr without the volume row)
  // <g,gC> and <gC,gC> over the touched rows before and after: the correction the fold adds to tile 0's partials
  double before[2] = {0.0, 0.0};
  if (C) {
    for (int i = threadIdx.x; i < a.n_touch; i += PB) {
      const size_t o = 3 * (size_t)a.touch_row[i];
      const P3 g = ld3(G + o), gc = ld3(C + o);
      before[0] += dot3(g, gc);
      before[1] += dot3(gc, gc);
    }
  }
  __syncthreads();
  // per-row directions (each row once)
  for (int k = threadIdx.x; k < a.n_grad; k += PB) {
    const size_t o = 3 * (size_t)a.grad_row[k];
    st3(G + o, pin_row_project(a, k, ld3(G + o)));
    if (C) st3(C + o, pin_row_project(a, k, ld3(C + o)));
  }
  __threadfence_block();
  __syncthreads();
  // slide-circle normal rows {ref: -n, v: +n}: their null space holds equal normal components over the support,
  // so the projection replaces each normal component by the support's mean
  for (int s = 0; s < a.n_avg; ++s) {
    const int i0 = a.avg_off[s], i1 = a.avg_off[s + 1];
    const P3 n = ld3(a.params + 7 * (size_t)a.avg_param[s]);
    double v[2] = {0.0, 0.0};
    for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
      const size_t o = 3 * (size_t)a.avg_row[i];
      v[0] += dot3(ld3(G + o), n);
      if (C) v[1] += dot3(ld3(C + o), n);
    }
    tree_sum<2>(v, red);
    const double inv = 1.0 / (double)(i1 - i0);
    const double mg = v[0] * inv, mc = v[1] * inv;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += PB) {
      const size_t o = 3 * (size_t)a.avg_row[i];
      const P3 g = ld3(G + o);
      st3(G + o, axpy3(mg - dot3(g, n), n, g));
      if (C) {
        const P3 gc = ld3(C + o);
        st3(C + o, axpy3(mc - dot3(gc, n), n, gc));
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  if (!C) return;
  double after[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < a.n_touch; i += PB) {
    const size_t o = 3 * (size_t)a.touch_row[i];
    const P3 g = ld3(G + o), gc = ld3(C + o);
    after[0] += dot3(g, gc);
    after[1] += dot3(gc, gc);
  }
  double d[3] = {after[0] - before[0], after[1] - before[1], 0.0};
  tree_sum<3>(d, red);
  if (threadIdx.x == 0) {
    a.partials[(size_t)MS_S_GGC * a.n_tiles + a.tile] += d[0];
    a.partials[(size_t)MS_S_GCGC * a.n_tiles + a.tile] += d[1];
  }
}


}  // namespace pin_dev
}  // namespace ms
