// tilt_rim_source_in/out on the device (modules/energy/tilt_rim_source_in.py:371-451): E = -sum over the rim edges of
// gamma L 1/2 (t_tail + t_head) . r_hat, with r_hat the in-plane unit vector from the circle's center to the edge's
// midpoint and L the edge's length; tilt gradient -1/2 gamma L r_hat at both ends, no shape gradient.
//
// On given positions the module is linear in the tilt field: E = sum over the rim rows of c_row . t_row with
// c_row = sum over the row's rim edges of -1/2 gamma L r_hat, and the tilt gradient is c itself.  k_rim_coef forms c
// from the row -> rim edge CSR the host built once in the library's row order (ms_set_leaflet_rim_source), one thread
// per rim row and no atomics; k_rim_apply sums c . t and, on request, adds c into the field's tilt gradient.  While a
// relaxation runs the positions are frozen: c is computed once and every evaluation only applies it.  k_rim_frame is
// the follow mode's center: the mean of the rim rows of x.  Every sum is fixed-order (thread t takes items t,
// t + stride, ... in order, then a halving tree in LDS): a run is bitwise reproducible in both modes of
// ms_set_deterministic.
#include "ms_internal.h"

namespace ms {
namespace {

constexpr int LB = 256;

struct P3 {
  double x, y, z;
};
// x + alpha d as the tile kernels form it (ms_kernels.hip, axpy1): the trial position of a row is the same double here
__device__ __forceinline__ double axpy1(double x, double alpha, double d) {
#ifdef MS_FP_CONTRACT_OFF
  return x + alpha * d;
#else
  return fma(alpha, d, x);
#endif
}
__device__ __forceinline__ P3 row_at(const RimArgs& a, int r) {
  const size_t o = 3 * (size_t)r;
  P3 p{a.x[o], a.x[o + 1], a.x[o + 2]};
  if (a.d != nullptr && !(a.vflags[r] & VF_FIXED))
    p = P3{axpy1(p.x, a.alpha, a.d[o]), axpy1(p.y, a.alpha, a.d[o + 1]), axpy1(p.z, a.alpha, a.d[o + 2])};
  return p;
}

// fixed-order sum over the workgroup; every thread gets the total
__device__ double tree_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = LB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}

// c_row of rim row i: its rim edges in CSR order (tilt_rim_source_in.py:409-449 per edge)
__device__ P3 rim_coef_of(const RimArgs& a, long long i) {
  const double cx = a.center_dev ? a.center_dev[0] : a.center[0];
  const double cy = a.center_dev ? a.center_dev[1] : a.center[1];
  const double cz = a.center_dev ? a.center_dev[2] : a.center[2];
  const P3 pv = row_at(a, a.vrow[i]);
  P3 c{0.0, 0.0, 0.0};
  for (int k = a.off[i]; k < a.off[i + 1]; ++k) {
    const P3 po = row_at(a, a.other[k]);
    double rx = 0.5 * (pv.x + po.x) - cx, ry = 0.5 * (pv.y + po.y) - cy, rz = 0.5 * (pv.z + po.z) - cz;
    const double rn_ = rx * a.normal[0] + ry * a.normal[1] + rz * a.normal[2];
    rx -= rn_ * a.normal[0];
    ry -= rn_ * a.normal[1];
    rz -= rn_ * a.normal[2];
    const double rn = sqrt(rx * rx + ry * ry + rz * rz);
    if (!(rn > 1e-12)) continue;  // r_hat = 0 (:429-434)
    const double ex = po.x - pv.x, ey = po.y - pv.y, ez = po.z - pv.z;
    const double f = -0.5 * (a.gamma[k] * sqrt(ex * ex + ey * ey + ez * ez)) / rn;
    c.x += f * rx;
    c.y += f * ry;
    c.z += f * rz;
  }
  return c;
}

__global__ __launch_bounds__(LB) void k_rim_frame(RimArgs a, double* center_out) {
  __shared__ double red[LB];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = threadIdx.x; i < a.n_touch; i += LB) {
    const size_t o = 3 * (size_t)a.vrow[i];
    sx += a.x[o];
    sy += a.x[o + 1];
    sz += a.x[o + 2];
  }
  sx = tree_sum(sx, red);
  sy = tree_sum(sy, red);
  sz = tree_sum(sz, red);
  if (threadIdx.x == 0) {
    center_out[0] = sx / (double)a.n_touch;
    center_out[1] = sy / (double)a.n_touch;
    center_out[2] = sz / (double)a.n_touch;
  }
}

__global__ __launch_bounds__(LB) void k_rim_coef(RimArgs a) {
  const long long stride = (long long)gridDim.x * LB;
  for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < a.n_touch; i += stride) {
    const P3 c = rim_coef_of(a, i);
    a.coef[3 * i] = c.x;
    a.coef[3 * i + 1] = c.y;
    a.coef[3 * i + 2] = c.z;
  }
}

__global__ __launch_bounds__(LB) void k_rim_apply(RimArgs a) {
  __shared__ double red[LB];
  __shared__ int is_last;
  const int w = blockIdx.x;
  const long long stride = (long long)a.grid * LB;
  double s = 0.0;
  for (long long i = (long long)w * LB + threadIdx.x; i < a.n_touch; i += stride) {
    P3 c;
    if (a.use_coef)
      c = P3{a.coef[3 * i], a.coef[3 * i + 1], a.coef[3 * i + 2]};
    else
      c = rim_coef_of(a, i);
    const size_t o = 3 * (size_t)a.vrow[i];
    s += c.x * a.tilts[o] + c.y * a.tilts[o + 1] + c.z * a.tilts[o + 2];
    if (a.tilt_grad != nullptr) {  // (one thread owns the row)
      a.tilt_grad[o] += c.x;
      a.tilt_grad[o + 1] += c.y;
      a.tilt_grad[o + 2] += c.z;
    }
  }
  s = tree_sum(s, red);
  double* cells = a.partials + (size_t)a.slot * a.n_tiles + a.tile0;
  if (a.define && w == 0)  // no pass before this one wrote the slot: the tiles without a workgroup of this launch hold 0
    for (int k = a.grid + threadIdx.x; k < a.n_cells; k += LB) cells[k] = 0.0;
  if (threadIdx.x == 0) {
    // (no other workgroup of this launch touches the cell)
    cells[w] = a.define ? s : cells[w] + s;
    a.wg_sums[w] = s;
    __threadfence();
    is_last = atomicAdd(a.done, 1u) == (unsigned)a.grid - 1u;
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    // the module's own energy: the workgroups' sums in index order, whichever workgroup arrived last
    __threadfence();
    double tot = 0.0;
    for (int k = 0; k < a.grid; ++k) tot += __hip_atomic_load(a.wg_sums + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *a.energy = tot;
    *a.done = 0u;  // (for the next launch)
  }
}

}  // namespace

hipError_t launch_rim_frame(const RimArgs& a, double* center_out, hipStream_t s) {
  if (a.n_touch <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rim_frame, dim3(1), dim3(LB), 0, s, a, center_out);
  return hipGetLastError();
}

hipError_t launch_rim_coef(const RimArgs& a, hipStream_t s) {
  if (a.n_touch <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rim_coef, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rim_apply(const RimArgs& a, hipStream_t s) {
  if (a.n_touch <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rim_apply, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
