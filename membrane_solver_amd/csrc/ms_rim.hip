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
// t + stride, ... in order, then a halving tree in LDS; ms_stream_dev.h): a run is bitwise reproducible in both modes
// of ms_set_deterministic.
#include "ms_stream_dev.h"

namespace ms {
namespace {

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
  // (no other workgroup of this launch touches the cell)
  if (threadIdx.x == 0) cells[w] = a.define ? s : cells[w] + s;
  publish_wg_sum(s, w, a.grid, a.wg_sums, a.done, a.energy);
}

// tilt_rim_source_bilayer (modules/energy/tilt_rim_source_bilayer.py:416-515): the same coefficients applied to both
// leaflet fields in one pass -- E = sum over the rim rows of c_row . (t_in,row + t_out,row), and c_row added into both
// tilt gradients.  k_rim_apply's shape: a.tilts / a.tilt_grad are the inner leaflet's, t_out / tg_out the outer one's;
// c_row comes from the cache or from rim_coef_of, so its doubles are the ones tilt_rim_source_in / _out get.
__global__ __launch_bounds__(LB) void k_rim_apply2(RimArgs a, const double* __restrict__ t_out, double* __restrict__ tg_out) {
  __shared__ double red[LB];
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
    s += c.x * (a.tilts[o] + t_out[o]) + c.y * (a.tilts[o + 1] + t_out[o + 1]) + c.z * (a.tilts[o + 2] + t_out[o + 2]);
    if (a.tilt_grad != nullptr) {  // (one thread owns the row, in both fields)
      a.tilt_grad[o] += c.x;
      a.tilt_grad[o + 1] += c.y;
      a.tilt_grad[o + 2] += c.z;
      tg_out[o] += c.x;
      tg_out[o + 1] += c.y;
      tg_out[o + 2] += c.z;
    }
  }
  s = tree_sum(s, red);
  double* cells = a.partials + (size_t)a.slot * a.n_tiles + a.tile0;
  if (a.define && w == 0)  // no pass before this one wrote the slot: the tiles without a workgroup of this launch hold 0
    for (int k = a.grid + threadIdx.x; k < a.n_cells; k += LB) cells[k] = 0.0;
  // (no other workgroup of this launch touches the cell)
  if (threadIdx.x == 0) cells[w] = a.define ? s : cells[w] + s;
  publish_wg_sum(s, w, a.grid, a.wg_sums, a.done, a.energy);
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

hipError_t launch_rim_apply2(const RimArgs& a, const double* t_out, double* tg_out, hipStream_t s) {
  if (a.n_touch <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rim_apply2, dim3(a.grid), dim3(LB), 0, s, a, t_out, tg_out);
  return hipGetLastError();
}

}  // namespace ms
