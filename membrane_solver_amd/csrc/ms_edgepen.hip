// edge_length_penalty on the device (modules/energy/edge_length_penalty.py:35-69): E = sum over the edges that carry a
// target length of 0.5 k (|x_h - x_t| - L0)^2, gradient k (L - L0) (x_v - x_o) / L at both ends, an edge shorter than
// 1e-15 contributing nothing to either.  k is the global edge_stiffness; L0 may be 0 and may lie on either side of L.
//
// The second half of the edge lane ms_line.hip opened, with the same structure: both kernels work from tables the host
// built once in the library's row order (ms_set_edge_length_penalty).  k_edgepen_energy runs behind the energy pass (and
// behind k_line_energy when both modules are on: the order of the two adds into a cell is the stream's) and adds its
// per-workgroup sums into the MS_S_ESURF partials, so the fold, the mailbox and every lane of the line search see
// surface + line + edge-penalty energy in one slot.  k_edgepen_grad runs behind the gradient pass and adds into G; one
// thread owns one row, so there are no atomics.  Every sum is fixed-order (thread t takes items t, t + stride, ... in
// order, then a halving tree in LDS): a run is bitwise reproducible in both modes of ms_set_deterministic.
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
__device__ __forceinline__ P3 row_at(const EdgePenEnergyArgs& a, int r) {
  const size_t o = 3 * (size_t)r;
  P3 p{a.x[o], a.x[o + 1], a.x[o + 2]};
  if (a.d != nullptr && !(a.vflags[r] & VF_FIXED))
    p = P3{axpy1(p.x, a.alpha, a.d[o]), axpy1(p.y, a.alpha, a.d[o + 1]), axpy1(p.z, a.alpha, a.d[o + 2])};
  return p;
}
__device__ __forceinline__ double len3(double dx, double dy, double dz) { return sqrt(dx * dx + dy * dy + dz * dz); }

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

__global__ __launch_bounds__(LB) void k_edgepen_energy(EdgePenEnergyArgs a) {
  __shared__ double red[LB];
  __shared__ int is_last;
  const int w = blockIdx.x;
  const long long stride = (long long)a.grid * LB;
  const double half_k = 0.5 * a.k;  // edge_length_penalty.py:58 evaluates (0.5 * k) * delta**2
  double s = 0.0;
  for (long long e = (long long)w * LB + threadIdx.x; e < a.n_edges; e += stride) {
    const P3 xt = row_at(a, a.tail[e]), xh = row_at(a, a.head[e]);
    const double len = len3(xh.x - xt.x, xh.y - xt.y, xh.z - xt.z);
    if (len < 1e-15) continue;  // edge_length_penalty.py:54-55
    const double delta = len - a.l0[e];
    s += half_k * (delta * delta);
  }
  s = tree_sum(s, red);
  if (threadIdx.x == 0) {
    // (no other workgroup of this launch touches the cell; the energy pass before it wrote every tile's, and
    // k_line_energy's add, if any, is complete: same stream)
    a.partials[(size_t)MS_S_ESURF * a.n_tiles + a.tile0 + w] += s;
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

__global__ __launch_bounds__(LB) void k_edgepen_grad(EdgePenGradArgs a) {
  __shared__ double red[LB];
  const long long stride = (long long)a.grid * LB;
  double corr = 0.0;
  for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < a.n_touch; i += stride) {
    const size_t o = 3 * (size_t)a.vrow[i];
    const P3 xv{a.x[o], a.x[o + 1], a.x[o + 2]};
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int k = a.off[i]; k < a.off[i + 1]; ++k) {
      const size_t q = 3 * (size_t)a.other[k];
      const double dx = xv.x - a.x[q], dy = xv.y - a.x[q + 1], dz = xv.z - a.x[q + 2];
      const double len = len3(dx, dy, dz);
      if (len < 1e-15) continue;
      // k (L - L0) (x_v - x_o) / L: +force at the head, -force at the tail (edge_length_penalty.py:63-67)
      const double f = a.k * (len - a.l0[k]) / len;
      gx += f * dx;
      gy += f * dy;
      gz += f * dz;
    }
    a.g[o] += gx;
    a.g[o + 1] += gy;
    a.g[o + 2] += gz;
    if (a.gc != nullptr) corr += gx * a.gc[o] + gy * a.gc[o + 1] + gz * a.gc[o + 2];
  }
  if (a.gc == nullptr) return;  // (uniform over the launch)
  // <g,gC> changes by sum dg_v . gC_v; <gC,gC> does not
  corr = tree_sum(corr, red);
  if (threadIdx.x == 0) a.partials[(size_t)MS_S_GGC * a.n_tiles + a.tile0 + blockIdx.x] += corr;
}

}  // namespace

hipError_t launch_edgepen_energy(const EdgePenEnergyArgs& a, hipStream_t s) {
  if (a.n_edges <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edgepen_energy, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_edgepen_grad(const EdgePenGradArgs& a, hipStream_t s) {
  if (a.n_touch <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edgepen_grad, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
