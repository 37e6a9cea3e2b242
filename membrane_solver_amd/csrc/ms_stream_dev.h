// Device-only helpers of the small streaming kernels (ms_edge.hip, ms_rim.hip): 256-thread workgroups that walk a table
// with a grid stride and sum in a fixed order -- thread t takes items t, t + stride, ... in order, then a halving tree in
// LDS -- so a run is bitwise reproducible in both modes of ms_set_deterministic.  Included inside a .hip file only.
#pragma once
#include "ms_internal.h"

namespace ms {
namespace {

constexpr int LB = 256;

struct P3 {
  double x, y, z;
};
// x + alpha d as the tile kernels form it: the trial position of a row is the same double here.  ms_kernels.hip keeps
// its own axpy1; the two must stay the same expression.
__device__ __forceinline__ double axpy1(double x, double alpha, double d) {
#ifdef MS_FP_CONTRACT_OFF
  return x + alpha * d;
#else
  return fma(alpha, d, x);
#endif
}
// row r of x, or of x + alpha d where a direction is given and the row is free; A has x, d, alpha and vflags
template <class A>
__device__ __forceinline__ P3 row_at(const A& a, int r) {
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

// A module's own energy: workgroup w of `grid` publishes its sum s, and whichever workgroup arrives last adds all the
// sums in index order into *energy and resets the counter for the next launch.  Called by every thread of the workgroup.
__device__ __forceinline__ void publish_wg_sum(double s, int w, int grid, double* wg_sums, uint32_t* done, double* energy) {
  __shared__ int is_last;
  if (threadIdx.x == 0) {
    wg_sums[w] = s;
    __threadfence();
    is_last = atomicAdd(done, 1u) == (unsigned)grid - 1u;
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __threadfence();
    double tot = 0.0;
    for (int k = 0; k < grid; ++k) tot += __hip_atomic_load(wg_sums + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *energy = tot;
    *done = 0u;
  }
}

}  // namespace
}  // namespace ms
