// The edge lane on the device: energy terms that are a sum over a table of edges of a function of the edge's length.
//
//   EDGE_LINE  line_tension (modules/energy/line_tension.py:103-140): E = sum over the tagged edges of gamma |x_h - x_t|,
//              gradient gamma (x_v - x_o) / |x_v - x_o| at both ends.
//   EDGE_PEN   edge_length_penalty (modules/energy/edge_length_penalty.py:35-69): E = sum over the edges that carry a
//              target length of 0.5 k (|x_h - x_t| - L0)^2, gradient k (L - L0) (x_v - x_o) / L at both ends.  k is the
//              global edge_stiffness; L0 may be 0 and may lie on either side of L.
//
// An edge shorter than 1e-15 contributes nothing to either.  The kernels work from tables the host built once in the
// library's row order (ms_set_line_tension, ms_set_edge_length_penalty): `col` is gamma or L0.  The energy kernel runs
// behind the energy pass and adds its per-workgroup sums into the MS_S_ESURF partials that pass has just written, so the
// fold, the mailbox and every lane of the line search see surface + line + edge-penalty energy in one slot.  The
// gradient kernel runs behind the gradient pass and adds into G; one thread owns one row, so there are no atomics.  With
// both modules on, line_tension's launch goes first: the order of the two adds into a cell is the stream's.  Every sum
// is fixed-order (ms_stream_dev.h).
#include "ms_stream_dev.h"

namespace ms {
namespace {

template <int TERM>
__device__ __forceinline__ void edge_energy_body(const EdgeEnergyArgs& a) {
  __shared__ double red[LB];
  const int w = blockIdx.x;
  const long long stride = (long long)a.grid * LB;
  [[maybe_unused]] const double half_k = 0.5 * a.k;  // edge_length_penalty.py:58 evaluates (0.5 * k) * delta**2
  double s = 0.0;
  for (long long e = (long long)w * LB + threadIdx.x; e < a.n_edges; e += stride) {
    const P3 xt = row_at(a, a.tail[e]), xh = row_at(a, a.head[e]);
    const double len = len3(xh.x - xt.x, xh.y - xt.y, xh.z - xt.z);
    if (len < 1e-15) continue;  // line_tension.py:133-134, edge_length_penalty.py:54-55
    if constexpr (TERM == EDGE_LINE) {
      s += a.col[e] * len;
    } else {
      const double delta = len - a.col[e];
      s += half_k * (delta * delta);
    }
  }
  s = tree_sum(s, red);
  // (no other workgroup of this launch touches the cell; the energy pass before it wrote every tile's, and the add of
  // the term launched before this one, if any, is complete: same stream)
  if (threadIdx.x == 0) a.partials[(size_t)MS_S_ESURF * a.n_tiles + a.tile0 + w] += s;
  publish_wg_sum(s, w, a.grid, a.wg_sums, a.done, a.energy);
}

template <int TERM>
__device__ __forceinline__ void edge_grad_body(const EdgeGradArgs& a) {
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
      // +force at the head, -force at the tail (line_tension.py:136-139, edge_length_penalty.py:63-67)
      double f;
      if constexpr (TERM == EDGE_LINE)
        f = a.col[k] / len;
      else
        f = a.k * (len - a.col[k]) / len;
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

// (the kernel names are what profiles and DESIGN.md's tables go by)
__global__ __launch_bounds__(LB) void k_line_energy(EdgeEnergyArgs a) { edge_energy_body<EDGE_LINE>(a); }
__global__ __launch_bounds__(LB) void k_edgepen_energy(EdgeEnergyArgs a) { edge_energy_body<EDGE_PEN>(a); }
__global__ __launch_bounds__(LB) void k_line_grad(EdgeGradArgs a) { edge_grad_body<EDGE_LINE>(a); }
__global__ __launch_bounds__(LB) void k_edgepen_grad(EdgeGradArgs a) { edge_grad_body<EDGE_PEN>(a); }

}  // namespace

hipError_t launch_edge_energy(int term, const EdgeEnergyArgs& a, hipStream_t s) {
  if (a.n_edges <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(term == EDGE_LINE ? k_line_energy : k_edgepen_energy, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_edge_grad(int term, const EdgeGradArgs& a, hipStream_t s) {
  if (a.n_touch <= 0 || a.grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(term == EDGE_LINE ? k_line_grad : k_edgepen_grad, dim3(a.grid), dim3(LB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
