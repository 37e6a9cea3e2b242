// tilt_thetaB_boundary_in on the device (modules/constraints/tilt_thetaB_boundary_in.py:162-236 the ring's directions,
// :293-336 the gradient rows, :339-378 the projection): the hard boundary condition t_in . d = theta_B on an inclusion's
// ring of vertices, a tilt-only projection that adds nothing to the energy.
//
// k_tbb_geom, one thread per ring row: r = (p - c) - ((p - c) . n) n, dropped when |r| <= 1e-12; the unit vertex normal
// N_v from the row's incident facets (a ring row -> facet CSR the host built once, every entry the facet's three rows, in
// ascending facet order: sum of (p1 - p0) x (p2 - p0), normalised where its length is >= 1e-12 as Mesh.vertex_normals
// does); d = r_hat - (r_hat . N_v) N_v, dropped when |d| <= 1e-12, else normalised.  A line-search trial pays
// O(ring x valence) for its directions, not a pass over the mesh.  Nothing is sorted, so the ring has no size limit.
//
// k_tbb_apply<MODE> on that table, one thread per ring row, rows distinct (no atomics, bitwise reproducible in both
// modes of ms_set_deterministic); rows with the inner field's fixed bit are skipped:
//   MODE 0  t <- t + (theta_B - t . d) d in place (:370-377); with `project` also t <- t - (t . N_v) N_v behind it
//           (the tangent projection the relaxation applies after an accepted step)
//   MODE 1  out <- P(enforce(t)) of the ring rows, `t` left as it is (the pinned-trial lane)
//   MODE 2  g <- g - ((g . d) / (d . d)) d: the relaxation's gradient projection, row by row (the rows of
//           C^T (C C^T)^-1 C are disjoint: constraint_projection.py:157-345 with a diagonal KKT matrix)
// (the streaming kernels' fixed-order sum helper comes with the header; nothing is summed here)
#pragma clang diagnostic ignored "-Wunused-function"
#include "ms_stream_dev.h"

namespace ms {
namespace {

__global__ __launch_bounds__(LB) void k_tbb_geom(TbbArgs a) {
  const int i = blockIdx.x * LB + threadIdx.x;
  if (i >= a.n) return;
  const P3 p = row_at(a, a.rows[i]);
  const double qx = p.x - a.center[0], qy = p.y - a.center[1], qz = p.z - a.center[2];
  const double qn = qx * a.normal[0] + qy * a.normal[1] + qz * a.normal[2];
  double rx = qx - qn * a.normal[0], ry = qy - qn * a.normal[1], rz = qz - qn * a.normal[2];
  const double rl = len3(rx, ry, rz);
  const bool good = rl > 1e-12;
  rx = good ? rx / rl : 0.0;
  ry = good ? ry / rl : 0.0;
  rz = good ? rz / rl : 0.0;
  double nx = 0.0, ny = 0.0, nz = 0.0;
  for (int k = a.off[i]; k < a.off[i + 1]; ++k) {
    const P3 p0 = row_at(a, a.fv[3 * k]), p1 = row_at(a, a.fv[3 * k + 1]), p2 = row_at(a, a.fv[3 * k + 2]);
    const double ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
    const double vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
    nx += uy * vz - uz * vy;
    ny += uz * vx - ux * vz;
    nz += ux * vy - uy * vx;
  }
  const double nl = len3(nx, ny, nz);
  if (nl >= 1e-12) {
    nx /= nl;
    ny /= nl;
    nz /= nl;
  }
  const double rn = rx * nx + ry * ny + rz * nz;
  double dx = rx - rn * nx, dy = ry - rn * ny, dz = rz - rn * nz;
  const double dl = len3(dx, dy, dz);
  const bool keep = good && dl > 1e-12;
  a.dir[3 * i] = keep ? dx / dl : 0.0;
  a.dir[3 * i + 1] = keep ? dy / dl : 0.0;
  a.dir[3 * i + 2] = keep ? dz / dl : 0.0;
  a.nrm[3 * i] = nx;
  a.nrm[3 * i + 1] = ny;
  a.nrm[3 * i + 2] = nz;
  a.keep[i] = keep ? 1 : 0;
}

template <int MODE>
__global__ __launch_bounds__(LB) void k_tbb_apply(TbbArgs a) {
  const int i = blockIdx.x * LB + threadIdx.x;
  if (i >= a.n) return;
  if (!a.keep[i]) return;
  const int r = a.rows[i];
  if (a.vflags[r] & a.fixed_bit) return;
  const size_t o = 3 * (size_t)r;
  const double dx = a.dir[3 * i], dy = a.dir[3 * i + 1], dz = a.dir[3 * i + 2];
  double tx = a.field[o], ty = a.field[o + 1], tz = a.field[o + 2];
  if (MODE == 2) {
    const double c = (tx * dx + ty * dy + tz * dz) / (dx * dx + dy * dy + dz * dz);
    a.field[o] = tx - c * dx;
    a.field[o + 1] = ty - c * dy;
    a.field[o + 2] = tz - c * dz;
    return;
  }
  const double c = a.theta_b - (tx * dx + ty * dy + tz * dz);
  tx += c * dx;
  ty += c * dy;
  tz += c * dz;
  if (MODE == 1 || a.project) {
    const double nx = a.nrm[3 * i], ny = a.nrm[3 * i + 1], nz = a.nrm[3 * i + 2];
    const double tn = tx * nx + ty * ny + tz * nz;
    tx -= tn * nx;
    ty -= tn * ny;
    tz -= tn * nz;
  }
  double* out = MODE == 1 ? a.out : a.field;
  out[o] = tx;
  out[o + 1] = ty;
  out[o + 2] = tz;
}

}  // namespace

hipError_t launch_tbb_geom(const TbbArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tbb_geom, dim3((a.n + LB - 1) / LB), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tbb_apply(int mode, const TbbArgs& a, hipStream_t s) {
  if (a.n <= 0 || !a.field || (mode == 1 && !a.out)) return hipErrorInvalidValue;
  const dim3 grid((a.n + LB - 1) / LB), block(LB);
  switch (mode) {
    case 0: hipLaunchKernelGGL(k_tbb_apply<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_tbb_apply<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_tbb_apply<2>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace ms
