// The enforce-only shape constraints on the device (modules/constraints/fixed_plane.py, perimeter.py): neither has a
// KKT row, both only move positions inside ConstraintModuleManager.enforce_all.
//
//   k_fixed_plane   grid-stride over the nv real rows of a position buffer: x -= ((x - q) . n) n on the rows that are
//                   not fixed (fixed_plane.py:18-22, :50-53); the plane {n (unit), q} rides in the kernel arguments.
//                   Two rows (48 B, 16-B aligned) per thread as three double2 accesses, the two flags as one 16-bit
//                   load (row by row where the buffer handed in is only 8-B aligned); a pair whose rows are both
//                   fixed is neither loaded nor stored, rows nv .. nvp are never touched.  No LDS, no atomics.  With n = (0, 0, 1), q = 0 the products with the zero components
//                   vanish and d = z exactly, contracted or not: z becomes 0.0 and x, y keep their bits.
//   k_perimeter     ONE workgroup of 256 threads, one launch per enforce call (perimeter.py:27-74): the loops in list
//                   order, every pass of a loop inside the launch, __syncthreads() between the phases -- the workgroup
//                   that writes the positions is the one that reads them.  Per pass: (1) threads stride over the loop's
//                   entries: length, unit direction (kept in scratch) and the partial sums of P; (2) P folded in a
//                   fixed order (wave shuffle, then the four wave sums through LDS), every thread takes
//                   |P - target| < tol from the same double; (3) threads stride over the loop's distinct vertices
//                   through the vertex -> entry CSR (signed, list order: g_v is the reference's own sum, :9-24; entries
//                   shorter than 1e-12 add nothing), g_v kept in scratch, sum |g_v|^2 folded the same way, < 1e-18
//                   ends the loop; (4) x_v -= lam g_v on the rows that are not fixed.  Every sum has one order, so
//                   the kernel is bitwise reproducible in both summation modes.  res[2 l] = passes of loop l that moved
//                   something, res[2 l + 1] = P of its last evaluation.
#include "ms_internal.h"

namespace ms {
namespace {

constexpr int EB = 256;  // threads of both kernels

__device__ __forceinline__ void plane_row(double& x, double& y, double& z, const FixedPlaneArgs& a) {
  const double d = (x - a.q[0]) * a.n[0] + (y - a.q[1]) * a.n[1] + (z - a.q[2]) * a.n[2];
  x -= d * a.n[0];
  y -= d * a.n[1];
  z -= d * a.n[2];
}

__global__ __launch_bounds__(EB) void k_fixed_plane(FixedPlaneArgs a) {
  // row pairs {2 p, 2 p + 1}: 48 B from a 16-B aligned address.  The context's buffers are slices of one allocation at
  // multiples of 24 nvp bytes, so a buffer of an odd nvp may start 8 B off: its rows then all go one by one below
  const bool wide = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int64_t np = wide ? a.nv >> 1 : 0;
  double2* x2 = reinterpret_cast<double2*>(a.x);
  const uint16_t* fl2 = reinterpret_cast<const uint16_t*>(a.vflags);
  const int64_t stride = (int64_t)gridDim.x * EB;
  for (int64_t p = (int64_t)blockIdx.x * EB + threadIdx.x; p < np; p += stride) {
    const unsigned fl = fl2[p];
    const bool m0 = !(fl & VF_FIXED), m1 = !((fl >> 8) & VF_FIXED);
    if (!m0 && !m1) continue;
    double2 u = x2[3 * p], v = x2[3 * p + 1], w = x2[3 * p + 2];
    if (m0) plane_row(u.x, u.y, v.x, a);
    if (m1) plane_row(v.y, w.x, w.y, a);
    x2[3 * p] = u;
    x2[3 * p + 1] = v;
    x2[3 * p + 2] = w;
  }
  // the rows no pair covers: the last one of an odd nv, or every row of a buffer that is not 16-B aligned
  for (int64_t r = 2 * np + (int64_t)blockIdx.x * EB + threadIdx.x; r < a.nv; r += stride) {
    if (a.vflags[r] & VF_FIXED) continue;
    double x = a.x[3 * r], y = a.x[3 * r + 1], z = a.x[3 * r + 2];
    plane_row(x, y, z, a);
    a.x[3 * r] = x;
    a.x[3 * r + 1] = y;
    a.x[3 * r + 2] = z;
  }
}

// fixed-order sum over the workgroup's 256 threads: shuffle tree inside each wave, the four wave sums through LDS; every
// thread gets the same double
__device__ __forceinline__ double wg_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(EB) void k_perimeter(PerimeterArgs a) {
  __shared__ double red[EB / 64];
  const int tid = threadIdx.x;
  double* e_len = a.ent;  // [4][max_ent]: length, unit direction
  double* e_dx = e_len + a.max_ent;
  double* e_dy = e_dx + a.max_ent;
  double* e_dz = e_dy + a.max_ent;
  double* g_x = a.gv;  // [4][max_verts]: g_v, the number of entries that added to it
  double* g_y = g_x + a.max_verts;
  double* g_z = g_y + a.max_verts;
  double* g_n = g_z + a.max_verts;
  for (int l = 0; l < a.n_loops; ++l) {
    const int e0 = a.loop_off[l], e1 = a.loop_off[l + 1];
    const int v0 = a.vert_off[l], v1 = a.vert_off[l + 1];
    const double target = a.target[l];
    int passes = 0;
    double P = 0.0;
    for (int pass = 0; pass < a.max_iter; ++pass) {
      // (1) perimeter.py:46-51 and the directions of :15-19
      double part = 0.0;
      for (int i = e0 + tid; i < e1; i += EB) {
        const size_t t = 3 * (size_t)a.tail[i], h = 3 * (size_t)a.head[i];
        const double vx = a.x[h] - a.x[t], vy = a.x[h + 1] - a.x[t + 1], vz = a.x[h + 2] - a.x[t + 2];
        const double len = sqrt(vx * vx + vy * vy + vz * vz);
        const int k = i - e0;
        e_len[k] = len;
        if (len >= 1e-12) {
          e_dx[k] = vx / len;
          e_dy[k] = vy / len;
          e_dz[k] = vz / len;
        }
        part += len;
      }
      // (2) :53-55 (the barriers inside the sum also publish the scratch rows of (1))
      P = wg_sum(part, red);
      const double delta = P - target;
      if (fabs(delta) < a.tol) break;
      // (3) :57-63
      part = 0.0;
      for (int j = v0 + tid; j < v1; j += EB) {
        double gx = 0.0, gy = 0.0, gz = 0.0;
        int n = 0;
        for (int k = a.csr_off[j]; k < a.csr_off[j + 1]; ++k) {
          const int s = a.csr_ent[k];  // -(entry + 1): the entry's tail, +(entry + 1): its head
          const int e = (s < 0 ? -s : s) - 1 - e0;
          if (e_len[e] < 1e-12) continue;
          const double sg = s < 0 ? -1.0 : 1.0;
          gx += sg * e_dx[e];
          gy += sg * e_dy[e];
          gz += sg * e_dz[e];
          ++n;
        }
        const int q = j - v0;
        g_x[q] = gx;
        g_y[q] = gy;
        g_z[q] = gz;
        g_n[q] = (double)n;
        part += gx * gx + gy * gy + gz * gz;
      }
      const double norm_sq = wg_sum(part, red);
      if (norm_sq < 1e-18) break;
      // (4) :65-74 (a vertex none of whose entries counted is not in the reference's gradient: it stays as it is)
      const double lam = delta / (norm_sq + 1e-18);
      for (int j = v0 + tid; j < v1; j += EB) {
        const int q = j - v0;
        const int r = a.vrow[j];
        if ((a.vflags[r] & VF_FIXED) || g_n[q] == 0.0) continue;
        const size_t o = 3 * (size_t)r;
        a.x[o] -= lam * g_x[q];
        a.x[o + 1] -= lam * g_y[q];
        a.x[o + 2] -= lam * g_z[q];
      }
      ++passes;
      __syncthreads();  // (the next pass, or the next loop, reads what this one wrote)
    }
    if (tid == 0) {
      a.res[2 * l] = (double)passes;
      a.res[2 * l + 1] = P;
    }
  }
}

}  // namespace

// (neither is recorded by the one-tile interpreter: the host flushes it first)
hipError_t launch_fixed_plane(const FixedPlaneArgs& a, hipStream_t s) {
  if (a.nv <= 0) return hipSuccess;
  const bool wide = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int64_t work = std::max<int64_t>(1, wide ? a.nv >> 1 : a.nv);
  const int nb = (int)std::min<int64_t>((work + EB - 1) / EB, 2048);
  hipLaunchKernelGGL(k_fixed_plane, dim3(nb), dim3(EB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_perimeter(const PerimeterArgs& a, hipStream_t s) {
  if (a.n_loops <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_perimeter, dim3(1), dim3(EB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
