// tilt_thetaB_contact_in on the device (modules/energy/tilt_thetaB_contact_in.py:200-268 the ring's geometry, :336-405
// the energy): the contact work of the inner leaflet's boundary mode theta_B on an inclusion's ring of vertices.
//
// The ring is re-ordered by angle from the positions it is handed at EVERY evaluation (_order_by_angle, :94-118:
// np.argsort of atan2 of the in-plane projection), so its table is not a CSR the host can build once: k_thetab_geom
// sorts, by the rank-by-counting of ms_ring_dev.h.  Only the cyclic order enters w, so where atan2's branch cut
// starts the ring does not matter.  Then w_i = 1/2 (|p_next - p_i| + |p_i - p_prev|) on the full
// ring (:121-130), the in-plane r of every row, the keep flag |r| > 1e-12 (:250-260: rows are dropped AFTER the weights
// are formed), wsum and R_eff over the kept rows and the two "wsum <= 1e-12" returns as a flag.
//
// k_thetab_apply reads that table: theta_i = t_in,i . r_hat_i, sum w theta and sum w (theta - theta_B)^2, the energy
// of the active modes and, on request, the rows of the inner tilt gradient (one thread owns a row, no atomics).  While
// a relaxation runs the positions are frozen: the geometry pass runs once and every evaluation only applies it.
// Every sum is fixed-order (thread t takes items t, t + 256, ... in order, then a halving tree in LDS;
// ms_stream_dev.h): a run is bitwise reproducible in both modes of ms_set_deterministic.
#include "ms_ring_dev.h"

namespace ms {
namespace {

constexpr int TB_MAX = MS_THETAB_MAX_ROWS;

__global__ __launch_bounds__(LB) void k_thetab_geom(ThetabArgs a) {
  __shared__ double key[TB_MAX];
  __shared__ int ord[TB_MAX];
  __shared__ double red[LB];
  const int n = a.n < TB_MAX ? a.n : TB_MAX;  // (the setter refuses a larger ring)
  const int t = threadIdx.x;
  for (int i = t; i < n; i += LB) {
    const P3 r = ring_in_plane(a, row_at(a, a.rows[i]));  // (:113-114: the ordering takes the component along the normal out first)
    const double px = r.x * a.u[0] + r.y * a.u[1] + r.z * a.u[2];
    const double py = r.x * a.v[0] + r.y * a.v[1] + r.z * a.v[2];
    key[i] = atan2(py, px);
    ord[i] = i;
  }
  ring_rank(key, ord, n);
  double sw_all = 0.0, sw = 0.0, swr = 0.0, nk = 0.0;
  for (int q = t; q < n; q += LB) {
    const int i = ord[q];
    const P3 p = row_at(a, a.rows[i]);
    const double w = ring_arc_weight(a, n, q, p, [&](int s) { return a.rows[ord[s]]; });
    const P3 r = ring_in_plane(a, p);  // (:250-251)
    const double rl = len3(r.x, r.y, r.z);
    const bool keep = rl > 1e-12;
    a.w[i] = w;
    a.keep[i] = keep ? 1 : 0;
    a.rhat[3 * i] = keep ? r.x / rl : 0.0;
    a.rhat[3 * i + 1] = keep ? r.y / rl : 0.0;
    a.rhat[3 * i + 2] = keep ? r.z / rl : 0.0;
    sw_all += w;
    if (keep) {
      sw += w;
      swr += w * rl;
      nk += 1.0;
    }
  }
  sw_all = tree_sum(sw_all, red);
  sw = tree_sum(sw, red);
  swr = tree_sum(swr, red);
  nk = tree_sum(nk, red);
  if (t == 0) {
    // :246-248 the full ring's wsum, :254-255 no row kept, :261-263 the kept rows' wsum
    const bool on = sw_all > 1e-12 && nk > 0.0 && sw > 1e-12;
    a.rec[0] = sw;
    a.rec[1] = on ? swr / sw : 0.0;
    a.rec[2] = nk;
    a.rec[3] = on ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(LB) void k_thetab_apply(ThetabArgs a) {
  __shared__ double red[LB];
  const int t = threadIdx.x;
  const double wsum = a.rec[0], reff = a.rec[1];
  const bool on = a.rec[3] != 0.0;
  const bool work = a.gamma != 0.0, pen = a.penalty != 0 && a.k != 0.0;
  const double two_pi_r_gamma = 2.0 * M_PI * reff * a.gamma;
  double s1 = 0.0, s2 = 0.0;
  if (on)
    for (int i = t; i < a.n; i += LB) {
      if (!a.keep[i]) continue;
      const size_t o = 3 * (size_t)a.rows[i];
      const double rx = a.rhat[3 * i], ry = a.rhat[3 * i + 1], rz = a.rhat[3 * i + 2];
      const double w = a.w[i];
      const double th = a.tilts[o] * rx + a.tilts[o + 1] * ry + a.tilts[o + 2] * rz;
      const double df = th - a.theta_b;
      s1 += w * th;
      s2 += w * df * df;
      if (a.tilt_grad != nullptr) {  // (one thread owns the row; the reference adds the two terms one after the other)
        if (work && a.field_linear) {
          const double c = -(two_pi_r_gamma / wsum) * w;
          a.tilt_grad[o] += c * rx;
          a.tilt_grad[o + 1] += c * ry;
          a.tilt_grad[o + 2] += c * rz;
        }
        if (pen) {
          const double c = a.k * w * df;
          a.tilt_grad[o] += c * rx;
          a.tilt_grad[o + 1] += c * ry;
          a.tilt_grad[o + 2] += c * rz;
        }
      }
    }
  s1 = tree_sum(s1, red);
  s2 = tree_sum(s2, red);
  const double mean = on ? s1 / wsum : 0.0;
  double e = 0.0;
  if (on) {
    if (work) e += -two_pi_r_gamma * (a.field_linear ? mean : a.theta_b);
    if (pen) e += 0.5 * a.k * s2;
  }
  if (t == 0) {
    a.scalars[0] = mean;
    a.scalars[1] = on ? reff : 0.0;
    a.scalars[2] = on ? wsum : 0.0;
  }
  if (a.partials == nullptr) return;  // (the scalar update's evaluation: no cell, no energy)
  double* cells = a.partials + (size_t)a.slot * a.n_tiles + a.tile0;
  if (a.define)  // no pass before this one wrote the slot: the other tiles' cells hold 0
    for (int k = 1 + t; k < a.n_cells; k += LB) cells[k] = 0.0;
  if (t == 0) cells[0] = a.define ? e : cells[0] + e;
  publish_wg_sum(e, 0, 1, a.wg_sums, a.done, a.energy);
}

}  // namespace

hipError_t launch_thetab_geom(const ThetabArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.n > TB_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_thetab_geom, dim3(1), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_thetab_apply(const ThetabArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.n > TB_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_thetab_apply, dim3(1), dim3(LB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
