// rim_slope_match_out on the device (modules/energy/rim_slope_match_out.py:352-629, pointwise_radial_v1 /
// ring_average_radial_v1): the outer leaflet's radial tilt on a rim ring is tied to the small-slope geometric slope
// phi = (h_out - h_rim) / (r_out - r_rim) towards an outer ring, E = 1/2 k sum w (t_out . r_hat - phi)^2, and with a disk
// ring the inner leaflet's to theta_disk - phi, E += 1/2 k sum w (t_in . r_hat - (theta_disk - phi))^2.
//
// The rings are re-ordered by angle from the positions handed to EVERY evaluation (geometry/plane_ops.py:73-103:
// np.argsort of atan2(rel . v, rel . u), the position NOT projected first), and rim and outer entries are paired BY INDEX
// after the ordering -- so, unlike in ms_thetab.hip, where atan2's branch cut starts a ring matters.  k_rsm_geom orders
// the two or three rings one after another by the rank-by-counting of ms_ring_dev.h (the LDS arrays are reused per ring),
// then forms the rim table, the pairing and the disk table.  With unequal counts the outer positions are interpolated at the
// rim's arc-length parameters (:190-229): the segment lengths are formed in parallel into LDS and ONE thread takes their
// running sum in order, as np.cumsum does (n - 1 dependent LDS adds: about 0.15 ms for a ring of 4096 at 80 cycles an
// add; the pass runs once per set of positions).  That reproduces the reference's unnormalised knots bit for bit, not
// its normalised ones: the reference divides by np.sum(seg), a pairwise sum, the device by the running sum's last
// value, so s differs from the reference's in the last bits either way (harmless at the bars in use; the serial form is
// kept for being the simplest one that is fixed-order, not for the rounding).
// searchsorted(side="right") is a binary search per rim entry.  Its result p is in 1 .. n_out and does not decrease along
// the rim, so idx0 = p - 1 is MONOTONE and the rim entries that hit one outer row through idx0 are a contiguous range
// (first0), those through idx1 = idx0 + 1 mod n_out the range of the outer row before it.
//
// k_rsm_apply reads those tables.  Nothing is accumulated with atomics: a thread owns a target row and adds the row's
// terms in the order np.add.at applies them (:573-627: the rim rows, then out0's entries in rim order, then out1's; the
// rim's t_in rows, then the disk's).  The three row tables are pairwise disjoint (the setter checks), so one row is one
// thread's.  Every sum is fixed-order (thread t takes items t, t + 256, ... in order, then a halving tree in LDS;
// ms_stream_dev.h): a run is bitwise reproducible in both modes of ms_set_deterministic.  While a relaxation runs the
// positions are frozen: the geometry pass runs once and every evaluation only applies it.
#include "ms_ring_dev.h"

namespace ms {
namespace {

constexpr int RSM_MAX = MS_RIM_MATCH_MAX_ROWS;

struct RsmShared {
  double key[RSM_MAX];  // a ring's angles; later its segment lengths / arc-length prefix
  int ord[RSM_MAX];
  double red[LB];
  double total[2];      // closed length of the rim, of the outer ring
};

__device__ __forceinline__ double dot_n(const RsmArgs& a, const P3& p) {
  return (p.x - a.center[0]) * a.normal[0] + (p.y - a.center[1]) * a.normal[1] + (p.z - a.center[2]) * a.normal[2];
}

// rows[0 .. n) in the order of their angles about the center -> orow; every thread of the workgroup calls it
__device__ void rsm_order(const RsmArgs& a, const int32_t* rows, int n, int32_t* orow, RsmShared& sh) {
  const int t = threadIdx.x;
  for (int i = t; i < n; i += LB) {
    const P3 p = row_at(a, rows[i]);
    const double rx = p.x - a.center[0], ry = p.y - a.center[1], rz = p.z - a.center[2];
    // plane_ops.py:93-102: rel @ u, rel @ v -- the component along the normal is not taken out first
    const double px = rx * a.u[0] + ry * a.u[1] + rz * a.u[2];
    const double py = rx * a.v[0] + ry * a.v[1] + rz * a.v[2];
    sh.key[i] = atan2(py, px);
    sh.ord[i] = i;
  }
  ring_rank(sh.key, sh.ord, n);
  for (int q = t; q < n; q += LB) orow[q] = rows[sh.ord[q]];
  __syncthreads();  // (orow is read by the whole workgroup from here on; key / ord are free again)
}

// _arc_length_params (:190-201) of an ordered ring: key[q] <- sum of the first q closed-ring segments, / total; returns
// the total (0: the ring has no length and key holds zeros)
__device__ double rsm_arc_params(const RsmArgs& a, const int32_t* orow, int n, RsmShared& sh, int which) {
  const int t = threadIdx.x;
  for (int q = t; q < n; q += LB) {
    const P3 p = row_at(a, orow[q]);
    const P3 pn = row_at(a, orow[q + 1 == n ? 0 : q + 1]);
    sh.key[q] = len3(pn.x - p.x, pn.y - p.y, pn.z - p.z);
  }
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int q = 0; q < n; ++q) {
      const double seg = sh.key[q];
      sh.key[q] = run;
      run += seg;
    }
    sh.total[which] = run;
  }
  __syncthreads();
  const double total = sh.total[which];
  for (int q = t; q < n; q += LB) sh.key[q] = total > 0.0 ? sh.key[q] / total : 0.0;
  __syncthreads();
  return total;
}

// the arc-length weight on the ordered closed ring (:178-187)
__device__ __forceinline__ double rsm_arc_weight(const RsmArgs& a, const int32_t* orow, int n, int q, const P3& p) {
  return ring_arc_weight(a, n, q, p, [orow](int s) { return orow[s]; });
}

__global__ __launch_bounds__(LB) void k_rsm_geom(RsmArgs a) {
  __shared__ RsmShared sh;
  const int t = threadIdx.x;
  const int nr = a.n_rim < RSM_MAX ? a.n_rim : RSM_MAX;  // (the setter refuses a larger ring)
  const int no = a.n_out < RSM_MAX ? a.n_out : RSM_MAX;
  const int nd = a.n_disk < RSM_MAX ? a.n_disk : RSM_MAX;
  rsm_order(a, a.rows_rim, nr, a.orow_rim, sh);
  rsm_order(a, a.rows_out, no, a.orow_out, sh);
  double sum_wd = 0.0;
  if (nd > 0) {
    rsm_order(a, a.rows_disk, nd, a.orow_disk, sh);
    // :523-547 the disk rows' r_hat and, for the mean variant, their arc-length weights
    for (int q = t; q < nd; q += LB) {
      const P3 p = row_at(a, a.orow_disk[q]);
      const P3 r = ring_in_plane(a, p);
      const double rl = len3(r.x, r.y, r.z);
      const bool good = rl > 1e-12;
      const double wd = good ? rsm_arc_weight(a, a.orow_disk, nd, q, p) : 0.0;
      a.rhat_d[3 * q] = good ? r.x / rl : 0.0;
      a.rhat_d[3 * q + 1] = good ? r.y / rl : 0.0;
      a.rhat_d[3 * q + 2] = good ? r.z / rl : 0.0;
      a.w_d[q] = wd;
      sum_wd += wd;
    }
    sum_wd = tree_sum(sum_wd, sh.red);
  }
  // :440-447 unequal counts: the outer ring's knots go to global memory, the rim's parameters stay in LDS
  const bool interp = nr != no;
  bool paired = true;
  if (interp) {
    const double total_out = rsm_arc_params(a, a.orow_out, no, sh, 1);
    for (int j = t; j < no; j += LB) a.s_out[j] = sh.key[j];
    __syncthreads();
    const double total_rim = rsm_arc_params(a, a.orow_rim, nr, sh, 0);
    paired = total_rim > 0.0 && total_out > 0.0 && no >= 2;  // :442-446, :211-212
  }
  double n_valid = 0.0;
  for (int q = t; q < nr; q += LB) {
    const P3 p = row_at(a, a.orow_rim[q]);
    const P3 r = ring_in_plane(a, p);  // (:450-451)
    const double rl = len3(r.x, r.y, r.z);
    const bool good = rl > 1e-12;
    int i0 = q, i1 = q;
    double w0 = 1.0, w1 = 0.0;
    P3 po;
    if (interp && paired) {
      // _interp_ring_positions (:204-229): p = #{j : s_out[j] <= s}, in 1 .. n_out because s_out[0] = 0 <= s
      const double s = sh.key[q];
      int lo = 0, hi = no;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.s_out[mid] <= s) lo = mid + 1; else hi = mid;
      }
      i1 = lo % no;
      i0 = (i1 + no - 1) % no;
      const double s0 = a.s_out[i0];
      double s1 = a.s_out[i1], st = s;
      if (s1 <= s0) s1 += 1.0;
      if (st < s0) st += 1.0;
      const double denom = s1 - s0;
      const double tt = denom > 1e-12 ? (st - s0) / denom : 0.0;
      w1 = tt;
      w0 = 1.0 - tt;
      const P3 p0 = row_at(a, a.orow_out[i0]), p1 = row_at(a, a.orow_out[i1]);
      po = P3{p0.x * w0 + p1.x * w1, p0.y * w0 + p1.y * w1, p0.z * w0 + p1.z * w1};
    } else {
      i0 = i1 = q < no ? q : no - 1;  // (q < no whenever the pairing is the identity; a ring that does not pair is not applied)
      po = row_at(a, a.orow_out[i0]);
    }
    // :481-492
    const double h_rim = dot_n(a, p), h_out = dot_n(a, po);
    const P3 ro = ring_in_plane(a, po);
    const double dr = len3(ro.x, ro.y, ro.z) - rl;
    const double ph = fabs(dr) > 1e-8 ? (h_out - h_rim) / dr : 0.0;
    const bool valid = fabs(dr) > 1e-8 && isfinite(ph) && good && paired;
    a.rhat[3 * q] = good ? r.x / rl : 0.0;
    a.rhat[3 * q + 1] = good ? r.y / rl : 0.0;
    a.rhat[3 * q + 2] = good ? r.z / rl : 0.0;
    a.w[q] = valid ? rsm_arc_weight(a, a.orow_rim, nr, q, p) : 0.0;
    a.phi[q] = valid ? ph : 0.0;
    a.inv_dr[q] = valid ? 1.0 / dr : 0.0;
    a.valid[q] = valid ? 1 : 0;
    a.idx0[q] = i0;
    a.w0[q] = w0;
    a.w1[q] = w1;
    n_valid += valid ? 1.0 : 0.0;
  }
  n_valid = tree_sum(n_valid, sh.red);  // (its barriers also order the idx0 stores before the reads below)
  // first0[j] = first rim entry with idx0 >= j
  for (int j = t; j <= no; j += LB) {
    int lo = 0, hi = nr;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.idx0[mid] < j) lo = mid + 1; else hi = mid;
    }
    a.first0[j] = lo;
  }
  if (t == 0) {
    a.rec[0] = n_valid;
    a.rec[1] = n_valid > 0.0 ? 1.0 : 0.0;  // :453-455 no good row, :493-494 no valid row, and the pairing's returns above
    a.rec[2] = (nd > 0 && nd == nr) ? 1.0 : 0.0;  // :540-541 local_disk
    a.rec[3] = sum_wd;
  }
}

__device__ __forceinline__ double dot_row(const double* f, int row, const double* r3) {
  const size_t o = 3 * (size_t)row;
  return f[o] * r3[0] + f[o + 1] * r3[1] + f[o + 2] * r3[2];
}
__device__ __forceinline__ void add_row(double* f, int row, double c, const double* r3) {
  const size_t o = 3 * (size_t)row;
  f[o] += c * r3[0];
  f[o + 1] += c * r3[1];
  f[o + 2] += c * r3[2];
}

__global__ __launch_bounds__(LB) void k_rsm_apply(RsmArgs a) {
  __shared__ double red[LB];
  const int t = threadIdx.x;
  const int nr = a.n_rim, no = a.n_out, nd = a.n_disk;
  const bool on = a.rec[1] != 0.0;
  const bool local_disk = a.rec[2] != 0.0;
  const double sum_wd = a.rec[3];
  const bool interp = nr != no;
  // :522-556 theta_disk: per entry, or the weighted mean over the disk ring where that ring has a weight
  const bool has_in = on && nd > 0 && (local_disk || sum_wd > 0.0);
  double theta_mean = 0.0;
  if (has_in && !local_disk) {
    double s = 0.0;
    for (int q = t; q < nd; q += LB) s += a.w_d[q] * dot_row(a.t_in, a.orow_disk[q], a.rhat_d + 3 * q);
    theta_mean = tree_sum(s, red) / sum_wd;
  }
  double e_out = 0.0, e_in = 0.0, c_in = 0.0;
  if (on)
    for (int q = t; q < nr; q += LB) {
      const int row = a.orow_rim[q];
      const double* rh = a.rhat + 3 * q;
      const bool valid = a.valid[q] != 0;
      const double w = a.w[q], ph = a.phi[q];
      const double df = valid ? dot_row(a.t_out, row, rh) - ph : 0.0;  // :505-506
      double dfi = 0.0;
      if (has_in && valid) {  // :558-567
        const double th = local_disk ? dot_row(a.t_in, a.orow_disk[q], a.rhat_d + 3 * q) : theta_mean;
        dfi = dot_row(a.t_in, row, rh) - (th - ph);
      }
      e_out += w * df * df;
      e_in += w * dfi * dfi;
      c_in += w * dfi;
      a.dif[q] = df;
      a.dif_in[q] = dfi;
      // the rim row is this thread's: :577-578, :586-587, :615-622
      if (a.tg_out != nullptr) add_row(a.tg_out, row, a.k * w * df, rh);
      if (a.tg_in != nullptr && has_in) add_row(a.tg_in, row, a.k * w * dfi, rh);
      if (a.g != nullptr) add_row(a.g, row, (a.k * w * (df - dfi)) * a.inv_dr[q], a.normal);
    }
  e_out = tree_sum(e_out, red);  // (the barriers order the dif / dif_in stores before the reads below)
  e_in = tree_sum(e_in, red);
  c_in = tree_sum(c_in, red);
  if (on && has_in && a.tg_in != nullptr) {
    // :590-608 the disk rows: -k w diff_in r_hat_d of the paired entry, or coeff (w_d / sum w_d) r_hat_d
    const double coeff = -a.k * c_in;
    for (int q = t; q < nd; q += LB) {
      const double c = local_disk ? (-a.k * a.w[q] * a.dif_in[q]) : coeff * (a.w_d[q] / sum_wd);
      add_row(a.tg_in, a.orow_disk[q], c, a.rhat_d + 3 * q);
    }
  }
  if (on && a.g != nullptr) {
    // :623-627 the outer rows: a thread owns row j and takes out0's entries, then out1's, each in rim order
    for (int j = t; j < no; j += LB) {
      const int row = a.orow_out[j];
      double gx = 0.0, gy = 0.0, gz = 0.0;
      bool any = false;
      for (int pass = 0; pass < (interp ? 2 : 1); ++pass) {
        const int jj = pass == 0 ? j : (j + no - 1) % no;  // idx1 == j where idx0 == j - 1
        for (int q = a.first0[jj]; q < a.first0[jj + 1]; ++q) {
          const double c = -(a.k * a.w[q] * (a.dif[q] - a.dif_in[q])) * a.inv_dr[q];
          const double wt = pass == 0 ? a.w0[q] : a.w1[q];
          if (!any) {  // (the first term goes in as the row's += does; the others follow in order)
            const size_t o = 3 * (size_t)row;
            gx = a.g[o], gy = a.g[o + 1], gz = a.g[o + 2];
            any = true;
          }
          gx += (c * a.normal[0]) * wt;
          gy += (c * a.normal[1]) * wt;
          gz += (c * a.normal[2]) * wt;
        }
      }
      if (any) {
        const size_t o = 3 * (size_t)row;
        a.g[o] = gx, a.g[o + 1] = gy, a.g[o + 2] = gz;
      }
    }
  }
  const double eo = on ? 0.5 * a.k * e_out : 0.0;
  const double ei = has_in ? 0.5 * a.k * e_in : 0.0;
  if (a.partials == nullptr) return;
  const int slots[2] = {a.slot_out, a.slot_in}, defs[2] = {a.define_out, a.define_in};
  const double es[2] = {eo, ei};
  for (int s = 0; s < 2; ++s) {
    if (defs[s] < 0) continue;  // (no inner leaflet term: the slot is not this module's)
    double* cells = a.partials + (size_t)slots[s] * a.n_tiles + a.tile0;
    if (defs[s])  // no pass before this one wrote the slot: the other tiles' cells hold 0
      for (int k = 1 + t; k < a.n_cells; k += LB) cells[k] = 0.0;
    if (t == 0) cells[0] = defs[s] ? es[s] : cells[0] + es[s];
  }
  if (t == 0) {  // the two terms on their own: each rides in another leaflet's slot
    a.rec[4] = eo;
    a.rec[5] = ei;
  }
  publish_wg_sum(eo + ei, 0, 1, a.wg_sums, a.done, a.energy);
}

bool rsm_sizes_ok(const RsmArgs& a) {
  return a.n_rim > 0 && a.n_rim <= RSM_MAX && a.n_out > 0 && a.n_out <= RSM_MAX && a.n_disk >= 0 && a.n_disk <= RSM_MAX;
}

}  // namespace

hipError_t launch_rsm_geom(const RsmArgs& a, hipStream_t s) {
  if (!rsm_sizes_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rsm_geom, dim3(1), dim3(LB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rsm_apply(const RsmArgs& a, hipStream_t s) {
  if (!rsm_sizes_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rsm_apply, dim3(1), dim3(LB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
