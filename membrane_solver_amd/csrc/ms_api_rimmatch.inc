// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// rim_slope_match_out -- the three rings' rows and frame (ms_set_rim_match), the pass behind every other pass that
// writes the leaflets' tilt-magnitude cells: k_rsm_geom on the positions of the evaluation (once per relaxation, whose
// positions are frozen) and k_rsm_apply.  Neither kernel is recorded by the one-tile interpreter: the pass flushes it
// first.
namespace {

int rim_match_pass(ms_ctx* c, uint32_t modules, bool use_dir, double alpha, bool trial_tilts, bool tilt_gradients,
                   double* g_out, int cell) {
  if (!c->rsm_set)
    return fail(c, MS_ERR_STATE, "rim_slope_match_out active but ms_set_rim_match was never called (or ms_clear_rim_match dropped its tables)");
  ms_ctx::TiltField &fi = c->tf[1], &fo = c->tf[2];
  const bool inner = c->rsm.n_disk > 0;
  if (!fo.tilts || (inner && !fi.tilts))
    return fail(c, MS_ERR_STATE, "rim_slope_match_out active but a leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (tilt_gradients && (!fo.grad || (inner && !fi.grad)))
    return fail(c, MS_ERR_STATE, "rim_slope_match_out: a leaflet has no tilt gradient buffer");
  if (int rc = exec_flush(c)) return rc;
  RsmArgs a = c->rsm;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.t_out = trial_tilts ? fo.trial : fo.tilts;
  a.t_in = inner ? (trial_tilts ? fi.trial : fi.tilts) : nullptr;
  if (!a.t_out || (inner && !a.t_in)) return fail(c, MS_ERR_STATE, "rim_slope_match_out: a leaflet has no trial tilt buffer");
  a.tg_out = tilt_gradients ? fo.grad : nullptr;
  a.tg_in = (tilt_gradients && inner) ? fi.grad : nullptr;
  a.g = g_out;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  a.n_cells = c->tile1 - c->tile0;
  a.slot_out = fo.s_etilt;
  a.slot_in = fi.s_etilt;
  if (cell == RSM_CELL_AUTO) {
    // the modules in front of this one that leave something in the slot's cells; none: this pass defines them
    a.define_out = (modules & (fo.mod_tilt | fo.mod_rs | fo.mod_rb_slot | fo.mod_cpl_slot)) ? 0 : 1;
    a.define_in = !inner ? -1 : ((modules & (fi.mod_tilt | fi.mod_rs | fi.mod_tb)) ? 0 : 1);
  } else if (cell == RSM_CELL_ADD) {
    // behind a gradient pass: only k_tilt<1> rewrites a leaflet's cells; where it did not run they still hold this
    // evaluation's sums
    a.define_out = (modules & fo.mod_tilt) ? 0 : -1;
    a.define_in = (inner && (modules & fi.mod_tilt)) ? 0 : -1;
  } else {
    a.define_out = a.define_in = -1;
  }
  ProfScope ps(c, 6);
  // a relaxation in progress: x is frozen, its first evaluation orders the rings and the others reuse the tables
  const bool frozen = c->tb_relax && !use_dir;
  if (!(frozen && c->rsm_geom_valid)) {
    HIPCHK(c, launch_rsm_geom(a, c->stream));
    ++c->rsm_launches[0];
    c->rsm_geom_valid = frozen;
  }
  HIPCHK(c, launch_rsm_apply(a, c->stream));
  ++c->rsm_launches[1];
  return MS_OK;
}

int rim_match_drop(ms_ctx* c) {
  if (c->d_rsm) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipFree(c->d_rsm));
    c->d_rsm = nullptr;
  }
  c->rsm = RsmArgs{};
  c->rsm_set = c->rsm_geom_valid = false;
  c->tf[1].mod_rsm = 0;
  c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (the energies held are the old term's)
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_rim_match(ms_ctx* c, int n_rim, const int32_t* rim, int n_outer, const int32_t* outer, int n_disk,
                     const int32_t* disk, const ms_rim_match_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_rim_match: the rim_slope_match_out module is not sharded (single GPU only)");
  if (!rim || !outer || !p || n_rim < 1 || n_outer < 1 || n_disk < 0 || (n_disk > 0 && !disk))
    return fail(c, MS_ERR_INVALID, "ms_set_rim_match: bad argument (a rim and an outer ring of at least one row each are required)");
  const int counts[3] = {n_rim, n_outer, n_disk};
  const int32_t* tabs[3] = {rim, outer, disk};
  const char* names[3] = {"rim", "outer", "disk"};
  const char* a_names[3] = {"a rim", "an outer", "a disk"};
  for (int k = 0; k < 3; ++k)
    if (counts[k] > MS_RIM_MATCH_MAX_ROWS)
      return fail(c, MS_ERR_INVALID, std::string("ms_set_rim_match: ") + a_names[k] + " ring of " + std::to_string(counts[k]) +
                                         " rows is above the " + std::to_string(MS_RIM_MATCH_MAX_ROWS) + " one workgroup orders");
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(p->center[k]) || !std::isfinite(p->normal[k]))
      return fail(c, MS_ERR_INVALID, "ms_set_rim_match: center and normal must be finite");
    nn += p->normal[k] * p->normal[k];
  }
  nn = std::sqrt(nn);
  if (!std::isfinite(p->strength)) return fail(c, MS_ERR_INVALID, "ms_set_rim_match: the strength must be finite");
  if (!(nn >= 1e-15)) return fail(c, MS_ERR_INVALID, "ms_set_rim_match: a non-zero plane normal is required");
  const int nv = c->til.nv;
  std::vector<int32_t> lib[3];
  {
    std::vector<uint8_t> seen((size_t)nv, 0);  // one map for the three tables: a thread of k_rsm_apply owns a row
    for (int k = 0; k < 3; ++k) {
      lib[k].assign((size_t)std::max(counts[k], 1), 0);
      for (int i = 0; i < counts[k]; ++i) {
        const int32_t r = tabs[k][i];
        if (r < 0 || r >= nv) return fail(c, MS_ERR_INVALID, std::string("ms_set_rim_match: ") + names[k] + " row out of range");
        if (seen[(size_t)r])
          return fail(c, MS_ERR_INVALID, std::string("ms_set_rim_match: ") + a_names[k] + " row is listed twice (within its ring or in another one)");
        seen[(size_t)r] = 1;
        lib[k][(size_t)i] = c->til.iperm[(size_t)r];
      }
    }
  }
  if (c->tile1 - c->tile0 <= 0) return fail(c, MS_ERR_STATE, "ms_set_rim_match: the context has no tiles");
  // one allocation: doubles first, then the int tables
  const size_t nr = (size_t)n_rim, no = (size_t)n_outer, nd = (size_t)std::max(n_disk, 1);
  size_t od = 0;
  auto dbl = [&od](size_t n) { const size_t o = od; od += n; return o; };
  const size_t o_rh = dbl(3 * nr), o_w = dbl(nr), o_phi = dbl(nr), o_idr = dbl(nr), o_w0 = dbl(nr), o_w1 = dbl(nr),
               o_dif = dbl(nr), o_dfi = dbl(nr), o_so = dbl(no), o_rhd = dbl(3 * nd), o_wd = dbl(nd), o_rec = dbl(6),
               o_wg = dbl(1), o_en = dbl(1), o_done = dbl(1);
  const size_t n_dbl = od;
  size_t oi = 0;
  auto i32 = [&oi](size_t n) { const size_t o = oi; oi += n; return o; };
  const size_t i_rr = i32(nr), i_ro = i32(no), i_rd = i32(nd), i_or = i32(nr), i_oo = i32(no), i_od = i32(nd),
               i_val = i32(nr), i_i0 = i32(nr), i_f0 = i32(no + 1);
  std::vector<double> blob(n_dbl + (oi + 1) / 2, 0.0);
  int32_t* bi = reinterpret_cast<int32_t*>(blob.data() + n_dbl);
  memcpy(bi + i_rr, lib[0].data(), sizeof(int32_t) * nr);
  memcpy(bi + i_ro, lib[1].data(), sizeof(int32_t) * no);
  memcpy(bi + i_rd, lib[2].data(), sizeof(int32_t) * nd);
  // (the ordered tables start as the rows themselves: every slot holds a row of its ring before the first geometry pass)
  memcpy(bi + i_or, lib[0].data(), sizeof(int32_t) * nr);
  memcpy(bi + i_oo, lib[1].data(), sizeof(int32_t) * no);
  memcpy(bi + i_od, lib[2].data(), sizeof(int32_t) * nd);
  if (int rc = rim_match_drop(c)) return rc;  // (only now: a refused call leaves the tables in use as they were)
  HIPCHK(c, hipMalloc(&c->d_rsm, blob.size() * sizeof(double)));
  HIPCHK(c, hipMemcpy(c->d_rsm, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  double* dp = static_cast<double*>(c->d_rsm);
  int32_t* di = reinterpret_cast<int32_t*>(dp + n_dbl);
  RsmArgs& a = c->rsm;
  a.n_rim = n_rim;
  a.n_out = n_outer;
  a.n_disk = n_disk;
  a.rows_rim = di + i_rr;
  a.rows_out = di + i_ro;
  a.rows_disk = di + i_rd;
  a.orow_rim = di + i_or;
  a.orow_out = di + i_oo;
  a.orow_disk = di + i_od;
  a.valid = di + i_val;
  a.idx0 = di + i_i0;
  a.first0 = di + i_f0;
  a.rhat = dp + o_rh;
  a.w = dp + o_w;
  a.phi = dp + o_phi;
  a.inv_dr = dp + o_idr;
  a.w0 = dp + o_w0;
  a.w1 = dp + o_w1;
  a.dif = dp + o_dif;
  a.dif_in = dp + o_dfi;
  a.s_out = dp + o_so;
  a.rhat_d = dp + o_rhd;
  a.w_d = dp + o_wd;
  a.rec = dp + o_rec;
  a.wg_sums = dp + o_wg;
  a.energy = dp + o_en;
  a.done = reinterpret_cast<uint32_t*>(dp + o_done);
  a.k = p->strength;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = p->normal[k] / nn;  // rim_slope_match_out.py:141-149
  }
  // the in-plane axes (geometry/plane_ops.py:21-41)
  double trial[3] = {1.0, 0.0, 0.0};
  if (std::fabs(a.normal[0]) > 0.9) {
    trial[0] = 0.0;
    trial[1] = 1.0;
  }
  const double tn = trial[0] * a.normal[0] + trial[1] * a.normal[1] + trial[2] * a.normal[2];
  double u[3], v[3];
  for (int k = 0; k < 3; ++k) u[k] = trial[k] - tn * a.normal[k];
  const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) u[k] = un < 1e-15 ? (k == 0 ? 1.0 : 0.0) : u[k] / un;
  v[0] = a.normal[1] * u[2] - a.normal[2] * u[1];
  v[1] = a.normal[2] * u[0] - a.normal[0] * u[2];
  v[2] = a.normal[0] * u[1] - a.normal[1] * u[0];
  const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  for (int k = 0; k < 3; ++k) {
    a.u[k] = u[k];
    a.v[k] = vn < 1e-15 ? (k == 1 ? 1.0 : 0.0) : v[k] / vn;
  }
  c->tf[1].mod_rsm = n_disk > 0 ? MS_MOD_RIM_SLOPE_MATCH_OUT : 0;  // (the inner leaflet is read only with a disk ring)
  c->rsm_set = true;
  return MS_OK;
}

int ms_clear_rim_match(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  return rim_match_drop(c);
}

int ms_get_rim_match_energy(ms_ctx* c, double energy[3]) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_rim_match_energy: bad argument");
  energy[0] = energy[1] = energy[2] = 0.0;
  if (!c->rsm_set) return MS_OK;  // (0.0 as uploaded until the first evaluation)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, c->rsm.energy, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(energy + 1, c->rsm.rec + 4, 2 * sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_rim_match_stats(ms_ctx* c, double stats[2]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 2; ++k) stats[k] = (double)c->rsm_launches[k];
  return MS_OK;
}

}  // extern "C"
