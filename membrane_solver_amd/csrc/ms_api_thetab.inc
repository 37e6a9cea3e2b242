// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_thetaB_contact_in -- the ring's rows and frame (ms_set_thetab_contact), theta_B (ms_set_thetab_value), the pass
// behind the inner leaflet's rim source: k_thetab_geom on the positions of the evaluation (once per relaxation, whose
// positions are frozen) and k_thetab_apply; and the scalar update.  Neither kernel is recorded by the one-tile
// interpreter: the pass flushes it first.
namespace {

// the positions, the tilt rows and where the energy goes
void thetab_fill(ms_ctx* c, ThetabArgs& a, bool use_dir, double alpha, const double* tilts, double* tilt_grad) {
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.tilts = tilts;
  a.tilt_grad = tilt_grad;
  a.theta_b = c->tb_theta;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  a.n_cells = c->tile1 - c->tile0;
  a.slot = c->tf[1].s_etilt;
}

int thetab_pass(ms_ctx* c, uint32_t modules, bool use_dir, double alpha, const double* tilts, double* tilt_grad, int cell) {
  if (!c->tb_set)
    return fail(c, MS_ERR_STATE, "tilt_thetaB_contact_in active but ms_set_thetab_contact was never called");
  ms_ctx::TiltField& f = c->tf[1];
  if (!tilts)
    return fail(c, MS_ERR_STATE, "tilt_thetaB_contact_in active but the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  // tilt_in and tilt_rim_source_in off: no pass before this one left anything in the slot's cells
  const bool define = cell == TB_CELL_AUTO ? !(modules & (f.mod_tilt | f.mod_rs)) : cell == TB_CELL_DEFINE;
  if (c->tb.n == 0) {  // a table without a row: nothing to add; the cells nobody else defines hold 0
    if (!define) return MS_OK;
    return zero_doubles(c, c->d_partials + (size_t)f.s_etilt * c->til.n_tiles + c->tile0,
                        sizeof(double) * (size_t)(c->tile1 - c->tile0));
  }
  if (int rc = exec_flush(c)) return rc;
  ThetabArgs a = c->tb;
  thetab_fill(c, a, use_dir, alpha, tilts, tilt_grad);
  a.define = define ? 1 : 0;
  ProfScope ps(c, 6);
  // a relaxation in progress: x is frozen, its first evaluation orders the ring and the others reuse the table
  const bool frozen = c->tb_relax && !use_dir;
  if (!(frozen && c->tb_geom_valid)) {
    HIPCHK(c, launch_thetab_geom(a, c->stream));
    ++c->tb_launches[0];
    c->tb_geom_valid = frozen;
  }
  HIPCHK(c, launch_thetab_apply(a, c->stream));
  ++c->tb_launches[1];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_thetab_contact(ms_ctx* c, int n_rows, const int32_t* rows, const ms_thetab_contact_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_thetab_contact: the tilt_thetaB_contact_in module is not sharded (single GPU only)");
  // the table in use is dropped only once the new arguments have passed every check: a refused call leaves it as it was
  auto drop_old = [c]() -> int {
    if (c->d_tb) {
      HIPCHK(c, hipStreamSynchronize(S(c)));
      HIPCHK(c, hipFree(c->d_tb));
      c->d_tb = nullptr;
    }
    c->tb = ThetabArgs{};
    c->tb_set = c->tb_geom_valid = false;
    c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (the energies held are the old term's)
    return MS_OK;
  };
  if (!rows) return drop_old();
  if (n_rows < 0 || !p) return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: bad argument");
  if (n_rows > MS_THETAB_MAX_ROWS)
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: a ring of " + std::to_string(n_rows) + " rows is above the " +
                                       std::to_string(MS_THETAB_MAX_ROWS) + " one workgroup orders");
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(p->center[k]) || !std::isfinite(p->normal[k]))
      return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: center and normal must be finite");
    nn += p->normal[k] * p->normal[k];
  }
  nn = std::sqrt(nn);
  if (!std::isfinite(p->k) || !std::isfinite(p->gamma))
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: k and gamma must be finite");
  if (!(nn >= 1e-15)) return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: a non-zero plane normal is required");
  if (p->work_mode != MS_THETAB_WORK_SCALAR && p->work_mode != MS_THETAB_WORK_FIELD_LINEAR)
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: work_mode must be MS_THETAB_WORK_SCALAR or MS_THETAB_WORK_FIELD_LINEAR");
  const int nv = c->til.nv;
  std::vector<int32_t> lib((size_t)std::max(n_rows, 1), 0), keep((size_t)std::max(n_rows, 1), 0);
  {
    std::vector<uint8_t> seen((size_t)nv, 0);
    for (int i = 0; i < n_rows; ++i) {
      const int32_t r = rows[i];
      if (r < 0 || r >= nv) return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: ring row out of range");
      if (seen[(size_t)r]) return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: a ring row is listed twice");
      seen[(size_t)r] = 1;
      lib[(size_t)i] = c->til.iperm[(size_t)r];
    }
  }
  if (n_rows > 0 && c->tile1 - c->tile0 <= 0) return fail(c, MS_ERR_STATE, "ms_set_thetab_contact: the context has no tiles");
  // one allocation: doubles first (w, r_hat, the record, the scalars, the workgroup's sum, the module's energy, the
  // arrival counter's cell), then the int tables (rows, keep)
  const size_t n = (size_t)n_rows;
  const size_t o_w = 0, o_rh = o_w + n, o_rec = o_rh + 3 * n, o_sc = o_rec + 4, o_wg = o_sc + 3, o_en = o_wg + 1,
               o_done = o_en + 1, n_dbl = o_done + 1;
  std::vector<double> blob(n_dbl + (2 * lib.size() + 1) / 2, 0.0);
  int32_t* bi = reinterpret_cast<int32_t*>(blob.data() + n_dbl);
  memcpy(bi, lib.data(), sizeof(int32_t) * lib.size());
  memcpy(bi + lib.size(), keep.data(), sizeof(int32_t) * keep.size());
  if (int rc = drop_old()) return rc;
  HIPCHK(c, hipMalloc(&c->d_tb, blob.size() * sizeof(double)));
  HIPCHK(c, hipMemcpy(c->d_tb, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  double* dp = static_cast<double*>(c->d_tb);
  int32_t* di = reinterpret_cast<int32_t*>(dp + n_dbl);
  ThetabArgs& a = c->tb;
  a.n = n_rows;
  a.rows = di;
  a.keep = di + lib.size();
  a.w = dp + o_w;
  a.rhat = dp + o_rh;
  a.rec = dp + o_rec;
  a.scalars = dp + o_sc;
  a.wg_sums = dp + o_wg;
  a.energy = dp + o_en;
  a.done = reinterpret_cast<uint32_t*>(dp + o_done);
  a.k = p->k;
  a.gamma = p->gamma;
  a.field_linear = p->work_mode == MS_THETAB_WORK_FIELD_LINEAR ? 1 : 0;
  a.penalty = p->penalty_mode != 0 ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = p->normal[k] / nn;  // tilt_thetaB_contact_in.py:63-67
  }
  // the in-plane axes (tilt_thetaB_contact_in.py:97-111)
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
  c->tb_set = true;
  return MS_OK;
}

int ms_set_thetab_value(ms_ctx* c, double theta_b) {
  if (!c) return MS_ERR_INVALID;
  if (!std::isfinite(theta_b)) return fail(c, MS_ERR_INVALID, "ms_set_thetab_value: theta_B must be finite");
  if (theta_b != c->tb_theta)
    c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (the energies held are the old value's)
  c->tb_theta = theta_b;
  return MS_OK;
}

int ms_get_thetab_contact_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_thetab_contact_energy: bad argument");
  *energy = 0.0;
  if (!c->tb_set || c->tb.n == 0) return MS_OK;  // (0.0 as uploaded until the first evaluation)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, c->tb.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_get_thetab_contact_scalars(ms_ctx* c, double out[3]) {
  if (!c || !out) return fail(c, MS_ERR_INVALID, "ms_get_thetab_contact_scalars: bad argument");
  out[0] = out[1] = out[2] = 0.0;
  if (!c->tb_set || c->tb.n == 0) return MS_OK;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(out, c->tb.scalars, 3 * sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_update_thetab_value(ms_ctx* c, double* theta_b, int* changed) {
  if (!c || !theta_b || !changed) return fail(c, MS_ERR_INVALID, "ms_update_thetab_value: bad argument");
  *theta_b = c->tb_theta;
  *changed = 0;
  if (!c->tb_set) return fail(c, MS_ERR_STATE, "ms_update_thetab_value: ms_set_thetab_contact was never called");
  // tilt_thetaB_contact_in.py:273-277 the legacy mode only, :298-299 k > 0
  if (!c->tb.penalty || !(c->tb.k > 0.0) || c->tb.n == 0) return MS_OK;
  if (!c->tf[1].tilts)
    return fail(c, MS_ERR_STATE, "ms_update_thetab_value: the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (int rc = exec_flush(c)) return rc;
  ThetabArgs a = c->tb;
  thetab_fill(c, a, false, 0.0, c->tf[1].tilts, nullptr);
  a.partials = nullptr;  // scalars only
  HIPCHK(c, launch_thetab_geom(a, c->stream));
  ++c->tb_launches[0];
  c->tb_geom_valid = false;
  HIPCHK(c, launch_thetab_apply(a, c->stream));
  ++c->tb_launches[1];
  double sc[3];
  if (int rc = ms_get_thetab_contact_scalars(c, sc)) return rc;
  if (!(sc[2] > 0.0)) return MS_OK;  // (:287-288 the ring contributes nothing)
  const double tb = sc[0] + (2.0 * M_PI * sc[1] * c->tb.gamma) / (c->tb.k * sc[2]);
  if (int rc = ms_set_thetab_value(c, tb)) return rc;
  *theta_b = tb;
  *changed = 1;
  return MS_OK;
}

int ms_thetab_contact_stats(ms_ctx* c, double stats[2]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 2; ++k) stats[k] = (double)c->tb_launches[k];
  return MS_OK;
}

}  // extern "C"
