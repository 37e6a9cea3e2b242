// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_thetaB_contact_in -- the ring's rows and frame (ms_set_thetab_contact), theta_B (ms_set_thetab_value), its pass
// (addon_passes runs it, never to leave the cells): k_thetab_geom on the positions of the evaluation (once per
// relaxation, whose positions are frozen) and k_thetab_apply; and the scalar update.  Neither kernel is recorded by the
// one-tile interpreter: the pass flushes it first.
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

int thetab_pass(ms_ctx* c, bool use_dir, double alpha, const double* tilts, double* tilt_grad, CellMode cell) {
  if (!c->tb_set)
    return fail(c, MS_ERR_STATE, "tilt_thetaB_contact_in active but ms_set_thetab_contact was never called");
  if (!tilts)
    return fail(c, MS_ERR_STATE, "tilt_thetaB_contact_in active but the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (c->tb.n == 0) return empty_table_cells(c, c->tf[1].s_etilt, cell);
  if (int rc = exec_flush(c)) return rc;
  ThetabArgs a = c->tb;
  thetab_fill(c, a, use_dir, alpha, tilts, tilt_grad);
  a.define = cell == CellMode::DEFINE ? 1 : 0;
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
    if (int rc = drop_table(c, c->d_tb)) return rc;
    c->tb = ThetabArgs{};
    c->tb_set = c->tb_geom_valid = false;
    c->carry.invalidate();  // (the energies held are the old term's)
    return MS_OK;
  };
  if (!rows) return drop_old();
  if (n_rows < 0 || !p) return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: bad argument");
  if (n_rows > MS_THETAB_MAX_ROWS)
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: a ring of " + std::to_string(n_rows) + " rows is above the " +
                                       std::to_string(MS_THETAB_MAX_ROWS) + " one workgroup orders");
  const char* who = "ms_set_thetab_contact";
  double unit[3], u[3], v[3];  // tilt_thetaB_contact_in.py:63-67 the unit normal, :97-111 the in-plane axes
  if (int rc = plane_finite(c, who, p->center, p->normal)) return rc;
  if (!std::isfinite(p->k) || !std::isfinite(p->gamma))
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: k and gamma must be finite");
  if (int rc = plane_frame(c, who, p->normal, unit, u, v)) return rc;
  if (p->work_mode != MS_THETAB_WORK_SCALAR && p->work_mode != MS_THETAB_WORK_FIELD_LINEAR)
    return fail(c, MS_ERR_INVALID, "ms_set_thetab_contact: work_mode must be MS_THETAB_WORK_SCALAR or MS_THETAB_WORK_FIELD_LINEAR");
  const size_t n = (size_t)n_rows, n_pad = (size_t)std::max(n_rows, 1);
  std::vector<int32_t> lib(n_pad, 0);
  {
    std::vector<uint8_t> seen((size_t)c->til.nv, 0);
    if (int rc = ring_rows(c, who, "ring", "a ring", c->til.nv, c->til.iperm.data(), n_rows, rows, seen, lib.data())) return rc;
  }
  if (n_rows > 0 && c->tile1 - c->tile0 <= 0) return fail(c, MS_ERR_STATE, "ms_set_thetab_contact: the context has no tiles");
  // one allocation (ms_table_blob.h): w, r_hat, the record, the scalars, the workgroup's sum, the module's energy, the
  // arrival counter's cell; the int tables (rows, keep: one slot each for a ring without a row)
  TableBlob b;
  const auto h_w = b.f64(n), h_rh = b.f64(3 * n), h_rec = b.f64(4), h_sc = b.f64(3), h_wg = b.f64(1), h_en = b.f64(1),
             h_done = b.f64(1);
  const auto h_rows = b.i32(lib), h_keep = b.i32(n_pad);
  if (int rc = drop_old()) return rc;
  if (int rc = upload_table(c, b, &c->d_tb)) return rc;
  ThetabArgs& a = c->tb;
  a.n = n_rows;
  a.rows = b.at(c->d_tb, h_rows);
  a.keep = b.at(c->d_tb, h_keep);
  a.w = b.at(c->d_tb, h_w);
  a.rhat = b.at(c->d_tb, h_rh);
  a.rec = b.at(c->d_tb, h_rec);
  a.scalars = b.at(c->d_tb, h_sc);
  a.wg_sums = b.at(c->d_tb, h_wg);
  a.energy = b.at(c->d_tb, h_en);
  a.done = b.u32(c->d_tb, h_done);
  a.k = p->k;
  a.gamma = p->gamma;
  a.field_linear = p->work_mode == MS_THETAB_WORK_FIELD_LINEAR ? 1 : 0;
  a.penalty = p->penalty_mode != 0 ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = unit[k];
    a.u[k] = u[k];
    a.v[k] = v[k];
  }
  c->tb_set = true;
  return MS_OK;
}

int ms_set_thetab_value(ms_ctx* c, double theta_b) {
  if (!c) return MS_ERR_INVALID;
  if (!std::isfinite(theta_b)) return fail(c, MS_ERR_INVALID, "ms_set_thetab_value: theta_B must be finite");
  if (theta_b != c->tb_theta)
    c->carry.invalidate();  // (the energies held are the old value's)
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
