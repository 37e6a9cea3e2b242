// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// rim_slope_match_out -- the three rings' rows and frame (ms_set_rim_match), its pass (addon_passes runs it, with a cell
// mode per leaflet: define_out / define_in 1 define, 0 add, -1 leave): k_rsm_geom on the positions of the evaluation
// (once per relaxation, whose positions are frozen) and k_rsm_apply.  Neither kernel is recorded by the one-tile
// interpreter: the pass flushes it first.
namespace {

int rim_match_pass(ms_ctx* c, bool use_dir, double alpha, bool trial_tilts, bool tilt_gradients, double* g_out,
                   CellMode cell_out, CellMode cell_in) {
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
  auto define = [](CellMode m) { return m == CellMode::DEFINE ? 1 : (m == CellMode::ADD ? 0 : -1); };
  a.define_out = define(cell_out);
  a.define_in = define(cell_in);  // (LEAVE without a disk ring)
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
  if (int rc = drop_table(c, c->d_rsm)) return rc;
  c->rsm = RsmArgs{};
  c->rsm_set = c->rsm_geom_valid = false;
  c->tf[1].mod_addons = addon_readers(1, /*rsm_inner=*/false);
  c->carry.invalidate();  // (the energies held are the old term's)
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
  const char* who = "ms_set_rim_match";
  double unit[3], u[3], v[3];  // rim_slope_match_out.py:141-149 the unit normal, geometry/plane_ops.py:21-41 the in-plane axes
  if (int rc = plane_finite(c, who, p->center, p->normal)) return rc;
  if (!std::isfinite(p->strength)) return fail(c, MS_ERR_INVALID, "ms_set_rim_match: the strength must be finite");
  if (int rc = plane_frame(c, who, p->normal, unit, u, v)) return rc;
  std::vector<int32_t> lib[3];
  {
    std::vector<uint8_t> seen((size_t)c->til.nv, 0);  // one map for the three tables: a thread of k_rsm_apply owns a row
    for (int k = 0; k < 3; ++k) {
      lib[k].assign((size_t)std::max(counts[k], 1), 0);
      if (int rc = ring_rows(c, who, names[k], a_names[k], c->til.nv, c->til.iperm.data(), counts[k], tabs[k], seen,
                             lib[k].data(), " (within its ring or in another one)"))
        return rc;
    }
  }
  if (c->tile1 - c->tile0 <= 0) return fail(c, MS_ERR_STATE, "ms_set_rim_match: the context has no tiles");
  // one allocation (ms_table_blob.h); a ring without a disk keeps one slot in each of the disk's tables
  const size_t nr = (size_t)n_rim, no = (size_t)n_outer, nd = (size_t)std::max(n_disk, 1);
  TableBlob b;
  const auto h_rh = b.f64(3 * nr), h_w = b.f64(nr), h_phi = b.f64(nr), h_idr = b.f64(nr), h_w0 = b.f64(nr), h_w1 = b.f64(nr),
             h_dif = b.f64(nr), h_dfi = b.f64(nr), h_so = b.f64(no), h_rhd = b.f64(3 * nd), h_wd = b.f64(nd),
             h_rec = b.f64(6), h_wg = b.f64(1), h_en = b.f64(1), h_done = b.f64(1);
  // (the ordered tables start as the rows themselves: every slot holds a row of its ring before the first geometry pass)
  const auto h_rr = b.i32(lib[0]), h_ro = b.i32(lib[1]), h_rd = b.i32(lib[2]), h_or = b.i32(lib[0]), h_oo = b.i32(lib[1]),
             h_od = b.i32(lib[2]), h_val = b.i32(nr), h_i0 = b.i32(nr), h_f0 = b.i32(no + 1);
  if (int rc = rim_match_drop(c)) return rc;  // (only now: a refused call leaves the tables in use as they were)
  if (int rc = upload_table(c, b, &c->d_rsm)) return rc;
  void* d = c->d_rsm;
  RsmArgs& a = c->rsm;
  a.n_rim = n_rim;
  a.n_out = n_outer;
  a.n_disk = n_disk;
  a.rows_rim = b.at(d, h_rr);
  a.rows_out = b.at(d, h_ro);
  a.rows_disk = b.at(d, h_rd);
  a.orow_rim = b.at(d, h_or);
  a.orow_out = b.at(d, h_oo);
  a.orow_disk = b.at(d, h_od);
  a.valid = b.at(d, h_val);
  a.idx0 = b.at(d, h_i0);
  a.first0 = b.at(d, h_f0);
  a.rhat = b.at(d, h_rh);
  a.w = b.at(d, h_w);
  a.phi = b.at(d, h_phi);
  a.inv_dr = b.at(d, h_idr);
  a.w0 = b.at(d, h_w0);
  a.w1 = b.at(d, h_w1);
  a.dif = b.at(d, h_dif);
  a.dif_in = b.at(d, h_dfi);
  a.s_out = b.at(d, h_so);
  a.rhat_d = b.at(d, h_rhd);
  a.w_d = b.at(d, h_wd);
  a.rec = b.at(d, h_rec);
  a.wg_sums = b.at(d, h_wg);
  a.energy = b.at(d, h_en);
  a.done = b.u32(d, h_done);
  a.k = p->strength;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = unit[k];
    a.u[k] = u[k];
    a.v[k] = v[k];
  }
  c->tf[1].mod_addons = addon_readers(1, /*rsm_inner=*/n_disk > 0);  // (the inner leaflet is read only with a disk ring)
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
