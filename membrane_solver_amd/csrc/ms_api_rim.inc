// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_rim_source_in/out -- the rim tables (ms_set_leaflet_rim_source) and the pass next to the disk-target pass:
// k_rim_frame (follow mode), k_rim_coef (once per relaxation) and k_rim_apply.  None of the three is recorded by the
// one-tile interpreter: the pass flushes it first.
namespace {

constexpr EdgeTableMsgs kRimMsgs = {"ms_set_leaflet_rim_source: edge row out of range", "",
                                    "ms_set_leaflet_rim_source: gamma must be finite",
                                    "ms_set_leaflet_rim_source: row permutation out of range"};

// The row -> rim edge CSR from external rows: the builder of the edge lane (ms_api_edge.inc) with a first column of
// ones -- it drops an edge whose first column is 0, and a rim edge with gamma == 0 still makes its ends rim rows (they
// count in the follow mode's mean) -- and gamma as the second column, carried to the CSR.
const char* build_rim_tables(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                             const double* gamma, EdgeTables& t) {
  const std::vector<double> ones((size_t)std::max(n_edges, 0), 1.0);
  return build_edge_tables(nv, iperm, n_edges, tail, head, ones.data(), gamma, kRimMsgs, t);
}

// c . t of the rim rows at x (+ alpha d) into the field's tilt-magnitude partials; gradient: c added into f.grad
int rim_pass(ms_ctx* c, ms_ctx::TiltField& f, bool use_dir, double alpha, const double* tilts, bool gradient) {
  if (!f.rs_set)
    return fail(c, MS_ERR_STATE, "tilt_rim_source active but ms_set_leaflet_rim_source was never called");
  if (!tilts) return fail(c, MS_ERR_STATE, "tilt_rim_source active but its tilt field was never set (ms_set_leaflet_tilts)");
  if (gradient && !f.grad) return fail(c, MS_ERR_STATE, "tilt_rim_source: the field has no tilt gradient buffer");
  if (f.rs.n_touch == 0) {  // tables without an edge: nothing to add; the cells nobody else defines hold 0
    if (c->params.modules & f.mod_tilt) return MS_OK;
    return zero_doubles(c, c->d_partials + (size_t)f.s_etilt * c->til.n_tiles + c->tile0,
                        sizeof(double) * (size_t)(c->tile1 - c->tile0));
  }
  if (int rc = exec_flush(c)) return rc;
  RimArgs a = f.rs;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.tilts = tilts;
  a.tilt_grad = gradient ? f.grad : nullptr;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  a.n_cells = c->tile1 - c->tile0;
  a.slot = f.s_etilt;
  // tilt_<leaflet> off: no pass before this one left anything in the slot's cells
  a.define = (c->params.modules & f.mod_tilt) ? 0 : 1;
  a.center_dev = f.rs_follow ? f.rs_center : nullptr;
  // a relaxation in progress: x is frozen, the coefficients are computed by its first evaluation and reused by the others
  // (the protocol of the disk target's profile, disk_target_pass)
  const bool frozen = c->relax_va_valid && !use_dir;
  ProfScope ps(c, 6);
  if (f.rs_follow && !use_dir && !(frozen && f.rs_coef_valid)) {
    // the center of x; a trial (use_dir) keeps the one of the evaluation at x before it
    HIPCHK(c, launch_rim_frame(a, f.rs_center, c->stream));
    ++f.rs_launches[0];
  }
  a.use_coef = frozen ? 1 : 0;
  if (frozen && !f.rs_coef_valid) {
    HIPCHK(c, launch_rim_coef(a, c->stream));
    ++f.rs_launches[1];
    f.rs_coef_valid = true;
  }
  HIPCHK(c, launch_rim_apply(a, c->stream));
  ++f.rs_launches[2];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_leaflet_rim_source(ms_ctx* c, int leaflet, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* gamma, const ms_rim_source_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_rim_source: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_leaflet_rim_source: the tilt_rim_source modules are not sharded (single GPU only)");
  ms_ctx::TiltField& f = c->tf[1 + leaflet];
  if (f.d_rim) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipFree(f.d_rim));
    f.d_rim = nullptr;
  }
  f.rs = RimArgs{};
  f.rs_set = f.rs_follow = f.rs_coef_valid = false;
  f.rs_center = nullptr;
  c->carry.carry_valid = c->carry.grad_valid = c->carry.maxg2_valid = false;  // (the energies held are the old term's)
  if (!tail) return MS_OK;
  if (n_edges < 0 || !head || !gamma || !p) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_rim_source: bad argument");
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(p->center[k]) || !std::isfinite(p->normal[k]))
      return fail(c, MS_ERR_INVALID, "ms_set_leaflet_rim_source: center and normal must be finite");
    nn += p->normal[k] * p->normal[k];
  }
  nn = std::sqrt(nn);
  if (!(nn >= 1e-15)) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_rim_source: a non-zero plane normal is required");
  EdgeTables tb;
  if (const char* why = build_rim_tables(c->til.nv, c->til.iperm.data(), n_edges, tail, head, gamma, tb))
    return fail(c, MS_ERR_INVALID, why);
  const int tiles = c->tile1 - c->tile0;
  const int ne = (int)tb.et.size(), nt = (int)tb.vrow.size();
  if (nt > 0 && tiles <= 0) return fail(c, MS_ERR_STATE, "ms_set_leaflet_rim_source: the context has no tiles");
  const int grid = nt > 0 ? std::min(tiles, (nt + 255) / 256) : 0;
  // one allocation: doubles first (gamma per CSR entry, the coefficients, the workgroup sums, the module's energy, the
  // follow mode's center, the arrival counter's cell), then the int tables
  const size_t n_dbl = 2 * (size_t)ne + 3 * (size_t)nt + (size_t)std::max(1, grid) + 1 + 3 + 1;
  const size_t n_int = (size_t)nt + (size_t)nt + 1 + 2 * (size_t)ne;
  std::vector<double> blob(n_dbl + (n_int + 1) / 2 + 1, 0.0);
  double* bp = blob.data();
  if (ne) memcpy(bp, tb.ol0.data(), sizeof(double) * 2 * (size_t)ne);
  const size_t o_coef = 2 * (size_t)ne, o_wg = o_coef + 3 * (size_t)nt, o_en = o_wg + (size_t)std::max(1, grid);
  const size_t o_cen = o_en + 1, o_done = o_cen + 3;
  for (int k = 0; k < 3; ++k) bp[o_cen + k] = p->center[k];  // (until the first evaluation at x)
  int32_t* ip = reinterpret_cast<int32_t*>(bp + n_dbl);
  size_t at = 0;
  auto put = [&](const std::vector<int32_t>& v) {
    const size_t o = at;
    if (!v.empty()) memcpy(ip + at, v.data(), sizeof(int32_t) * v.size());
    at += v.size();
    return o;
  };
  const size_t o_v = put(tb.vrow), o_o = put(tb.off), o_x = put(tb.other);
  HIPCHK(c, hipMalloc(&f.d_rim, blob.size() * sizeof(double)));
  HIPCHK(c, hipMemcpy(f.d_rim, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  double* dp = static_cast<double*>(f.d_rim);
  const int32_t* di = reinterpret_cast<const int32_t*>(dp + n_dbl);
  RimArgs& a = f.rs;
  a.n_touch = nt;
  a.vrow = di + o_v;
  a.off = di + o_o;
  a.other = di + o_x;
  a.gamma = dp;
  a.coef = dp + o_coef;
  a.wg_sums = dp + o_wg;
  a.energy = dp + o_en;
  a.done = reinterpret_cast<uint32_t*>(dp + o_done);
  a.grid = grid;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = p->normal[k] / nn;  // tilt_rim_source_in.py:150-159
  }
  f.rs_center = dp + o_cen;
  f.rs_follow = p->follow != 0;
  f.rs_set = true;
  return MS_OK;
}

int ms_rim_source_tables_host(int nv, const int32_t* iperm, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* gamma, int32_t counts[2], int32_t* vrow, int32_t* off, int32_t* other,
                              double* csr_gamma) {
  if (nv < 0 || n_edges < 0 || !iperm || !tail || !head || !gamma || !counts || !vrow || !off || !other || !csr_gamma)
    return fail(nullptr, MS_ERR_INVALID, "ms_rim_source_tables_host: bad argument");
  EdgeTables t;
  if (const char* why = build_rim_tables(nv, iperm, n_edges, tail, head, gamma, t)) return fail(nullptr, MS_ERR_INVALID, why);
  counts[0] = (int32_t)t.et.size();
  counts[1] = (int32_t)t.vrow.size();
  std::copy(t.vrow.begin(), t.vrow.end(), vrow);
  std::copy(t.off.begin(), t.off.end(), off);
  std::copy(t.other.begin(), t.other.end(), other);
  std::copy(t.ol0.begin(), t.ol0.end(), csr_gamma);
  return MS_OK;
}

int ms_get_leaflet_rim_source_energy(ms_ctx* c, int leaflet, double* energy) {
  if (!c || !energy || (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT))
    return fail(c, MS_ERR_INVALID, "ms_get_leaflet_rim_source_energy: bad argument");
  *energy = 0.0;
  const ms_ctx::TiltField& f = c->tf[1 + leaflet];
  if (!f.rs_set || f.rs.n_touch == 0) return MS_OK;  // (0.0 as uploaded until the first evaluation)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, f.rs.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_leaflet_rim_source_stats(ms_ctx* c, int leaflet, double stats[3]) {
  if (!c || !stats || (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)) return MS_ERR_INVALID;
  for (int k = 0; k < 3; ++k) stats[k] = (double)c->tf[1 + leaflet].rs_launches[k];
  return MS_OK;
}

}  // extern "C"
