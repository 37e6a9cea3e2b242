// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_rim_source_in/out -- the rim tables (ms_set_leaflet_rim_source) and their pass: k_rim_frame (follow mode),
// k_rim_coef (once per relaxation) and k_rim_apply -- and tilt_rim_source_bilayer (ms_set_rim_source_bilayer): the same
// tables kept once per context, k_rim_frame / k_rim_coef as they are and k_rim_apply2 on both leaflet fields.
// addon_passes runs both passes, never to leave the cells.  None of the four kernels is recorded by the one-tile
// interpreter: the passes flush it first.
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

// one rim table's state: TiltField's rs_* members (tilt_rim_source_in / _out) or the context's rb_* (the bilayer module)
struct RimState {
  void*& d_rim;
  RimArgs& rs;
  bool& set;
  bool& follow;
  bool& coef_valid;
  double*& center;
  long* launches;
};
RimState rim_state(ms_ctx::TiltField& f) {
  return {f.d_rim, f.rs, f.rs_set, f.rs_follow, f.rs_coef_valid, f.rs_center, f.rs_launches};
}
RimState rim_state(ms_ctx* c) {
  return {c->d_rimb, c->rb, c->rb_set, c->rb_follow, c->rb_coef_valid, c->rb_center, c->rb_launches};
}

// what every rim pass hands its kernels besides the tilts: the positions, the partials' geometry and the frame
void rim_fill(ms_ctx* c, const RimState& st, RimArgs& a, bool use_dir, double alpha, int slot, bool define) {
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.partials = c->d_partials;
  a.n_tiles = c->til.n_tiles;
  a.tile0 = c->tile0;
  a.n_cells = c->tile1 - c->tile0;
  a.slot = slot;
  a.define = define ? 1 : 0;
  a.center_dev = st.follow ? st.center : nullptr;
}

// the followed center and, while a relaxation holds x frozen, the coefficients: computed by the relaxation's first
// evaluation and reused by the others (the protocol of the disk target's profile, disk_target_pass)
int rim_coefficients(ms_ctx* c, const RimState& st, RimArgs& a, bool use_dir) {
  const bool frozen = c->relax_va_valid && !use_dir;
  if (st.follow && !use_dir && !(frozen && st.coef_valid)) {
    // the center of x; a trial (use_dir) keeps the one of the evaluation at x before it
    HIPCHK(c, launch_rim_frame(a, st.center, c->stream));
    ++st.launches[0];
  }
  a.use_coef = frozen ? 1 : 0;
  if (frozen && !st.coef_valid) {
    HIPCHK(c, launch_rim_coef(a, c->stream));
    ++st.launches[1];
    st.coef_valid = true;
  }
  return MS_OK;
}

// tables without an edge or a row: nothing to add; the cells nobody else defines hold 0
int empty_table_cells(ms_ctx* c, int slot, CellMode cell) {
  if (cell != CellMode::DEFINE) return MS_OK;
  return zero_doubles(c, c->d_partials + (size_t)slot * c->til.n_tiles + c->tile0, sizeof(double) * (size_t)(c->tile1 - c->tile0));
}

// c . t of the rim rows at x (+ alpha d) into the field's tilt-magnitude partials; gradient: c added into f.grad
int rim_pass(ms_ctx* c, ms_ctx::TiltField& f, bool use_dir, double alpha, const double* tilts, bool gradient, CellMode cell) {
  if (!f.rs_set)
    return fail(c, MS_ERR_STATE, "tilt_rim_source active but ms_set_leaflet_rim_source was never called");
  if (!tilts) return fail(c, MS_ERR_STATE, "tilt_rim_source active but its tilt field was never set (ms_set_leaflet_tilts)");
  if (gradient && !f.grad) return fail(c, MS_ERR_STATE, "tilt_rim_source: the field has no tilt gradient buffer");
  if (f.rs.n_touch == 0) return empty_table_cells(c, f.s_etilt, cell);
  if (int rc = exec_flush(c)) return rc;
  const RimState st = rim_state(f);
  RimArgs a = f.rs;
  rim_fill(c, st, a, use_dir, alpha, f.s_etilt, cell == CellMode::DEFINE);
  a.tilts = tilts;
  a.tilt_grad = gradient ? f.grad : nullptr;
  ProfScope ps(c, 6);
  if (int rc = rim_coefficients(c, st, a, use_dir)) return rc;
  HIPCHK(c, launch_rim_apply(a, c->stream));
  ++f.rs_launches[2];
  return MS_OK;
}

// tilt_rim_source_bilayer: c . (t_in + t_out) of the rim rows at x (+ alpha d) into the OUTER leaflet's tilt-magnitude
// partials; gradient: c added into both fields' grad
int rim_bilayer_pass(ms_ctx* c, bool use_dir, double alpha, bool trial_tilts, bool gradient, CellMode cell) {
  if (!c->rb_set)
    return fail(c, MS_ERR_STATE, "tilt_rim_source_bilayer active but ms_set_rim_source_bilayer was never called");
  ms_ctx::TiltField &fi = c->tf[1], &fo = c->tf[2];
  const double* t_in = trial_tilts ? fi.trial : fi.tilts;
  const double* t_out = trial_tilts ? fo.trial : fo.tilts;
  if (!t_in || !t_out)
    return fail(c, MS_ERR_STATE, "tilt_rim_source_bilayer active but a leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (gradient && (!fi.grad || !fo.grad))
    return fail(c, MS_ERR_STATE, "tilt_rim_source_bilayer: a leaflet has no tilt gradient buffer");
  if (c->rb.n_touch == 0) return empty_table_cells(c, fo.s_etilt, cell);
  if (int rc = exec_flush(c)) return rc;
  const RimState st = rim_state(c);
  RimArgs a = c->rb;
  rim_fill(c, st, a, use_dir, alpha, fo.s_etilt, cell == CellMode::DEFINE);
  a.tilts = t_in;
  a.tilt_grad = gradient ? fi.grad : nullptr;
  ProfScope ps(c, 6);
  if (int rc = rim_coefficients(c, st, a, use_dir)) return rc;
  HIPCHK(c, launch_rim_apply2(a, t_out, gradient ? fo.grad : nullptr, c->stream));
  ++c->rb_launches[2];
  return MS_OK;
}

// the setters' common part: the old tables freed, the arguments checked, the CSR built and uploaded as ONE blob
int rim_upload(ms_ctx* c, const char* who, const RimState& st, int n_edges, const int32_t* tail, const int32_t* head,
               const double* gamma, const ms_rim_source_params* p) {
  const std::string w(who);
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, w + ": the tilt_rim_source modules are not sharded (single GPU only)");
  if (int rc = drop_table(c, st.d_rim)) return rc;
  st.rs = RimArgs{};
  st.set = st.follow = st.coef_valid = false;
  st.center = nullptr;
  c->carry.invalidate();  // (the energies held are the old term's)
  if (!tail) return MS_OK;
  if (n_edges < 0 || !head || !gamma || !p) return fail(c, MS_ERR_INVALID, w + ": bad argument");
  double unit[3];
  if (int rc = plane_finite(c, who, p->center, p->normal)) return rc;
  if (int rc = plane_frame(c, who, p->normal, unit)) return rc;  // tilt_rim_source_in.py:150-159
  EdgeTables tb;
  if (const char* why = build_rim_tables(c->til.nv, c->til.iperm.data(), n_edges, tail, head, gamma, tb)) {
    // (the builder's texts name the leaflet setter)
    const std::string msg(why);
    const size_t colon = msg.find(':');
    return fail(c, MS_ERR_INVALID, colon == std::string::npos ? w + ": " + msg : w + msg.substr(colon));
  }
  const int tiles = c->tile1 - c->tile0;
  const int ne = (int)tb.et.size(), nt = (int)tb.vrow.size();
  if (nt > 0 && tiles <= 0) return fail(c, MS_ERR_STATE, w + ": the context has no tiles");
  const int grid = nt > 0 ? std::min(tiles, (nt + 255) / 256) : 0;
  // one allocation (ms_table_blob.h): gamma per CSR entry, the coefficients, the workgroup sums, the module's energy,
  // the follow mode's center (the given one until the first evaluation at x), the arrival counter's cell; the int tables
  TableBlob b;
  const auto h_gamma = b.f64(2 * (size_t)ne, tb.ol0.data()), h_coef = b.f64(3 * (size_t)nt);
  const auto h_wg = b.f64((size_t)std::max(1, grid)), h_en = b.f64(1), h_cen = b.f64(3, p->center), h_done = b.f64(1);
  const auto h_v = b.i32(tb.vrow), h_o = b.i32(tb.off), h_x = b.i32(tb.other);
  if (int rc = upload_table(c, b, &st.d_rim)) return rc;
  RimArgs& a = st.rs;
  a.n_touch = nt;
  a.vrow = b.at(st.d_rim, h_v);
  a.off = b.at(st.d_rim, h_o);
  a.other = b.at(st.d_rim, h_x);
  a.gamma = b.at(st.d_rim, h_gamma);
  a.coef = b.at(st.d_rim, h_coef);
  a.wg_sums = b.at(st.d_rim, h_wg);
  a.energy = b.at(st.d_rim, h_en);
  a.done = b.u32(st.d_rim, h_done);
  a.grid = grid;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = unit[k];
  }
  st.center = b.at(st.d_rim, h_cen);
  st.follow = p->follow != 0;
  st.set = true;
  return MS_OK;
}

int rim_energy(ms_ctx* c, const RimState& st, double* energy) {
  *energy = 0.0;
  if (!st.set || st.rs.n_touch == 0) return MS_OK;  // (0.0 as uploaded until the first evaluation)
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(energy, st.rs.energy, sizeof(double), hipMemcpyDeviceToHost));
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_leaflet_rim_source(ms_ctx* c, int leaflet, int n_edges, const int32_t* tail, const int32_t* head,
                              const double* gamma, const ms_rim_source_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_rim_source: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  return rim_upload(c, "ms_set_leaflet_rim_source", rim_state(c->tf[1 + leaflet]), n_edges, tail, head, gamma, p);
}

int ms_set_rim_source_bilayer(ms_ctx* c, int n_edges, const int32_t* tail, const int32_t* head, const double* gamma,
                              const ms_rim_source_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_rim_source_bilayer: the tilt_rim_source_bilayer module is not sharded (single GPU only)");
  return rim_upload(c, "ms_set_rim_source_bilayer", rim_state(c), n_edges, tail, head, gamma, p);
}

int ms_get_rim_source_bilayer_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_rim_source_bilayer_energy: bad argument");
  return rim_energy(c, rim_state(c), energy);
}

int ms_rim_source_bilayer_stats(ms_ctx* c, double stats[3]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 3; ++k) stats[k] = (double)c->rb_launches[k];
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
  return rim_energy(c, rim_state(c->tf[1 + leaflet]), energy);
}

int ms_leaflet_rim_source_stats(ms_ctx* c, int leaflet, double stats[3]) {
  if (!c || !stats || (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)) return MS_ERR_INVALID;
  for (int k = 0; k < 3; ++k) stats[k] = (double)c->tf[1 + leaflet].rs_launches[k];
  return MS_OK;
}

}  // extern "C"
