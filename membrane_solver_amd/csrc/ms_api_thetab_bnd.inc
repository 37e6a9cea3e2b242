// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_thetaB_boundary_in -- the constraint's ring, frame and row -> facet CSR (ms_set_thetab_boundary), the launches of
// k_tbb_geom / k_tbb_apply the relaxation makes (tbb_geom_run, tbb_apply_run: ms_api_tilt.inc calls them), the
// relaxation's cadence (ms_set_tilt_projection) and the entry points the tests read.  Neither kernel is recorded by the
// one-tile interpreter: the launches flush it first.
namespace {

// The ring row -> incident facet CSR: for ring row i the facets that have it as a corner, in ascending facet order, every
// entry the facet's three rows in the facet's own order.  tri holds library rows; a facet with a row outside
// [0, nv) is skipped (the tiling drops it as well).  ring holds distinct library rows.
void build_tbb_csr(int nv, int nf, const int32_t* tri, int n_rows, const int32_t* ring, std::vector<int32_t>& off,
                   std::vector<int32_t>& fv) {
  std::vector<int32_t> slot((size_t)std::max(nv, 1), -1);
  for (int i = 0; i < n_rows; ++i) slot[(size_t)ring[i]] = i;
  auto valid = [&](int f) {
    for (int k = 0; k < 3; ++k)
      if (tri[3 * (size_t)f + k] < 0 || tri[3 * (size_t)f + k] >= nv) return false;
    return true;
  };
  off.assign((size_t)n_rows + 1, 0);
  for (int f = 0; f < nf; ++f) {
    if (!valid(f)) continue;
    for (int k = 0; k < 3; ++k) {
      const int32_t s = slot[(size_t)tri[3 * (size_t)f + k]];
      if (s >= 0) ++off[(size_t)s + 1];
    }
  }
  for (int i = 0; i < n_rows; ++i) off[(size_t)i + 1] += off[(size_t)i];
  fv.assign(3 * (size_t)off[(size_t)n_rows], 0);
  std::vector<int32_t> cur(off.begin(), off.end() - 1);
  for (int f = 0; f < nf; ++f) {
    if (!valid(f)) continue;
    for (int k = 0; k < 3; ++k) {
      const int32_t s = slot[(size_t)tri[3 * (size_t)f + k]];
      if (s < 0) continue;
      const size_t e = 3 * (size_t)cur[(size_t)s]++;
      for (int j = 0; j < 3; ++j) fv[e + j] = tri[3 * (size_t)f + j];
    }
  }
}

// the context's facets in library rows, by external facet number (-1 rows: a facet the tiling dropped)
void tbb_context_facets(const ms_ctx* c, std::vector<int32_t>& tri) {
  const Tiling& t = c->til;
  tri.assign(3 * (size_t)t.nf, -1);
  for (int tile = 0; tile < t.n_tiles; ++tile) {
    const int v_lo = tile * t.own;
    const int n_owned = std::min(t.nv, v_lo + t.own) - v_lo;
    const int32_t* halo = t.halo_ids.data() + t.tile_halo_off[(size_t)tile];
    for (int32_t p = t.tile_facet_off[(size_t)tile]; p < t.tile_facet_off[(size_t)tile + 1]; ++p) {
      const TileFacet& f = t.tile_facets[(size_t)p];
      if (!(f.flags & TF_OWNER)) continue;
      const uint16_t l[3] = {f.l0, f.l1, f.l2};
      const size_t e = 3 * (size_t)t.tile_facet_ext[(size_t)p];
      for (int k = 0; k < 3; ++k) tri[e + k] = l[k] < n_owned ? v_lo + l[k] : halo[l[k] - n_owned];
    }
  }
}

void tbb_fill(ms_ctx* c, TbbArgs& a, const double* x, bool use_dir, double alpha) {
  a.x = x ? x : c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.vflags = c->d_vflags;
  a.theta_b = c->tb_theta;
  a.fixed_bit = c->tf[1].fixed_bit;
}

}  // namespace

namespace {

bool tbb_active(const ms_ctx* c) { return c->tbb_set && c->tbb.n > 0; }

// d, N_v and keep of the ring on x (nullptr: the context's positions; else a buffer of positions) or on x + alpha d.
// While a relaxation holds x frozen (`frozen`) the table is formed once and kept.
int tbb_geom_run(ms_ctx* c, const double* x, bool use_dir, double alpha, bool frozen) {
  if (!tbb_active(c)) return MS_OK;
  if (frozen && c->tbb_geom_valid) return MS_OK;
  if (int rc = exec_flush(c)) return rc;
  TbbArgs a = c->tbb;
  tbb_fill(c, a, x, use_dir, alpha);
  ProfScope ps(c, 6);
  HIPCHK(c, launch_tbb_geom(a, c->stream));
  ++c->tbb_launches[0];
  c->tbb_geom_valid = frozen;
  return MS_OK;
}

// k_tbb_apply<mode> on the table the last geometry launch left: field = the inner tilts (modes 0 / 1) or the inner tilt
// gradient (mode 2); out: mode 1's target; project: mode 0 applies the tangent projection behind the enforcement
int tbb_apply_run(ms_ctx* c, int mode, double* field, double* out, bool project) {
  if (!tbb_active(c)) return MS_OK;
  if (!field) return fail(c, MS_ERR_STATE, "tilt_thetaB_boundary_in: the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (int rc = exec_flush(c)) return rc;
  TbbArgs a = c->tbb;
  tbb_fill(c, a, nullptr, false, 0.0);
  a.field = field;
  a.out = out;
  a.project = project ? 1 : 0;
  ProfScope ps(c, 6);
  HIPCHK(c, launch_tbb_apply(mode, a, c->stream));
  ++c->tbb_launches[mode == 2 ? 2 : 1];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_thetab_boundary(ms_ctx* c, int n_rows, const int32_t* rows, const ms_thetab_boundary_params* p) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_thetab_boundary: the tilt_thetaB_boundary_in constraint is not sharded (single GPU only)");
  // the table in use is dropped only once the new arguments have passed every check: a refused call leaves it as it was
  auto drop_old = [c]() -> int {
    if (int rc = drop_table(c, c->d_tbb)) return rc;
    c->tbb = TbbArgs{};
    c->tbb_set = c->tbb_geom_valid = false;
    return MS_OK;
  };
  if (!rows) return drop_old();
  if (n_rows < 0 || !p) return fail(c, MS_ERR_INVALID, "ms_set_thetab_boundary: bad argument");
  const char* who = "ms_set_thetab_boundary";
  double unit[3];  // tilt_thetaB_boundary_in.py:41-45, :79-82
  if (int rc = plane_finite(c, who, p->center, p->normal)) return rc;
  // tilt_thetaB_boundary_in.py:77-86: the fitted-plane branch stays host work
  if (int rc = plane_frame(c, who, p->normal, unit)) return rc;
  const int nv = c->til.nv;
  std::vector<int32_t> lib((size_t)n_rows, 0);
  {
    std::vector<uint8_t> seen((size_t)nv, 0);
    if (int rc = ring_rows(c, who, "ring", "a ring", nv, c->til.iperm.data(), n_rows, rows, seen, lib.data())) return rc;
  }
  std::vector<int32_t> off, fv;
  {
    std::vector<int32_t> tri;
    tbb_context_facets(c, tri);
    build_tbb_csr(nv, c->til.nf, tri.data(), n_rows, lib.data(), off, fv);
  }
  // one allocation (ms_table_blob.h): d, N_v; the int tables (rows, off, fv); keep
  const size_t n = (size_t)n_rows;
  TableBlob b;
  const auto h_dir = b.f64(3 * n), h_nrm = b.f64(3 * n);
  const auto h_rows = b.i32(lib), h_off = b.i32(off), h_fv = b.i32(fv);
  const auto h_keep = b.u8(n);
  if (int rc = drop_old()) return rc;
  if (int rc = upload_table(c, b, &c->d_tbb)) return rc;
  TbbArgs& a = c->tbb;
  a.n = n_rows;
  a.dir = b.at(c->d_tbb, h_dir);
  a.nrm = b.at(c->d_tbb, h_nrm);
  a.rows = b.at(c->d_tbb, h_rows);
  a.off = b.at(c->d_tbb, h_off);
  a.fv = b.at(c->d_tbb, h_fv);
  a.keep = b.at(c->d_tbb, h_keep);
  for (int k = 0; k < 3; ++k) {
    a.center[k] = p->center[k];
    a.normal[k] = unit[k];
  }
  c->tbb_set = true;
  return MS_OK;
}

int ms_set_tilt_projection(ms_ctx* c, int cadence, int interval) {
  if (!c) return MS_ERR_INVALID;
  // tilt_relaxation.py:494-510
  if (cadence != MS_TILT_PROJECTION_PER_STEP && cadence != MS_TILT_PROJECTION_PER_PASS)
    return fail(c, MS_ERR_INVALID, "ms_set_tilt_projection: cadence must be MS_TILT_PROJECTION_PER_STEP or MS_TILT_PROJECTION_PER_PASS");
  if (interval < 1) return fail(c, MS_ERR_INVALID, "ms_set_tilt_projection: interval must be >= 1");
  c->tilt_proj_cadence = cadence;
  c->tilt_proj_interval = interval;
  return MS_OK;
}

int ms_thetab_boundary_enforce(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  if (!c->tbb_set) return fail(c, MS_ERR_STATE, "ms_thetab_boundary_enforce: ms_set_thetab_boundary was never called");
  if (!tbb_active(c)) return MS_OK;
  if (!c->tf[1].tilts)
    return fail(c, MS_ERR_STATE, "ms_thetab_boundary_enforce: the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (int rc = tbb_geom_run(c, nullptr, false, 0.0, false)) return rc;
  if (int rc = tbb_apply_run(c, 0, c->tf[1].tilts, nullptr, false)) return rc;
  // the tilt-dependent energies held belong to the tilts before the projection
  c->carry.invalidate_with_bt();
  return MS_OK;
}

int ms_thetab_boundary_directions(ms_ctx* c, double* d, uint8_t* keep) {
  if (!c || !d || !keep) return fail(c, MS_ERR_INVALID, "ms_thetab_boundary_directions: bad argument");
  if (!c->tbb_set) return fail(c, MS_ERR_STATE, "ms_thetab_boundary_directions: ms_set_thetab_boundary was never called");
  if (!tbb_active(c)) return MS_OK;
  if (int rc = tbb_geom_run(c, nullptr, false, 0.0, false)) return rc;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(d, c->tbb.dir, sizeof(double) * 3 * (size_t)c->tbb.n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(keep, c->tbb.keep, (size_t)c->tbb.n, hipMemcpyDeviceToHost));
  return MS_OK;
}

int ms_thetab_boundary_projected_gradient(ms_ctx* c, double* energy, double* grad_in, double* grad_out) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_thetab_boundary_projected_gradient: NULL argument");
  if (!c->tbb_set)
    return fail(c, MS_ERR_STATE, "ms_thetab_boundary_projected_gradient: ms_set_thetab_boundary was never called");
  TiltField* fl[2];
  int nf = 0;
  int rc = leaflet_ready(c, "ms_thetab_boundary_projected_gradient", fl, &nf);
  if (rc) return rc;
  if (!c->tf[1].tilts || !(c->params.modules & c->tf[1].mods()))
    return fail(c, MS_ERR_STATE, "ms_thetab_boundary_projected_gradient: no inner-leaflet module is active");
  rc = tilt_eval(c, false, true);
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  *energy = tilt_energy_from_mailbox(c);
  // tilt_relaxation.py:826-853: the projection, then the fixed rows' zeroing
  rc = tbb_geom_run(c, nullptr, false, 0.0, false);
  if (rc) return rc;
  rc = tbb_apply_run(c, 2, c->tf[1].grad, nullptr, false);
  if (rc) return rc;
  const Tiling& t = c->til;
  double* outs[2] = {grad_in, grad_out};
  for (int l = 0; l < 2; ++l) {
    if (!outs[l]) continue;
    TiltField& f = c->tf[1 + l];
    if (f.tilts && (c->params.modules & f.mods())) {
      rc = patch_to_ext(c, f.grad, outs[l], 3);
      if (rc) return rc;
      for (int e = 0; e < t.nv; ++e)  // (the copy handed out only: the relaxation's own pass clamps its rows itself)
        if (c->h_vflags[(size_t)t.iperm[(size_t)e]] & f.fixed_bit) outs[l][3 * e] = outs[l][3 * e + 1] = outs[l][3 * e + 2] = 0.0;
    } else {
      memset(outs[l], 0, sizeof(double) * 3 * (size_t)c->til.nv);
    }
  }
  return MS_OK;
}

int ms_thetab_boundary_stats(ms_ctx* c, double stats[3]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 3; ++k) stats[k] = (double)c->tbb_launches[k];
  return MS_OK;
}

int ms_thetab_boundary_tables_host(int nv, const int32_t* iperm, int n_facets, const int32_t* tri, int n_rows,
                                   const int32_t* rows, int32_t* off, int32_t* fv) {
  if (nv < 0 || n_facets < 0 || n_rows < 0 || !iperm || !tri || !rows || !off)
    return fail(nullptr, MS_ERR_INVALID, "ms_thetab_boundary_tables_host: bad argument");
  for (int i = 0; i < nv; ++i)
    if (iperm[i] < 0 || iperm[i] >= nv)
      return fail(nullptr, MS_ERR_INVALID, "ms_thetab_boundary_tables_host: row permutation out of range");
  std::vector<int32_t> lib((size_t)n_rows, 0);
  {
    std::vector<uint8_t> seen((size_t)nv, 0);
    if (int rc = ring_rows(nullptr, "ms_thetab_boundary_tables_host", "ring", "a ring", nv, iperm, n_rows, rows, seen, lib.data()))
      return rc;
  }
  std::vector<int32_t> t3(3 * (size_t)n_facets, -1);
  for (int f = 0; f < n_facets; ++f) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && tri[3 * (size_t)f + k] >= 0 && tri[3 * (size_t)f + k] < nv;
    for (int k = 0; k < 3 && ok; ++k) t3[3 * (size_t)f + k] = iperm[tri[3 * (size_t)f + k]];
  }
  std::vector<int32_t> o, v;
  build_tbb_csr(nv, n_facets, t3.data(), n_rows, lib.data(), o, v);
  std::copy(o.begin(), o.end(), off);
  if (fv) std::copy(v.begin(), v.end(), fv);
  return MS_OK;
}

}  // extern "C"
