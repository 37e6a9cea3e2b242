// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): the hard area
// constraints body_area / global_area -- the setter, the KKT row's part in the gradient projection (behind the gradient
// pass, in front of k_direction) and the enforcer loop (ms_project_area).  The kernels are ms_area.hip's; none of them
// is a record of the one-tile interpreter: each launch flushes it first, as the edge lane does.
namespace {

inline bool area_con_set(const ms_ctx* c) { return c->area_con_kind != MS_AREA_NONE; }
// the row takes part in the projection: MS_CON_BODY_AREA in the module word and a body_area target set
inline bool area_row_active(const ms_ctx* c) { return c->area_row && c->area_con_kind == MS_AREA_BODY; }

int area_buffers(ms_ctx* c) {
  if (c->d_area_ga) return MS_OK;
  const size_t row_bytes = sizeof(double) * 3 * (size_t)std::max<int64_t>(1, c->til.nvp);
  const size_t part_bytes = sizeof(double) * AP_ROWS * (size_t)std::max(1, c->til.n_tiles);
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_area_ga), row_bytes));
  HIPCHK(c, hipMemset(c->d_area_ga, 0, row_bytes));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_area_part), part_bytes));
  HIPCHK(c, hipMemset(c->d_area_part, 0, part_bytes));
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_area_res), sizeof(double) * AP_RES));
  HIPCHK(c, hipMemset(c->d_area_res, 0, sizeof(double) * AP_RES));
  return MS_OK;
}

// gA of `x` into d_area_ga, the area and <gA,gA> partials into d_area_part
int area_row_run(ms_ctx* c, const double* x) {
  if (int rc = area_buffers(c)) return rc;
  if (int rc = exec_flush(c)) return rc;
  AreaRowArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = x;
  a.ga = c->d_area_ga;
  a.part = c->d_area_part;
  a.all_facets = c->area_con_kind == MS_AREA_GLOBAL ? 1 : 0;
  a.cap = c->cap;
  HIPCHK(c, launch_area_row(a, !c->deterministic, c->stream));
  ++c->area_launches[0];
  return MS_OK;
}

// The area row's part in the projection of G (queue_energy_and_gradient, behind the gradient pass and the edge terms'
// adds): the row at x, the dot products in one pass over G, lambda on the device, G -= lambda_V gV + lambda_A gA.
// Nothing comes back to the host; k_direction then zeroes the fixed rows of the projected G and does not project.
int area_project_gradient(ms_ctx* c) {
  if (c->stage().cur_gate != nullptr)
    return fail(c, MS_ERR_STATE, "the area constraint row cannot follow a gated gradient pass");
  const bool volrow = (c->params.modules & MS_CON_VOLUME) != 0;
  if (int rc = area_row_run(c, c->buf[MS_BUF_X])) return rc;
  AreaProjArgs p;
  p.tile0 = c->tile0;
  p.tile1 = c->tile1;
  p.nv = c->til.nv;
  p.own = c->til.own;
  p.n_tiles = c->til.n_tiles;
  p.g = c->buf[MS_BUF_G];
  p.gv = volrow ? c->buf[MS_BUF_GC] : nullptr;
  p.ga = c->d_area_ga;
  p.part = c->d_area_part;
  p.res = c->d_area_res;
  if (int rc = exec_flush(c)) return rc;
  HIPCHK(c, launch_area_dots(p, c->stream));
  HIPCHK(c, launch_area_fold(c->d_area_part, c->d_area_res, c->til.n_tiles, c->tile0, c->tile1, volrow ? 2 : 1, c->stream));
  HIPCHK(c, launch_area_apply(p, c->stream));
  ++c->area_launches[1];
  ++c->area_launches[2];
  ++c->area_launches[3];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_area_constraint(ms_ctx* c, int kind, double target_area) {
  if (!c) return MS_ERR_INVALID;
  if (kind != MS_AREA_NONE && kind != MS_AREA_BODY && kind != MS_AREA_GLOBAL)
    return fail(c, MS_ERR_INVALID, "ms_set_area_constraint: kind is MS_AREA_NONE, MS_AREA_BODY or MS_AREA_GLOBAL");
  if (kind != MS_AREA_NONE && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_area_constraint: the area constraints are not sharded (single GPU only)");
  if (kind != MS_AREA_NONE && !(std::isfinite(target_area) && target_area > 0.0))
    return fail(c, MS_ERR_INVALID, "ms_set_area_constraint: the target area must be finite and positive");
  if (kind != c->area_con_kind) c->area_cache_valid = false;  // (another body of facets)
  c->area_con_kind = kind;
  c->area_con_target = kind == MS_AREA_NONE ? 0.0 : target_area;
  // (the gradient held may have been projected against the old row set)
  c->carry.invalidate();
  return MS_OK;
}

int ms_clear_area_constraint(ms_ctx* c) { return ms_set_area_constraint(c, MS_AREA_NONE, 0.0); }

int ms_project_area_cached(ms_ctx* c, double tol, int max_iter, int first_step_cached, int* iters_out, double* area_out) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_project_area: single shard only");
  if (!area_con_set(c)) return fail(c, MS_ERR_STATE, "ms_project_area: no area constraint (ms_set_area_constraint)");
  int it = 0;
  double res[AP_RES] = {0};
  const size_t row_bytes = sizeof(double) * 3 * (size_t)std::max<int64_t>(1, c->til.nvp);
  if (!c->d_area_cache) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_area_cache), row_bytes));
    HIPCHK(c, hipMemset(c->d_area_cache, 0, row_bytes));
  }
  // body_area.py:106-139 / global_area.py:23-51: up to max_iter linearised steps x -= (dA / (|gA|^2 + 1e-18)) gA on the
  // movable rows, |gA|^2 over all rows; `it` counts the steps taken
  for (int pass = 0; pass < max_iter; ++pass) {
    // compute_area_and_gradient (body.py:347-384): area and gradient come from Body's cache on the first pass when the
    // caller says the cache looks current (an evaluation of the volume at this mesh version preceded, which refreshes the
    // cached version but neither the cached area nor its gradient), freshly evaluated (and cached) otherwise
    const bool stale = pass == 0 && first_step_cached != 0 && c->area_cache_valid && c->area_con_kind == MS_AREA_BODY;
    const double* g = c->d_area_cache;
    if (stale) {
      res[AP_A] = c->area_cache_area;
      res[AP_GAGA] = c->area_cache_norm2;
    } else {
      int rc = area_row_run(c, c->buf[MS_BUF_X]);
      if (rc) return rc;
      HIPCHK(c, launch_area_fold(c->d_area_part, c->d_area_res, c->til.n_tiles, c->tile0, c->tile1, 0, c->stream));
      ++c->area_launches[2];
      HIPCHK(c, hipMemcpyAsync(res, c->d_area_res, sizeof(double) * AP_ROWS, hipMemcpyDeviceToHost, c->stream));
      if (c->area_con_kind == MS_AREA_BODY)
        HIPCHK(c, hipMemcpyAsync(c->d_area_cache, c->d_area_ga, row_bytes, hipMemcpyDeviceToDevice, c->stream));
      else
        g = c->d_area_ga;  // (global_area: Mesh.compute_total_area_and_gradient keeps no cache)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (c->area_con_kind == MS_AREA_BODY) {
        c->area_cache_area = res[AP_A];
        c->area_cache_norm2 = res[AP_GAGA];
        c->area_cache_valid = true;
      }
    }
    const double delta = res[AP_A] - c->area_con_target;
    if (std::fabs(delta) < tol) break;
    if (res[AP_GAGA] < 1e-18) break;
    const double lam = delta / (res[AP_GAGA] + 1e-18);
    HIPCHK(c, launch_axpy_masked(c->til.nv, c->d_vflags, c->buf[MS_BUF_X], g, -lam, c->stream));
    c->carry.factors_valid = false;
    c->carry.invalidate_with_bt();
    ++it;
  }
  if (iters_out) *iters_out = it;
  if (area_out) *area_out = res[AP_A];  // (of the last evaluation: the positions before the last step when max_iter ran out)
  return MS_OK;
}

int ms_project_area(ms_ctx* c, double tol, int max_iter, int* iters_out, double* area_out) {
  return ms_project_area_cached(c, tol, max_iter, 0, iters_out, area_out);
}

int ms_area_row(ms_ctx* c, double* row, double* area, double* norm2) {
  if (!c) return MS_ERR_INVALID;
  if (!area_con_set(c)) return fail(c, MS_ERR_STATE, "ms_area_row: no area constraint (ms_set_area_constraint)");
  int rc = area_row_run(c, c->buf[MS_BUF_X]);
  if (rc) return rc;
  HIPCHK(c, launch_area_fold(c->d_area_part, c->d_area_res, c->til.n_tiles, c->tile0, c->tile1, 0, c->stream));
  ++c->area_launches[2];
  double res[AP_ROWS];
  HIPCHK(c, hipMemcpyAsync(res, c->d_area_res, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (area) *area = res[AP_A];
  if (norm2) *norm2 = res[AP_GAGA];
  if (row) return patch_to_ext(c, c->d_area_ga, row, 3);
  return MS_OK;
}

int ms_area_stats(ms_ctx* c, double stats[4]) {
  if (!c || !stats) return fail(c, MS_ERR_INVALID, "ms_area_stats: NULL argument");
  for (int k = 0; k < 4; ++k) stats[k] = (double)c->area_launches[k];
  return MS_OK;
}

}  // extern "C"
