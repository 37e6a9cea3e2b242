// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_coupling -- its setter and getters, and its pass (addon_passes runs it): k_couple<0> / k_couple<1> on
// x (+ alpha d), k_couple_vec while a relaxation holds the positions frozen.  Neither kernel is recorded by the
// one-tile interpreter: the pass flushes it first.  No host-side table: the kernels work from the tiling alone.
namespace {

int couple_pass(ms_ctx* c, bool use_dir, double alpha, bool tilt_gradients, bool trial_tilts, double* g_out, CellMode cell) {
  const bool gradient_into_g = g_out != nullptr;
  if (c->cpl_sign == 0 || !c->d_cpl)
    return fail(c, MS_ERR_STATE, "tilt_coupling active but ms_set_tilt_coupling was never called (or switched it off)");
  ms_ctx::TiltField &fi = c->tf[1], &fo = c->tf[2];
  if (!fi.tilts || !fo.tilts)
    return fail(c, MS_ERR_STATE, "tilt_coupling active but a leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (tilt_gradients && (!fi.grad || !fo.grad))
    return fail(c, MS_ERR_STATE, "tilt_coupling: a leaflet has no tilt gradient buffer");
  if (int rc = exec_flush(c)) return rc;
  double* dp = static_cast<double*>(c->d_cpl);
  CoupleArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.t_in = trial_tilts ? fi.trial : fi.tilts;
  a.t_out = trial_tilts ? fo.trial : fo.tilts;
  if (!a.t_in || !a.t_out) return fail(c, MS_ERR_STATE, "tilt_coupling: a leaflet has no trial tilt buffer");
  a.k_c = c->cpl_k;
  a.sign = (double)c->cpl_sign;
  a.g = g_out;
  a.tg_in = tilt_gradients ? fi.grad : nullptr;
  a.tg_out = tilt_gradients ? fo.grad : nullptr;
  a.va = nullptr;
  a.partials = c->d_partials;
  a.slot = fo.s_etilt;
  a.cell_mode = kernel_cell_mode(cell);
  a.wg_sums = dp;
  // a relaxation in progress: x is frozen and the mode-3 set-up launch left the barycentric vertex areas (the same
  // doubles in either leaflet's array -- unless the outer leaflet carries an absence mask: its array then holds the kept
  // facets' areas, and the coupling is not masked (tilt_coupling.py:160-203 takes every facet), so the inner leaflet's
  // array is read; both fields are relaxed whenever this module is on)
  const double* va = fo.absent_bit ? fi.va : (fo.va ? fo.va : fi.va);
  const bool frozen = c->relax_va_valid && !use_dir && !gradient_into_g && va && !c->cpl_force_tile;
  ProfScope ps(c, 6);
  if (frozen) {
    a.va = va;
    HIPCHK(c, launch_couple_vec(a, tilt_gradients ? 1 : 0, c->stream));
    ++c->cpl_launches[2];
    return MS_OK;
  }
  const int mode = (gradient_into_g || tilt_gradients) ? 1 : 0;
  HIPCHK(c, launch_couple(a, mode, c->cap, c->til.max_ent, c->stream));
  ++c->cpl_launches[mode];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_tilt_coupling(ms_ctx* c, double modulus, int sign) {
  if (!c) return MS_ERR_INVALID;
  if (!std::isfinite(modulus)) return fail(c, MS_ERR_INVALID, "ms_set_tilt_coupling: the modulus must be finite");
  if (sign != -1 && sign != 0 && sign != 1)
    return fail(c, MS_ERR_INVALID, "ms_set_tilt_coupling: sign must be -1 (difference), +1 (sum) or 0 (off)");
  if (sign != 0 && c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_tilt_coupling: the tilt_coupling module is not sharded (single GPU only)");
  const int tiles = c->tile1 - c->tile0;
  if (sign != 0 && tiles <= 0) return fail(c, MS_ERR_STATE, "ms_set_tilt_coupling: the context has no tiles");
  if (sign != 0 && !c->d_cpl) {
    // the per-workgroup sums of the last launch
    const size_t bytes = sizeof(double) * (size_t)tiles;
    HIPCHK(c, hipMalloc(&c->d_cpl, bytes));
    HIPCHK(c, hipMemset(c->d_cpl, 0, bytes));
  }
  c->cpl_k = modulus;
  c->cpl_sign = sign;
  if (const char* e = getenv("MS_COUPLE_VEC")) c->cpl_force_tile = atoi(e) == 0;
  c->carry.invalidate();  // (the energies held are the old term's)
  return MS_OK;
}

int ms_get_tilt_coupling_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_tilt_coupling_energy: bad argument");
  *energy = 0.0;
  if (!c->d_cpl || c->cpl_sign == 0) return MS_OK;  // (0.0 when off, and until the first evaluation)
  // the workgroups' sums of the last launch, added in index order
  std::vector<double> sums((size_t)std::max(0, c->tile1 - c->tile0));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(sums.data(), c->d_cpl, sizeof(double) * sums.size(), hipMemcpyDeviceToHost));
  double tot = 0.0;
  for (double v : sums) tot += v;
  *energy = tot;
  return MS_OK;
}

int ms_tilt_coupling_stats(ms_ctx* c, double stats[3]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 3; ++k) stats[k] = (double)c->cpl_launches[k];
  return MS_OK;
}

}  // extern "C"
