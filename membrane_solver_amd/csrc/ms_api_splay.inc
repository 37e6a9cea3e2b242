// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit):
// tilt_splay_twist_in -- its setter and getters, and its pass (addon_passes runs it):
// k_splay<0> / k_splay<1> on x (+ alpha d).  Neither kernel is recorded by the one-tile interpreter: the pass flushes
// it first.  No host-side table: the kernels work from the tiling alone.
namespace {

int splay_pass(ms_ctx* c, bool use_dir, double alpha, const double* tilts, double* tilt_grad, CellMode cell) {
  ms_ctx::TiltField& f = c->tf[1];
  if (!c->st_set || !c->d_st)
    return fail(c, MS_ERR_STATE, "tilt_splay_twist_in active but ms_set_tilt_splay_twist was never called");
  if (!f.tilts || !tilts)
    return fail(c, MS_ERR_STATE, "tilt_splay_twist_in active but the inner leaflet's tilt field was never set (ms_set_leaflet_tilts)");
  if (int rc = exec_flush(c)) return rc;
  SplayArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.tilts = tilts;
  a.k_splay = c->st_k_splay;
  a.k_twist = c->st_k_twist;
  a.tilt_grad = tilt_grad;
  a.partials = c->d_partials;
  a.slot = f.s_ets;
  a.cell_mode = kernel_cell_mode(cell);
  a.wg_sums = static_cast<double*>(c->d_st);
  const int mode = tilt_grad ? 1 : 0;
  ProfScope ps(c, 11);
  HIPCHK(c, launch_splay(a, mode, c->cap, c->til.max_ent, c->stream));
  ++c->st_launches[mode];
  return MS_OK;
}

}  // namespace

extern "C" {

int ms_set_tilt_splay_twist(ms_ctx* c, double k_splay, double k_twist) {
  if (!c) return MS_ERR_INVALID;
  if (!std::isfinite(k_splay) || !std::isfinite(k_twist))
    return fail(c, MS_ERR_INVALID, "ms_set_tilt_splay_twist: the moduli must be finite");
  if (k_splay < 0.0 || k_twist < 0.0)
    return fail(c, MS_ERR_INVALID, "ms_set_tilt_splay_twist: the moduli must be non-negative");
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_set_tilt_splay_twist: the tilt_splay_twist_in module is not sharded (single GPU only)");
  const int tiles = c->tile1 - c->tile0;
  if (tiles <= 0) return fail(c, MS_ERR_STATE, "ms_set_tilt_splay_twist: the context has no tiles");
  if (!c->d_st) {
    // the per-workgroup sums of the last launch
    const size_t bytes = sizeof(double) * (size_t)tiles;
    HIPCHK(c, hipMalloc(&c->d_st, bytes));
    HIPCHK(c, hipMemset(c->d_st, 0, bytes));
  }
  c->st_k_splay = k_splay;
  c->st_k_twist = k_twist;
  c->st_set = true;
  c->carry.invalidate();  // (the energies held are the old term's)
  return MS_OK;
}

int ms_get_tilt_splay_twist_energy(ms_ctx* c, double* energy) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_get_tilt_splay_twist_energy: bad argument");
  *energy = 0.0;
  if (!c->d_st || !c->st_set) return MS_OK;  // (0.0 until the first evaluation)
  // the workgroups' sums of the last launch, added in index order
  std::vector<double> sums((size_t)std::max(0, c->tile1 - c->tile0));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipMemcpy(sums.data(), c->d_st, sizeof(double) * sums.size(), hipMemcpyDeviceToHost));
  double tot = 0.0;
  for (double v : sums) tot += v;
  *energy = tot;
  return MS_OK;
}

int ms_tilt_splay_twist_stats(ms_ctx* c, double stats[2]) {
  if (!c || !stats) return MS_ERR_INVALID;
  for (int k = 0; k < 2; ++k) stats[k] = (double)c->st_launches[k];
  return MS_OK;
}

}  // extern "C"
