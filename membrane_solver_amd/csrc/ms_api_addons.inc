// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): the one driver
// of the leaflet add-on passes (AddonCall, ms_api_phases.inc) over the slot-writer table (ms_slot_writers.h).
namespace {

int addon_passes(ms_ctx* c, uint32_t modules, const AddonCall& k) {
  if (!(modules & MS_LEAFLET_ADDONS)) return MS_OK;
  if (k.phase == Phase::GRADIENT && !k.g_out) return MS_OK;
  TiltField &fi = c->tf[1], &fo = c->tf[2];
  const bool rsm_inner = (fi.mod_addons & MS_MOD_RIM_SLOPE_MATCH_OUT) != 0;  // (a disk ring is loaded: ms_set_rim_match)
  const double* t_in = k.trial_tilts ? fi.trial : fi.tilts;
  const double* t_out = k.trial_tilts ? fo.trial : fo.tilts;
  const bool tg = k.tilt_gradients;
  double* tg_in = tg ? fi.grad : nullptr;
  for (int w = 0; w < kNumSlotWriters; ++w) {
    const SlotWriter& r = kSlotWriters[w];
    if (r.base || !launched(w, modules, rsm_inner, k.phase)) continue;
    const CellMode cell = cell_mode(w, r.slot, modules, rsm_inner, k.phase);
    int rc = MS_OK;
    switch (r.bit) {
      case MS_MOD_TILT_SPLAY_TWIST_IN: rc = splay_pass(c, k.use_dir, k.alpha, t_in, tg_in, cell); break;
      case MS_MOD_TILT_RIM_SOURCE_IN: rc = rim_pass(c, fi, k.use_dir, k.alpha, t_in, tg, cell); break;
      case MS_MOD_TILT_THETAB_CONTACT_IN: rc = thetab_pass(c, k.use_dir, k.alpha, t_in, tg_in, cell); break;
      case MS_MOD_TILT_RIM_SOURCE_OUT: rc = rim_pass(c, fo, k.use_dir, k.alpha, t_out, tg, cell); break;
      case MS_MOD_TILT_RIM_SOURCE_BILAYER: rc = rim_bilayer_pass(c, k.use_dir, k.alpha, k.trial_tilts, tg, cell); break;
      case MS_MOD_TILT_COUPLING: rc = couple_pass(c, k.use_dir, k.alpha, tg, k.trial_tilts, k.g_out, cell); break;
      case MS_MOD_RIM_SLOPE_MATCH_OUT:
        rc = rim_match_pass(c, k.use_dir, k.alpha, k.trial_tilts, tg, k.g_out, cell,
                            cell_mode(w, r.slot_disk, modules, rsm_inner, k.phase));
        break;
      default: return fail(c, MS_ERR_STATE, "addon_passes: a row of the slot-writer table has no pass");
    }
    if (rc) return rc;
  }
  return MS_OK;
}

}  // namespace
