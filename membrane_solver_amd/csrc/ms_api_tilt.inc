// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): tilt-module evaluation, the relaxations (host-driven, device program, fused), leaflet fields.
namespace {
// Energy of the tilt-reading modules (+ dense tilt gradients) on the current x, reading each
// field's `trial` or stored tilts (runtime/evaluation_manager.py:303-462 for the single field,
// :537-742 for the leaflets; needs d_bt_vert valid when bending_tilt is on).  With positions
// frozen the leaflet magnitude modules take the lumped vertex-area form whatever their mass mode
// (evaluation_manager.py:565-581, 663-695: the relaxation always passes tilt_vertex_areas).
int tilt_eval(ms_ctx* c, bool trial, bool gradient) {
  const uint32_t mods = c->params.modules;
  int rc = MS_OK;
  uint32_t mask = 0;
  const size_t b3 = sizeof(double) * 3 * (size_t)c->til.nvp;
  if (mods & MS_TILT_MODS) {
    const double* tilts = trial ? c->tf[0].trial : c->tf[0].tilts;
    // energy only, both modules of the field: the bending_tilt kernel sums the tilt-magnitude energy as well (it has
    // the tilt rows staged; a non-zero rigidity, or the slot would not be written)
    const bool fuse = !gradient && (mods & MS_MOD_TILT) && (mods & MS_MOD_BENDING_TILT) && c->tf[0].k_tilt != 0.0 &&
                      !c->tf[0].consistent;
    if ((mods & MS_MOD_TILT) && !fuse) {
      rc = tilt_pass(c, gradient ? 1 : 0, false, 0.0, tilts, nullptr, /*shape_gradient=*/false);
      if (rc) return rc;
      mask |= 1u << MS_S_ETILT;
    } else if (fuse) {
      mask |= 1u << MS_S_ETILT;
    } else if (gradient) {
      if (int rz = zero_doubles(c, c->tf[0].grad, b3)) return rz;
    }
    if (mods & MS_MOD_BENDING_TILT) {
      rc = bt_pass(c, gradient ? 2 : 0, false, 0.0, tilts, fuse);
      if (rc) return rc;
      mask |= 1u << MS_S_EBT;
    }
    if (mods & MS_MOD_TILT_SMOOTH) {
      rc = ts_pass(c, gradient ? 1 : 0, false, 0.0, tilts);
      if (rc) return rc;
      mask |= 1u << MS_S_ETS;
    }
  }
  for (int l = 1; l <= 2; ++l) {
    TiltField& f = c->tf[l];
    if (!(mods & f.mods())) continue;
    if (mods & f.etilt_mods()) mask |= 1u << f.s_etilt;  // (the slot's own module or an add-on riding there)
    if (mods & f.ets_mods()) mask |= 1u << f.s_ets;
    const double* tilts = trial ? f.trial : f.tilts;
    if ((mods & f.mod_tilt) && c->relax_va_valid && f.va) {
      // positions frozen, vertex areas at hand: the reference's own form of this evaluation, one streaming pass
      ProfScope ps(c, 6);
      HIPCHK(c, launch_tvec(4, c->tile0, c->tile1, c->til.nv, c->til.own, c->d_vflags, f.grad, f.va, f.dir, tilts,
                            nullptr, nullptr, nullptr, f.k_tilt, gradient ? 1 : 0, c->d_partials, c->til.n_tiles,
                            c->stream, f.fixed_bit, f.s_etilt, f.s_rz));
    } else if (mods & f.mod_tilt) {
      // (module form -- ms_leaflet_tilt_energy_and_gradient_ex: the field's own mass mode, tilt gradient included)
      rc = tilt_pass_f(c, f, gradient ? 1 : 0, false, 0.0, tilts, nullptr, /*shape_gradient=*/false,
                       /*lumped=*/!c->tilt_module_form);
      if (rc) return rc;
    } else if (gradient) {
      if (int rz = zero_doubles(c, f.grad, b3)) return rz;
    }
    if (mods & f.mod_bt) {
      rc = bt_pass_f(c, f, gradient ? 2 : 0, false, 0.0, tilts);
      if (rc) return rc;
      mask |= 1u << f.s_ebt;
    }
    if (mods & f.mod_dt) {
      rc = disk_target_pass(c, f, gradient ? 1 : 0, false, 0.0, tilts, false, gradient);
      if (rc) return rc;
      mask |= 1u << f.s_edt;
    }
    if (mods & f.mod_smooth) {
      rc = ts_pass_f(c, f, gradient ? 1 : 0, false, 0.0, tilts);
      if (rc) return rc;
    }
  }
  // the add-ons, behind both leaflets' blocks: the base passes have written the slots' cells and both fields' grad rows
  rc = addon_passes(c, mods, {Phase::TILT_EVAL, false, 0.0, trial, gradient, nullptr});
  if (rc) return rc;
  return mask ? reduce_slots(c, mask) : MS_OK;
}
double tilt_energy_from(const ms_ctx* c, const double* hs) {
  double e = 0.0;
  if (c->params.modules & MS_MOD_TILT) e += hs[MS_S_ETILT];
  if (c->params.modules & MS_MOD_BENDING_TILT) e += hs[MS_S_EBT];
  if (c->params.modules & MS_MOD_TILT_SMOOTH) e += hs[MS_S_ETS];
  for (int l = 1; l <= 2; ++l) {
    const TiltField& f = c->tf[l];
    if (c->params.modules & f.etilt_mods()) e += hs[f.s_etilt];  // (the slot's add-ons ride in it)
    if (c->params.modules & f.ets_mods()) e += hs[f.s_ets];
    if (c->params.modules & f.mod_bt) e += hs[f.s_ebt];
    if (c->params.modules & f.mod_dt) e += hs[f.s_edt];
  }
  return e;
}
double tilt_energy_from_mailbox(const ms_ctx* c) { return tilt_energy_from(c, c->h_scal); }

// The search pass of a relaxation (ms_tsearch.inc): can it evaluate this module set?  Fills the per-field part of its
// arguments and the mask of the slots it writes.
bool tsearch_plan(ms_ctx* c, TiltField** fl, int nf, bool along_dir, TsearchArgs* a, uint32_t* mask) {
  const uint32_t mods = c->params.modules;
  if (!c->tsearch_enable || nf < 1 || nf > 2 || !c->d_tn) return false;
  // the add-ons keep their own passes.  (Whichever fields are relaxed: the leaflets are relaxed as a pair -- every field
  // an active module reads, leaflet_ready -- so a field the add-on reads is always among them, and ms_relax_tilts
  // refuses leaflet modules next to the single field)
  if (mods & MS_LEAFLET_ADDONS) return false;
  for (int k = 0; k < nf; ++k)
    if (fl[k]->absent_bit) return false;  // an absence mask: the launch-per-module passes honour it, k_tsearch / k_tgrad do not
  *mask = 0;
  for (int k = 0; k < nf; ++k) {
    TiltField& f = *fl[k];
    TsearchField& o = a->f[k];
    const bool single = &f == &c->tf[0];
    const bool tilt_on = single ? (mods & MS_MOD_TILT) != 0 : (mods & f.mod_tilt) != 0;
    const bool bt_on = single ? (mods & MS_MOD_BENDING_TILT) != 0 : (mods & f.mod_bt) != 0;
    const bool ts_on = single ? (mods & MS_MOD_TILT_SMOOTH) != 0 : (mods & f.mod_smooth) != 0;
    if (!single && (mods & f.mod_dt)) return false;  // (so does the disk target)
    o.tilts = f.tilts;
    o.src = along_dir ? f.dir : f.grad;
    o.bt_vert = nullptr;
    o.kappa = nullptr;
    o.va = nullptr;
    o.div_sign = f.div_sign;
    o.k_tilt = f.k_tilt;
    o.k_smooth = f.k_smooth;
    o.tilt_form = 0;
    o.s_ebt = o.s_ets = -1;
    o.s_etilt = f.s_etilt;
    o.fixed_bit = f.fixed_bit;
    o.trial_out = nullptr;
    if (tilt_on) {
      if (single) {
        // the per-facet form rides with bending_tilt's term (tilt_eval: `fuse`); alone, or with the consistent mass,
        // k_tilt keeps it
        if (!(bt_on && f.k_tilt != 0.0 && !f.consistent)) return false;
        o.tilt_form = 1;
      } else {
        if (!(c->relax_va_valid && f.va)) return false;
        o.tilt_form = 2;
        o.va = f.va;
      }
      *mask |= 1u << f.s_etilt;
    }
    if (bt_on) {
      o.bt_vert = single ? c->d_bt_vert : f.bt_vert;
      o.kappa = single ? device_mesh(c).kappa : f.kappa;
      if (!o.bt_vert || !o.kappa) return false;
      o.s_ebt = f.s_ebt;
      *mask |= 1u << f.s_ebt;
    }
    if (ts_on) {
      o.s_ets = f.s_ets;
      *mask |= 1u << f.s_ets;
    }
    if (!o.tilts || !o.src) return false;
  }
  if (*mask == 0) return false;
  a->m = device_mesh(c);
  a->tile0 = c->tile0;
  a->tile1 = c->tile1;
  a->x = c->buf[MS_BUF_X];
  a->normals = c->d_tn;
  a->d = nullptr;
  a->alpha = 0.0;
  a->plain = 0;
  a->n_fields = nf;
  if (nf == 1) a->f[1] = a->f[0];
  return tsearch_fits(c->cap, nf, MS_MAX_TRIALS);
}

// The gradient pass of a relaxation (ms_tsearch.inc: k_tgrad) covers what the search pass covers
bool tgrad_plan(ms_ctx* c, TiltField** fl, int nf, TgradArgs* a, uint32_t* mask) {
  TsearchArgs sa;
  for (int k = 0; k < nf; ++k)
    if (!fl[k]->grad || !fl[k]->minv) return false;
  if (!tsearch_plan(c, fl, nf, /*along_dir=*/false, &sa, mask)) return false;
  for (int k = 0; k < nf; ++k) {
    const TiltField& f = *fl[k];
    const TsearchField& o = sa.f[k];
    TgradField& g = a->f[k];
    g.tilts = o.tilts;
    g.bt_vert = o.bt_vert;
    g.kappa = o.kappa;
    g.va = o.va;
    g.minv = f.minv;
    g.grad = f.grad;
    g.div_sign = o.div_sign;
    g.k_tilt = o.k_tilt;
    g.k_smooth = o.k_smooth;
    g.tilt_form = o.tilt_form;
    g.s_ebt = o.s_ebt;
    g.s_etilt = o.s_etilt;
    g.s_ets = o.s_ets;
    g.s_gn2 = f.s_gn2;
    g.s_rz = f.s_rz;
    g.fixed_bit = o.fixed_bit;
    *mask |= (1u << f.s_gn2) | (1u << f.s_rz);
  }
  if (nf == 1) a->f[1] = a->f[0];
  a->m = sa.m;
  a->tile0 = sa.tile0;
  a->tile1 = sa.tile1;
  a->x = sa.x;
  a->n_fields = nf;
  a->partials = c->d_partials;
  return tgrad_fits(c->til.T, c->cap, c->til.max_ent, nf);
}

// n step sizes of one ladder in one pass + one fold, queued; `second`: a pass queued BEHIND one whose results have not
// been taken yet -- its folds post to mailboxes of their own (the side sets' other parity, tsearch_mb for the last trial)
int tsearch_queue(ms_ctx* c, TsearchArgs& a, uint32_t mask, const double* coefs, int n, bool second) {
  int rc = ensure_side_sets(c, n - 1);
  if (rc) return rc;
  if (second) {
    rc = make_mailbox(c, c->tsearch_mb);
    if (rc) return rc;
  }
  a.n_trials = n;
  for (int j = 0; j < MS_MAX_TRIALS; ++j) {
    a.coef[j] = coefs[std::min(j, n - 1)];
    a.partials[j] = j < n - 1 ? c->side[j].partials : (j == n - 1 ? c->d_partials : nullptr);
  }
  {
    ProfScope ps(c, 12);
    HIPCHK(c, launch_tsearch(a, c->cap, c->stream));
  }
  ++c->tsearch_launches;
  c->tsearch_trials += n;
  StageCtl st = c->stage();  // (whatever else the caller's stage says holds for this fold as well)
  st.cur_parity = second ? 1 : 0;
  st.pair_on = n > 1 ? n : 0;
  st.multi_any_slot = true;
  StageScope scope(c, st);
  if (second) swap_mailbox(c, c->tsearch_mb);
  rc = reduce_slots(c, mask);
  if (second) swap_mailbox(c, c->tsearch_mb);
  return rc;
}
// ... and taken: E[j] = the energy the reference's loop would see at trial j
int tsearch_take(ms_ctx* c, int n, bool second, double* E) {
  double v[MS_NSCAL];
  const int p = second ? 1 : 0;
  for (int j = 0; j + 1 < n; ++j) {
    int rc = wait_mailbox(c, c->side[j].mb[p].h_seq, c->side[j].mb[p].expected, v, nullptr);
    if (rc) return rc;
    E[j] = tilt_energy_from(c, v);
  }
  if (second) swap_mailbox(c, c->tsearch_mb);
  int rc = fetch(c);
  if (rc == MS_OK) E[n - 1] = tilt_energy_from_mailbox(c);
  if (second) swap_mailbox(c, c->tsearch_mb);
  return rc;
}
int ensure_bt_record(ms_ctx* c) {
  if (!(c->params.modules & (MS_MOD_BENDING_TILT | MS_LEAFLET_BT)) || c->carry.bt_valid) return MS_OK;
  return phase_energy(c, c->params.modules, false, 0.0, false, false, false, /*reduce_now=*/false);
}

// The relaxation loop of relax_fields as a device program: the command lists the loop launches over and over are
// CAPTURED once (both parities of the tilts <-> trial swap), the control flow runs in the interpreter's workgroup
// (ms_exec.inc: exec_relax).  *used = false: not possible here (the caller runs the host-driven loop).
int relax_program(ms_ctx* c, const ms_tilt_relax_params* rp, TiltField** fl, int nf, uint32_t norm_mask, int* iters,
                  int* evals, bool* used) {
  *used = false;
  if (nf < 1 || nf > 2) return MS_OK;
  const Tiling& t = c->til;
  if (!c->d_relax_cells) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_relax_cells), sizeof(double) * 2));
    HIPCHK(c, hipMemset(c->d_relax_cells, 0, sizeof(double) * 2));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_relax_box), sizeof(unsigned long long) * 8, hipHostMallocMapped));
    memset(c->h_relax_box, 0, sizeof(unsigned long long) * 8);
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_h_relax_box), c->h_relax_box, 0));
  }
  int rc = exec_flush(c);  // (the set-up passes recorded so far run first, as a pack of their own)
  if (rc) return rc;
  ExecRecorder& R = c->exec;
  auto wait_result = [&](unsigned long long ticket, unsigned long long v[4]) -> int {
    auto entry = [&](int k, unsigned long long* val) {
      const unsigned long long tag = __atomic_load_n(&c->h_relax_box[2 * k + 1], __ATOMIC_ACQUIRE);
      *val = __atomic_load_n(&c->h_relax_box[2 * k], __ATOMIC_ACQUIRE);
      return (*val ^ tag) == ticket;
    };
    bool done = false;
    for (long spin = 0; !done && spin < 400000000L; ++spin) {
      done = entry(3, &v[3]) && entry(0, &v[0]) && entry(1, &v[1]) && entry(2, &v[2]);
      if (!done) __builtin_ia32_pause();
    }
    if (!done) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      done = entry(3, &v[3]) && entry(0, &v[0]) && entry(1, &v[1]) && entry(2, &v[2]);
      if (!done) return fail(c, MS_ERR_STATE, "relaxation program: the result mailbox was not posted");
    }
    return MS_OK;
  };
  // ---- leaflet fields, frozen surface, LDS-atomic contexts: the fused evaluator (ms_relax_fused.inc) ----------------
  bool absent = false;  // an absence mask: the fused evaluator does not honour it, the captured program's bodies do
  for (int k = 0; k < nf; ++k) absent = absent || fl[k]->absent_bit != 0;
  if (!absent && c->exec_fused && c->relax_va_valid && !c->deterministic && c->d_tn) {
    const uint32_t mods = c->params.modules;
    ExecRelaxFusedArgs a;
    memset(&a, 0, sizeof(a));
    a.m = device_mesh(c);
    a.x = c->buf[MS_BUF_X];
    a.normals = c->d_tn;
    a.nf = nf;
    a.solver = rp->solver;
    a.max_iters = rp->max_iters;
    a.cap = c->cap;
    a.max_ent = t.max_ent;
    a.step_size = rp->step_size;
    a.tol = rp->tol;
    a.host_box = c->d_h_relax_box;
    a.ticket = ++c->relax_ticket;
    bool ok = true;
    for (int k = 0; k < nf; ++k) {
      TiltField& f = *fl[k];
      ExecRelaxFusedField& q = a.f[k];
      q.tilts = f.tilts;
      q.minv = f.minv;
      q.va = f.va;
      q.bt_vert = f.bt_vert;
      q.kappa = f.kappa;
      q.dt_target = f.dt_target;
      q.disk = f.disk;
      q.k_tilt = f.k_tilt;
      q.k_smooth = f.k_smooth;
      q.dt_strength = f.dt.strength;
      q.div_sign = f.div_sign;
      q.has_tilt = (mods & f.mod_tilt) ? 1 : 0;
      q.has_bt = (mods & f.mod_bt) ? 1 : 0;
      q.has_ts = (mods & f.mod_smooth) ? 1 : 0;
      q.has_dt = (mods & f.mod_dt) ? 1 : 0;
      q.fixed_bit = f.fixed_bit;
      // (no add-on is on here: relax_fields keeps this program for module sets without one)
      ok = ok && f.minv && (!q.has_tilt || f.va) && (!q.has_bt || (f.bt_vert && f.kappa)) &&
           (!q.has_dt || (f.dt_target && f.disk && f.dt_target_valid));
    }
    const size_t need = relax_fused_lds_bytes(c->cap, t.max_ent, t.max_tile_facets);
    if (ok && need <= MS_LDS_TILT_PASS) {
      const hipError_t he = R.push(CK_RELAX_FUSED, 0, c->cap, t.max_ent, 1, 0, need, &a, sizeof(a), &a.m);
      if (he != hipSuccess) return fail_hip(c, he, "k_exec (fused relaxation)");
      rc = exec_flush(c);
      if (rc) return rc;
      unsigned long long v[4] = {0, 0, 0, 0};
      rc = wait_result(a.ticket, v);
      if (rc) return rc;
      *iters = (int)v[0];
      *evals = (int)v[1];
      ++c->relax_fused_runs;
      ++c->relax_programs;
      *used = true;
      return MS_OK;
    }
  }
  const bool along_dir = rp->solver != 0;
  ExecRelaxHead head;
  memset(&head, 0, sizeof(head));
  // -- capture -------------------------------------------------------------------------------------------------
  const unsigned long long s_ticket = c->ticket;
  unsigned long long s_expected[MS_MB_WORDS];
  memcpy(s_expected, c->expected, sizeof(s_expected));
  const long s_cmds = R.cmds;
  R.capture = true;
  auto count = [&]() { return (int)reinterpret_cast<const ExecPackHead*>(R.buf.data())->n_cmds; };
  auto fail_capture = [&](int code) {
    R.capture = false;
    R.buf.clear();
    R.cmds = s_cmds;
    c->ticket = s_ticket;
    memcpy(c->expected, s_expected, sizeof(s_expected));
    return code;
  };
  hipError_t he = R.push(CK_RELAX, 0, 0, 0, 1, 0, 0, &head, sizeof(head));
  if (he != hipSuccess) return fail_capture(MS_OK);
  const size_t head_at = sizeof(ExecPackHead);
  auto tvec = [&](TiltField& f, int mode, const double* src, double* out, int flag) -> hipError_t {
    return launch_tvec(mode, c->tile0, c->tile1, t.nv, t.own, c->d_vflags, f.grad, f.minv, f.dir, f.tilts, src, c->d_tn,
                       out, 0.0, flag, c->d_partials, t.n_tiles, c->stream, f.fixed_bit, f.s_gn2, f.s_rz);
  };
  bool ok = true;
  for (int par = 0; par < 2 && ok; ++par) {
    head.off_grad[par] = (int32_t)R.buf.size();
    int n0 = count();
    ok = ok && tilt_eval(c, false, true) == MS_OK;
    for (int k = 0; k < nf && ok; ++k) ok = tvec(*fl[k], 0, nullptr, nullptr, 0) == hipSuccess;
    ok = ok && reduce_slots(c, norm_mask) == MS_OK;
    head.n_grad[par] = count() - n0;
    head.off_trial[par] = (int32_t)R.buf.size();
    n0 = count();
    for (int k = 0; k < nf && ok; ++k) {
      TiltField& f = *fl[k];
      ok = tvec(f, 2, along_dir ? f.dir : f.grad, f.trial, 1) == hipSuccess;
    }
    ok = ok && tilt_eval(c, true, false) == MS_OK;
    head.n_trial[par] = count() - n0;
    for (int k = 0; k < nf; ++k) std::swap(fl[k]->tilts, fl[k]->trial);  // (twice in all: back where they were)
  }
  head.off_dir0 = (int32_t)R.buf.size();
  {
    const int n0 = count();
    for (int k = 0; k < nf && ok; ++k) ok = tvec(*fl[k], 1, nullptr, nullptr, 1) == hipSuccess;
    head.n_dir0 = count() - n0;
  }
  head.off_dir1 = (int32_t)R.buf.size();
  {
    const int n0 = count();
    for (int k = 0; k < nf && ok; ++k) ok = tvec(*fl[k], 1, nullptr, nullptr, 0) == hipSuccess;
    head.n_dir1 = count() - n0;
  }
  if (!ok) return fail_capture(MS_OK);  // (e.g. the program does not fit the largest pack: host-driven loop)
  std::vector<unsigned char> prog;
  prog.swap(R.buf);
  const size_t prog_lds = R.lds;
  R.capture = false;
  R.cmds = s_cmds;
  c->ticket = s_ticket;
  memcpy(c->expected, s_expected, sizeof(s_expected));
  // -- patch: the trial / direction passes take their coefficient from the program's cells, the folds post nothing
  {
    size_t at = head_at + sizeof(ExecCmdHead) + sizeof(ExecRelaxHead);
    while (at + sizeof(ExecCmdHead) <= prog.size()) {
      ExecCmdHead h;
      memcpy(&h, prog.data() + at, sizeof(h));
      unsigned char* args = prog.data() + at + sizeof(ExecCmdHead);
      if (h.kind == CK_TVEC) {
        TvecArgs a;
        memcpy(&a, args, sizeof(a));
        if (a.mode == 2) a.coef_dev = c->d_relax_cells;
        if (a.mode == 1 && (int32_t)at >= head.off_dir1) a.coef_dev = c->d_relax_cells + 1;
        memcpy(args, &a, sizeof(a));
      } else if (h.kind == CK_REDUCE) {
        FoldArgs a;
        memcpy(&a, args, sizeof(a));
        for (int j = 0; j < MS_MAX_TRIALS; ++j) a.set[j].host_box = nullptr;
        memcpy(args, &a, sizeof(a));
      }
      at += h.bytes;
    }
  }
  // -- the head ---------------------------------------------------------------------------------------------------
  head.solver = rp->solver;
  head.max_iters = rp->max_iters;
  head.nf = nf;
  head.step_size = rp->step_size;
  head.tol = rp->tol;
  {
    const uint32_t mods = c->params.modules;  // (the order of tilt_energy_from_mailbox)
    int n = 0;
    if (mods & MS_MOD_TILT) head.e_slot[n++] = MS_S_ETILT;
    if (mods & MS_MOD_BENDING_TILT) head.e_slot[n++] = MS_S_EBT;
    if (mods & MS_MOD_TILT_SMOOTH) head.e_slot[n++] = MS_S_ETS;
    for (int l = 1; l <= 2; ++l) {
      const TiltField& f = c->tf[l];
      if (mods & f.etilt_mods()) head.e_slot[n++] = f.s_etilt;
      if (mods & f.ets_mods()) head.e_slot[n++] = f.s_ets;
      if (mods & f.mod_bt) head.e_slot[n++] = f.s_ebt;
      if (mods & f.mod_dt) head.e_slot[n++] = f.s_edt;
    }
    head.n_e = n;
  }
  for (int k = 0; k < nf; ++k) {
    head.s_gn2[k] = fl[k]->s_gn2;
    head.s_rz[k] = fl[k]->s_rz;
  }
  head.scal = c->d_scal;
  head.cells = c->d_relax_cells;
  head.host_box = c->d_h_relax_box;
  head.ticket = ++c->relax_ticket;
  head.total_bytes = (int32_t)(prog.size() - head_at);
  {
    ExecCmdHead h;
    memcpy(&h, prog.data() + head_at, sizeof(h));
    h.pad = head.total_bytes;
    memcpy(prog.data() + head_at, &h, sizeof(h));
    memcpy(prog.data() + head_at + sizeof(h), &head, sizeof(head));
    reinterpret_cast<ExecPackHead*>(prog.data())->n_cmds = 1;  // (the lists belong to the CK_RELAX record)
  }
  he = R.launch_pack(prog, prog_lds);
  if (he != hipSuccess) return fail_hip(c, he, "k_exec (relaxation program)");
  ++c->relax_programs;
  // -- result ------------------------------------------------------------------------------------------------------
  unsigned long long v[4] = {0, 0, 0, 0};
  rc = wait_result(head.ticket, v);
  if (rc) return rc;
  *iters = (int)v[0];
  *evals = (int)v[1];
  if (v[2] & 1ull)
    for (int k = 0; k < nf; ++k) std::swap(fl[k]->tilts, fl[k]->trial);
  *used = true;
  return MS_OK;
}

// TiltRelaxationManager.relax_tilts (tilt_relaxation.py:237-424) for one field and
// relax_leaflet_tilts (:426-1478, default options) for the (in, out) pair: the same driver over
// the concatenated free rows of `fl[0..nf)` -- one energy, |grad|^2 and <r, M^-1 r> summed over
// the fields, one step length for all of them.
int relax_fields(ms_ctx* c, const ms_tilt_relax_params* rp, TiltField** fl, int nf, bool jacobi_smooth_by_param,
                 int* iters_out, int* evals_out) {
  const uint32_t mods = c->params.modules;
  const Tiling& t = c->til;
  bool any_free = false;
  for (int k = 0; k < nf; ++k) any_free = any_free || fl[k]->any_free;
  if (!any_free) return MS_OK;
  const size_t b3 = sizeof(double) * 3 * (size_t)t.nvp;
  if (!c->d_tn) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_tn), b3));
    HIPCHK(c, hipMemset(c->d_tn, 0, b3));
  }
  for (int k = 0; k < nf; ++k) {
    TiltField& f = *fl[k];
    if (f.dir) continue;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.dir), b3));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.minv), sizeof(double) * (size_t)t.nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.va), sizeof(double) * (size_t)t.nvp));
    HIPCHK(c, hipMemset(f.dir, 0, b3));
    HIPCHK(c, hipMemset(f.minv, 0, sizeof(double) * (size_t)t.nvp));
    HIPCHK(c, hipMemset(f.va, 0, sizeof(double) * (size_t)t.nvp));
  }
  int iters = 0, evals = 0;
  int rc = ensure_bt_record(c);
  if (rc) return rc;
  // tilt_thetaB_boundary_in: the constraint acts on the inner leaflet's field (the single-field driver never sees it).
  // x is frozen: the directions are formed once, here; the stored tilts are enforced before the set-up launch projects
  // them (tilt_relaxation.py:612-616)
  bool tbb_on = false;
  for (int k = 0; k < nf; ++k) tbb_on = tbb_on || (fl[k] == &c->tf[1] && tbb_active(c));
  c->tbb_geom_valid = false;
  // enforce (+ P on the ring rows: every other row of both fields is a projected row already)
  auto tbb_enforce = [&](bool project) -> int {
    if (!tbb_on) return MS_OK;
    int r = tbb_geom_run(c, nullptr, false, 0.0, /*frozen=*/true);
    if (r) return r;
    return tbb_apply_run(c, 0, c->tf[1].tilts, nullptr, project);
  };
  rc = tbb_enforce(false);
  if (rc) return rc;
  auto tvec = [&](TiltField& f, int mode, const double* src, double* out, double coef, int flag) -> int {
    ProfScope ps(c, 6);
    HIPCHK(c, launch_tvec(mode, c->tile0, c->tile1, t.nv, t.own, c->d_vflags, f.grad, f.minv, f.dir, f.tilts, src,
                          c->d_tn, out, coef, flag, c->d_partials, t.n_tiles, c->stream, f.fixed_bit, f.s_gn2,
                          f.s_rz));
    return MS_OK;
  };
  // the same op on every field of the relaxation: one launch for the two leaflets (multi-tile contexts; the
  // interpreter records per field)
  auto tvec_all = [&](int mode, bool from_dir, double coef, int flag) -> int {
    if (nf == 2 && !c->exec_on && c->tsearch_enable) {
      TvecArgs a[2];
      for (int k = 0; k < 2; ++k) {
        TiltField& f = *fl[k];
        a[k].mode = mode; a[k].tile0 = c->tile0; a[k].nv = t.nv; a[k].T = t.own; a[k].vflags = c->d_vflags;
        a[k].tg = f.grad; a[k].minv = f.minv; a[k].dir = f.dir; a[k].tilts = f.tilts;
        a[k].src = mode == 2 ? (from_dir ? f.dir : f.grad) : nullptr;
        a[k].normals = c->d_tn; a[k].out = mode == 2 ? f.trial : nullptr; a[k].coef = coef; a[k].coef_dev = nullptr;
        a[k].flag = flag; a[k].partials = c->d_partials; a[k].n_tiles = t.n_tiles; a[k].fixed_bit = f.fixed_bit;
        a[k].s_gn2 = f.s_gn2; a[k].s_rz = f.s_rz;
      }
      ProfScope ps(c, 6);
      HIPCHK(c, launch_tvec2(a[0], a[1], c->tile1 - c->tile0, c->stream));
      return MS_OK;
    }
    for (int k = 0; k < nf; ++k) {
      TiltField& f = *fl[k];
      int r = tvec(f, mode, mode == 2 ? (from_dir ? f.dir : f.grad) : nullptr, mode == 2 ? f.trial : nullptr, coef, flag);
      if (r) return r;
    }
    return MS_OK;
  };
  uint32_t norm_mask = 0;
  for (int k = 0; k < nf; ++k) {
    TiltField& f = *fl[k];
    norm_mask |= (1u << f.s_gn2) | (1u << f.s_rz);
    {  // frozen geometry: unit vertex normals and the tilt-rigidity part of the Jacobi diagonal
      TiltArgs a;
      a.fields = nullptr;
      a.fields_rows = 0;
      a.m = device_mesh(c);
      a.tile0 = c->tile0;
      a.tile1 = c->tile1;
      a.x = c->buf[MS_BUF_X];
      a.d = nullptr;
      a.alpha = 0.0;
      a.tilts = f.tilts;
      a.tilts_out = c->d_tn;
      a.k_tilt = (rp->solver == 1 && rp->jacobi) ? f.k_tilt : 0.0;
      a.g = nullptr;
      a.tilt_grad = f.grad;
      a.minv = f.minv;
      a.partials = c->d_partials;
      a.e_slot = f.s_etilt;
      a.consistent = 0;
      a.tg_accumulate = 0;
      a.cons_tilt_grad = 0;
      a.va_out = f.va;
      // + 1/2 k_s sum (c_a + c_b): the parameter alone decides, loaded module or not
      // (preconditioners.py:42-57 single field, :111-139 leaflets)
      const double ks = jacobi_smooth_by_param ? f.k_smooth_precond : f.k_smooth;
      const bool smooth_diag = rp->solver == 1 && rp->jacobi && ks != 0.0;
      // the same launch finishes the set-up: tilts <- P(tilts) on every row (:303-305 / :640-663; fixed rows keep that
      // value from now on), and the diagonal -> clamped inverse when nothing is added to it first
      a.proj_out = f.trial;
      a.finish_minv = smooth_diag ? 0 : 1;
      a.fixed_bit = f.fixed_bit;
      a.absent_bit = f.absent_bit;
      if (nf == 2 && k == 0) {  // both fields of the relaxation in this one launch (same normals, same vertex areas)
        TiltField& fb = *fl[1];
        const double ksb = jacobi_smooth_by_param ? fb.k_smooth_precond : fb.k_smooth;
        a.tilts_b = fb.tilts;
        a.proj_out_b = fb.trial;
        a.minv_b = fb.minv;
        a.va_out_b = fb.va;
        a.k_tilt_b = (rp->solver == 1 && rp->jacobi) ? fb.k_tilt : 0.0;
        a.finish_minv_b = (rp->solver == 1 && rp->jacobi && ksb != 0.0) ? 0 : 1;
        a.fixed_bit_b = fb.fixed_bit;
        a.absent_bit_b = fb.absent_bit;
      }
      if (!(nf == 2 && k == 1)) HIPCHK(c, launch_tilt(a, 3, c->cap, t.max_ent, c->stream));
      if (smooth_diag) {
        rc = ts_pass_f(c, f, 2, false, 0.0, f.tilts, f.minv, ks);
        if (rc) return rc;
        rc = tvec(f, 3, nullptr, f.minv, 0.0, 0);  // diagonal -> clamped inverse
        if (rc) return rc;
      }
    }
    std::swap(f.tilts, f.trial);
  }
  struct VaScope {  // the cached vertex areas / disk-target profiles are valid only while this relaxation runs (x frozen)
    ms_ctx* c;
    ~VaScope() {
      c->relax_va_valid = false;
      for (int l = 0; l < 3; ++l) c->tf[l].dt_target_valid = c->tf[l].rs_coef_valid = false;
      c->rb_coef_valid = false;
      c->tb_relax = c->tb_geom_valid = c->rsm_geom_valid = false;
      c->tbb_geom_valid = false;
    }
  } va_scope{c};
  c->relax_va_valid = jacobi_smooth_by_param;  // leaflet driver only (the single field has no such form)
  // tilt_thetaB_contact_in: x is frozen from here on whatever the preconditioner -- the ring is ordered by the first
  // evaluation of this relaxation and the others only apply its table
  c->tb_relax = true;
  c->tb_geom_valid = c->rsm_geom_valid = false;
  for (int k = 0; k < nf && c->relax_va_valid; ++k) {
    // prime the frozen-surface caches of the disk target (radius, theta(r) r_hat) before the loop: every evaluation of
    // the relaxation -- and the device program's captured lists -- then only take differences
    TiltField& f = *fl[k];
    f.dt_target_valid = false;
    f.rs_coef_valid = false;  // (the first rim pass of this relaxation computes the coefficients, the others reuse them)
    c->rb_coef_valid = false;
    if (!(mods & f.mod_dt)) continue;
    rc = disk_target_pass(c, f, 0, false, 0.0, f.tilts, false, false);
    if (rc) return rc;
  }
  auto grad_at = [&](double* E, double* gnorm, double* rz) -> int {
    int r = MS_OK;
    TgradArgs ga;
    uint32_t gmask = 0;
    if (!tbb_on && tgrad_plan(c, fl, nf, &ga, &gmask)) {  // (the constraint's projection sits between the gradient and its norms)
      // every module of every field, the clamped rows and the norms in ONE pass and one fold
      {
        ProfScope ps(c, 12);
        HIPCHK(c, launch_tgrad(ga, c->cap, t.max_ent, /*combine=*/!c->deterministic, c->stream));
      }
      ++c->tsearch_launches;
      r = reduce_slots(c, gmask);
    } else {
      r = tilt_eval(c, false, true);
      if (r) return r;
      if (tbb_on) {  // tilt_relaxation.py:826-853: the projection, then the fixed rows' zeroing and the norms below
        r = tbb_apply_run(c, 2, c->tf[1].grad, nullptr, false);
        if (r) return r;
      }
      for (int k = 0; k < nf; ++k) {
        r = tvec(*fl[k], 0, nullptr, nullptr, 0.0, 0);
        if (r) return r;
      }
      r = reduce_slots(c, norm_mask);
    }
    if (r) return r;
    r = fetch(c);
    if (r) return r;
    ++evals;
    *E = tilt_energy_from_mailbox(c);
    double g2 = 0.0, z = 0.0;
    for (int k = 0; k < nf; ++k) {
      g2 += c->h_scal[fl[k]->s_gn2];
      z += c->h_scal[fl[k]->s_rz];
    }
    *gnorm = std::sqrt(g2);
    *rz = z;
    return MS_OK;
  };
  // backtracking on E(P(t + step*src)) <= E0 (:330-347 / :380-398 / :918-973); accepts by pointer swap
  auto search = [&](bool along_dir, double sign, double E0, double* E_acc, bool* accepted) -> int {
    double step = rp->step_size;
    *accepted = false;
    for (int bt = 0; bt < 12; ++bt) {
      for (int k = 0; k < nf; ++k) {
        TiltField& f = *fl[k];
        int r = tvec(f, 2, along_dir ? f.dir : f.grad, f.trial, sign * step, 1);
        if (r) return r;
      }
      int r = tilt_eval(c, true, false);
      if (r) return r;
      r = fetch(c);
      if (r) return r;
      ++evals;
      const double E1 = tilt_energy_from_mailbox(c);
      if (E1 <= E0) {
        for (int k = 0; k < nf; ++k) std::swap(fl[k]->tilts, fl[k]->trial);
        *E_acc = E1;
        *accepted = true;
        return MS_OK;
      }
      step *= 0.5;
      if (step < 1e-16) break;
    }
    return MS_OK;
  };
  // the same search as multi-trial passes: the ladder's step sizes are evaluated several at a time, the first one that
  // passes is the one the loop above would have stopped at (`evals` counts what that loop would have evaluated)
  auto search_multi = [&](bool along_dir, double sign, double E0, double* E_acc, bool* accepted, bool* used) -> int {
    TsearchArgs ta;
    uint32_t mask = 0;
    *used = tsearch_plan(c, fl, nf, along_dir, &ta, &mask);
    if (!*used) return MS_OK;
    *accepted = false;
    double steps[12];
    int n_lad = 0;
    for (double st = rp->step_size; n_lad < 12;) {
      steps[n_lad++] = st;
      st *= 0.5;
      if (st < 1e-16) break;
    }
    int b = 0;
    // the last search rejected every step size: this one's two passes are queued back to back (the second one's
    // results are only looked at if the first one accepts nothing)
    const bool both = c->tsearch_all_failed && !c->tsearch_first_single && n_lad > MS_MAX_TRIALS;
    bool second_queued = false;
    double coefs2[MS_MAX_TRIALS];
    while (b < n_lad) {
      const int n = (b == 0 && c->tsearch_first_single) ? 1 : std::min(MS_MAX_TRIALS, n_lad - b);
      double coefs[MS_MAX_TRIALS], E[MS_MAX_TRIALS];
      for (int j = 0; j < n; ++j) coefs[j] = sign * steps[b + j];
      for (int k = 0; k < nf; ++k) ta.f[k].trial_out = n == 1 ? fl[k]->trial : nullptr;  // (one step size: its rows are kept)
      int r = MS_OK;
      const bool is_second = second_queued;
      if (!is_second) {
        r = tsearch_queue(c, ta, mask, coefs, n, false);
        if (r) return r;
        if (both && b == 0) {
          const int n2 = n_lad - n;
          for (int j = 0; j < n2; ++j) coefs2[j] = sign * steps[n + j];
          r = tsearch_queue(c, ta, mask, coefs2, n2, true);
          if (r) return r;
          second_queued = true;
        }
      }
      r = tsearch_take(c, n, is_second, E);
      if (r) return r;
      for (int j = 0; j < n; ++j) {
        ++evals;
        if (!(E[j] <= E0)) continue;
        if (n > 1) {  // the accepted trial field, written once
          r = tvec_all(2, along_dir, coefs[j], 1);
          if (r) return r;
        }
        for (int k = 0; k < nf; ++k) std::swap(fl[k]->tilts, fl[k]->trial);
        *E_acc = E[j];
        *accepted = true;
        c->tsearch_first_single = (b + j) == 0;
        c->tsearch_all_failed = false;
        return MS_OK;
      }
      b += n;
    }
    c->tsearch_first_single = false;
    c->tsearch_all_failed = true;
    return MS_OK;
  };
  auto search_any = [&](bool along_dir, double sign, double E0, double* E_acc, bool* accepted) -> int {
    bool used = false;
    int r = search_multi(along_dir, sign, E0, E_acc, accepted, &used);
    if (r || used) return r;
    return search(along_dir, sign, E0, E_acc, accepted);
  };
  // (the add-ons' kernels are not recorded)
  if (!tbb_on && c->exec_on && c->exec_relax && !(mods & MS_LEAFLET_ADDONS)) {
    // one-tile context: the whole solve below as ONE launch (ms_internal.h: ExecRelaxHead)
    bool used = false;
    rc = relax_program(c, rp, fl, nf, norm_mask, &iters, &evals, &used);
    if (rc) return rc;
    if (used) {
      if (iters_out) *iters_out = iters;
      if (evals_out) *evals_out = evals;
      c->carry.carry_valid = c->carry.grad_valid = false;
      c->carry.factors_valid = c->carry.factors_valid && !(mods & (MS_MOD_BENDING_TILT | MS_LEAFLET_BT));
      return MS_OK;
    }
  }
  const double tol = rp->tol > 0.0 ? rp->tol : 0.0;
  double E0 = 0.0, gnorm = 0.0, rz_old = 0.0;
  // behind an accepted step (:1048-1052 / :1372-1378): the constraint enforced on the accepted field, then P
  int accepted = 0;
  auto tbb_after_accept = [&]() -> int {
    ++accepted;
    if (c->tilt_proj_cadence != MS_TILT_PROJECTION_PER_STEP || accepted % c->tilt_proj_interval != 0) return MS_OK;
    return tbb_enforce(true);
  };
  if (rp->solver == 0) {  // gradient descent (:312-351 / :892-1058)
    for (int it = 0; it < rp->max_iters; ++it) {
      rc = grad_at(&E0, &gnorm, &rz_old);
      if (rc) return rc;
      if (gnorm == 0.0 || (tol > 0.0 && gnorm < tol)) break;
      bool acc = false;
      double E1 = E0;
      rc = search_any(false, -1.0, E0, &E1, &acc);
      if (rc) return rc;
      ++iters;
      if (!acc) break;
      rc = tbb_after_accept();
      if (rc) return rc;
    }
  } else {  // (preconditioned) Fletcher-Reeves CG (:352-421 / :1059-1398)
    rc = grad_at(&E0, &gnorm, &rz_old);
    if (rc) return rc;
    if (!(gnorm == 0.0 || (tol > 0.0 && gnorm < tol))) {
      rc = tvec_all(1, false, 0.0, 1);
      if (rc) return rc;
      for (int it = 0; it < rp->max_iters; ++it) {
        if (gnorm == 0.0 || (tol > 0.0 && gnorm < tol)) break;
        bool acc = false;
        double E1 = E0;
        rc = search_any(true, 1.0, E0, &E1, &acc);
        if (rc) return rc;
        ++iters;
        if (!acc) break;
        rc = tbb_after_accept();
        if (rc) return rc;
        double rz_new = 0.0;
        rc = grad_at(&E0, &gnorm, &rz_new);
        if (rc) return rc;
        if (gnorm == 0.0 || (tol > 0.0 && gnorm < tol)) break;
        if (rz_old == 0.0) break;
        const double beta = rz_new / rz_old;
        rc = tvec_all(1, false, beta, 0);
        if (rc) return rc;
        rz_old = rz_new;
      }
    }
  }
  if (c->tilt_proj_cadence == MS_TILT_PROJECTION_PER_PASS) {  // :1416-1417
    rc = tbb_enforce(true);
    if (rc) return rc;
  }
  rc = tbb_enforce(false);  // :1474-1478, the stored field
  if (rc) return rc;
  if (iters_out) *iters_out = iters;
  if (evals_out) *evals_out = evals;
  // the tilt-dependent energies in the mailbox belong to whatever was evaluated last
  c->carry.carry_valid = c->carry.grad_valid = false;
  c->carry.factors_valid = c->carry.factors_valid && !(mods & (MS_MOD_BENDING_TILT | MS_LEAFLET_BT));
  return MS_OK;
}
}  // namespace

int ms_tilt_energy_and_gradient(ms_ctx* c, double* energy, double* tilt_grad) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_tilt_energy_and_gradient: NULL argument");
  if (!(c->params.modules & MS_TILT_MODS) || !c->tf[0].tilts)
    return fail(c, MS_ERR_STATE, "ms_tilt_energy_and_gradient: no tilt-reading module / no tilts set");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "tilt passes are single-shard only");
  int rc = ensure_bt_record(c);
  if (rc) return rc;
  rc = tilt_eval(c, false, true);
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  *energy = tilt_energy_from_mailbox(c);
  if (tilt_grad) return patch_to_ext(c, c->tf[0].grad, tilt_grad, 3);
  return MS_OK;
}

int ms_relax_tilts(ms_ctx* c, const ms_tilt_relax_params* rp, int* iters_out, int* evals_out) {
  if (!c || !rp) return fail(c, MS_ERR_INVALID, "ms_relax_tilts: NULL argument");
  if (iters_out) *iters_out = 0;
  if (evals_out) *evals_out = 0;
  const uint32_t mods = c->params.modules;
  if (!(mods & MS_TILT_MODS) || !c->tf[0].tilts)
    return fail(c, MS_ERR_STATE, "ms_relax_tilts: no tilt-reading module / no tilts set");
  if (mods & MS_LEAFLET_MODS)
    return fail(c, MS_ERR_STATE, "ms_relax_tilts: leaflet modules are active, use ms_relax_leaflet_tilts");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "tilt passes are single-shard only");
  if (rp->step_size <= 0.0 || rp->max_iters <= 0) return MS_OK;
  TiltField* fl[1] = {&c->tf[0]};
  return relax_fields(c, rp, fl, 1, /*jacobi_smooth_by_param=*/false, iters_out, evals_out);
}

// ---- two-leaflet tilt fields ---------------------------------------------------------------
int ms_set_leaflet_tilts(ms_ctx* c, int leaflet, const double* tilts, const uint8_t* tilt_fixed,
                         const ms_leaflet_params* lp) {
  if (!c || !tilts || !lp) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_tilts: NULL argument");
  if (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_tilts: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  TiltField& f = c->tf[1 + leaflet];
  const Tiling& t = c->til;
  const size_t bytes = sizeof(double) * 3 * (size_t)t.nvp;
  if (!f.tilts) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.tilts), bytes));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.grad), bytes));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.trial), bytes));
    HIPCHK(c, hipMemset(f.tilts, 0, bytes));
    HIPCHK(c, hipMemset(f.grad, 0, bytes));
    HIPCHK(c, hipMemset(f.trial, 0, bytes));
  }
  f.k_tilt = lp->tilt_modulus;
  f.consistent = lp->tilt_mass_consistent ? 1 : 0;
  f.k_smooth = lp->smoothness;
  f.k_smooth_precond = lp->precond_smoothness;
  bool flags_changed = false;
  for (int i = 0; i < t.nv; ++i) {
    uint8_t fl = c->h_vflags[(size_t)i] & (uint8_t)~f.fixed_bit;
    if (tilt_fixed && tilt_fixed[t.perm[i]]) fl |= f.fixed_bit;
    flags_changed = flags_changed || fl != c->h_vflags[(size_t)i];
    c->h_vflags[(size_t)i] = fl;
  }
  if (flags_changed || !tilt_fixed) {
    f.any_free = t.nv == 0 || !tilt_fixed;
    for (int i = 0; i < t.nv && !f.any_free; ++i) f.any_free = !(c->h_vflags[(size_t)i] & f.fixed_bit);
  }
  if (flags_changed) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipMemcpy(c->d_vflags, c->h_vflags.data(), c->h_vflags.size(), hipMemcpyHostToDevice));
  }
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return ext_to_patch(c, tilts, f.tilts, 3);
}

namespace {
// flags[i] of library row i takes VF_ABSENT_OUT from absent[perm[i]] (NULL: from nobody) and keeps its other bits
// -> 1 some flag changed | 2 some row carries the bit
int absent_flags_apply(int nv, const int32_t* perm, const uint8_t* absent, uint8_t* flags) {
  int r = 0;
  for (int i = 0; i < nv; ++i) {
    uint8_t fl = flags[i] & (uint8_t)~VF_ABSENT_OUT;
    if (absent && absent[perm[i]]) fl |= VF_ABSENT_OUT;
    if (fl & VF_ABSENT_OUT) r |= 2;
    if (fl != flags[i]) r |= 1;
    flags[i] = fl;
  }
  return r;
}
}  // namespace

int ms_leaflet_absent_flags_host(int nv, const int32_t* perm, const uint8_t* absent, uint8_t* flags, int* state) {
  if (nv < 0 || (nv > 0 && (!perm || !flags))) return fail(nullptr, MS_ERR_INVALID, "ms_leaflet_absent_flags_host: bad argument");
  for (int i = 0; i < nv; ++i)
    if (perm[i] < 0 || perm[i] >= nv) return fail(nullptr, MS_ERR_INVALID, "ms_leaflet_absent_flags_host: permutation out of range");
  const int r = absent_flags_apply(nv, perm, absent, flags);
  if (state) *state = r;
  return MS_OK;
}

// Rows the outer leaflet is absent on (leaflet_presence.py:34-122), through the vertex permutation as ms_set_tilt_fixed
// takes its flags; NULL clears.  No per-facet array: a facet is masked when one of its corners carries VF_ABSENT_OUT.
int ms_set_leaflet_absent(ms_ctx* c, int leaflet, const uint8_t* absent) {
  if (!c) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_absent: NULL context");
  if (leaflet == MS_LEAFLET_IN)
    return fail(c, MS_ERR_UNSUPPORTED, "ms_set_leaflet_absent: an absent inner leaflet is outside the device path");
  if (leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_absent: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  if (c->shard_count != 1) return fail(c, MS_ERR_UNSUPPORTED, "ms_set_leaflet_absent: tilt passes are single-shard only");
  TiltField& f = c->tf[1 + leaflet];
  const Tiling& t = c->til;
  const int state = absent_flags_apply(t.nv, t.perm.data(), absent, c->h_vflags.data());
  f.absent_bit = (state & 2) ? VF_ABSENT_OUT : 0;
  if (state & 1) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    HIPCHK(c, hipMemcpy(c->d_vflags, c->h_vflags.data(), c->h_vflags.size(), hipMemcpyHostToDevice));
  }
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return MS_OK;
}

int ms_set_leaflet_bending(ms_ctx* c, int leaflet, const double* kappa, const double* c0) {
  if (!c || !kappa || !c0) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_bending: NULL argument");
  if (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_bending: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  TiltField& f = c->tf[1 + leaflet];
  const Tiling& t = c->til;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  if (!f.kappa) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.kappa), sizeof(double) * (size_t)t.nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.c0), sizeof(double) * (size_t)t.nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.bt_vert), sizeof(double) * 4 * (size_t)t.nvp));
    HIPCHK(c, hipMemset(f.bt_vert, 0, sizeof(double) * 4 * (size_t)t.nvp));
  }
  std::vector<double> k((size_t)t.nvp, 0.0), z((size_t)t.nvp, 0.0);
  for (int i = 0; i < t.nv; ++i) {
    k[i] = kappa[t.perm[i]];
    z[i] = c0[t.perm[i]];
  }
  HIPCHK(c, hipMemcpy(f.kappa, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(f.c0, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice));
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  return MS_OK;
}

int ms_set_leaflet_disk_target(ms_ctx* c, int leaflet, const uint8_t* disk_rows, const ms_disk_target_params* p) {
  if (!c || !p) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_disk_target: NULL argument");
  if (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT)
    return fail(c, MS_ERR_INVALID, "ms_set_leaflet_disk_target: leaflet must be MS_LEAFLET_IN or MS_LEAFLET_OUT");
  TiltField& f = c->tf[1 + leaflet];
  const Tiling& t = c->til;
  const double nn = std::sqrt(p->normal[0] * p->normal[0] + p->normal[1] * p->normal[1] + p->normal[2] * p->normal[2]);
  if (!(nn >= 1e-15)) return fail(c, MS_ERR_INVALID, "ms_set_leaflet_disk_target: a plane normal is required");
  HIPCHK(c, hipStreamSynchronize(S(c)));
  if (!f.disk) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.disk), (size_t)t.nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.diff), sizeof(double) * 3 * (size_t)t.nvp));
    HIPCHK(c, hipMemset(f.diff, 0, sizeof(double) * 3 * (size_t)t.nvp));
  }
  std::vector<uint8_t> m((size_t)t.nvp, 0);
  for (int i = 0; i < t.nv && disk_rows; ++i) m[(size_t)i] = disk_rows[t.perm[i]] ? 1 : 0;
  HIPCHK(c, hipMemcpy(f.disk, m.data(), m.size(), hipMemcpyHostToDevice));
  f.dt = *p;
  for (int k = 0; k < 3; ++k) f.dt.normal[k] = p->normal[k] / nn;  // tilt_disk_target_in.py:73-77
  c->carry.invalidate();
  return MS_OK;
}

int ms_get_leaflet_tilts(ms_ctx* c, int leaflet, double* tilts) {
  if (!c || !tilts || (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT) || !c->tf[1 + leaflet].tilts)
    return fail(c, MS_ERR_INVALID, "ms_get_leaflet_tilts: bad leaflet / no tilts set");
  return patch_to_ext(c, c->tf[1 + leaflet].tilts, tilts, 3);
}

int ms_get_leaflet_relax_geometry(ms_ctx* c, int leaflet, double* vertex_areas, double* minv) {
  if (!c || (leaflet != MS_LEAFLET_IN && leaflet != MS_LEAFLET_OUT))
    return fail(c, MS_ERR_INVALID, "ms_get_leaflet_relax_geometry: bad leaflet");
  const TiltField& f = c->tf[1 + leaflet];
  if (!f.va || !f.minv) return fail(c, MS_ERR_STATE, "ms_get_leaflet_relax_geometry: this leaflet was never relaxed");
  if (vertex_areas)
    if (int rc = patch_to_ext(c, f.va, vertex_areas, 1)) return rc;
  if (minv) return patch_to_ext(c, f.minv, minv, 1);
  return MS_OK;
}

namespace {
int leaflet_ready(ms_ctx* c, const char* who, TiltField** fl, int* nf) {
  const uint32_t mods = c->params.modules;
  if (!(mods & MS_LEAFLET_MODS)) return fail(c, MS_ERR_STATE, std::string(who) + ": no leaflet module is active");
  if (mods & MS_TILT_MODS)
    return fail(c, MS_ERR_STATE, std::string(who) + ": single-field and leaflet tilt modules together are outside the device path");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "tilt passes are single-shard only");
  *nf = 0;
  for (int l = 1; l <= 2; ++l) {
    TiltField& f = c->tf[l];
    if (!(mods & f.mods())) continue;
    if (!f.tilts) return fail(c, MS_ERR_STATE, std::string(who) + ": ms_set_leaflet_tilts was not called for an active leaflet");
    fl[(*nf)++] = &f;
  }
  return MS_OK;
}
}  // namespace

int ms_leaflet_tilt_energy_and_gradient(ms_ctx* c, double* energy, double* grad_in, double* grad_out) {
  return ms_leaflet_tilt_energy_and_gradient_ex(c, 0, energy, grad_in, grad_out);
}

int ms_leaflet_tilt_energy_and_gradient_ex(ms_ctx* c, int module_form, double* energy, double* grad_in,
                                           double* grad_out) {
  if (!c || !energy) return fail(c, MS_ERR_INVALID, "ms_leaflet_tilt_energy_and_gradient: NULL argument");
  TiltField* fl[2];
  int nf = 0;
  int rc = leaflet_ready(c, "ms_leaflet_tilt_energy_and_gradient", fl, &nf);
  if (rc) return rc;
  c->tilt_module_form = module_form != 0;
  rc = tilt_eval(c, false, true);
  c->tilt_module_form = false;
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  *energy = tilt_energy_from_mailbox(c);
  double* outs[2] = {grad_in, grad_out};
  for (int l = 0; l < 2; ++l) {
    if (!outs[l]) continue;
    TiltField& f = c->tf[1 + l];
    if (f.tilts && (c->params.modules & f.mods())) {
      rc = patch_to_ext(c, f.grad, outs[l], 3);
      if (rc) return rc;
    } else {
      memset(outs[l], 0, sizeof(double) * 3 * (size_t)c->til.nv);
    }
  }
  return MS_OK;
}

int ms_relax_leaflet_tilts(ms_ctx* c, const ms_tilt_relax_params* rp, int* iters_out, int* evals_out) {
  if (!c || !rp) return fail(c, MS_ERR_INVALID, "ms_relax_leaflet_tilts: NULL argument");
  if (iters_out) *iters_out = 0;
  if (evals_out) *evals_out = 0;
  TiltField* fl[2];
  int nf = 0;
  int rc = leaflet_ready(c, "ms_relax_leaflet_tilts", fl, &nf);
  if (rc) return rc;
  if (rp->step_size <= 0.0 || rp->max_iters <= 0) return MS_OK;
  return relax_fields(c, rp, fl, nf, /*jacobi_smooth_by_param=*/true, iters_out, evals_out);
}
