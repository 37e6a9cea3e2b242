// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): energy / gradient entry points, line-search rounds, ms_step, volume projection, the resident step, ms_minimize.
int ms_set_positions(ms_ctx* c, const double* positions) {
  if (!c || !positions) return fail(c, MS_ERR_INVALID, "ms_set_positions: NULL argument");
  c->carry.factors_valid = false;
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  return ext_to_patch(c, positions, c->buf[MS_BUF_X], 3);
}

int ms_get_positions(ms_ctx* c, double* positions) {
  if (!c || !positions) return fail(c, MS_ERR_INVALID, "ms_get_positions: NULL argument");
  return patch_to_ext(c, c->buf[MS_BUF_X], positions, 3);
}

int ms_get_gradient(ms_ctx* c, double* grad) {
  if (!c || !grad) return fail(c, MS_ERR_INVALID, "ms_get_gradient: NULL argument");
  return patch_to_ext(c, c->carry.last_g, grad, 3);
}

int ms_get_vertex_buffer(ms_ctx* c, int buffer, double* out) {
  if (!c || !out || buffer < 0 || buffer > MS_BUF_FA)
    return fail(c, MS_ERR_INVALID, "ms_get_vertex_buffer: bad argument");
  if (buffer == MS_BUF_D && c->carry.kc_pending) {
    // the gradient pass queued behind the accepted trial has run: D is that pass's direction (the carried flags still
    // describe the step before it) -- stored by the pass, or left to k_direction
    if (int rc = materialize_direction(c, c->kc_dir_unwritten[c->carry.kc_parity])) return rc;
  } else if (buffer == MS_BUF_D && c->carry.dir_unwritten) {
    if (int rc = materialize_direction(c)) return rc;
  } else if ((buffer == MS_BUF_D && c->carry.dir_implicit) || (buffer == MS_BUF_PD && c->carry.pd_neg_pg)) {
    // the direction asked for exists only as -G / -PG: write it out
    const int src = buffer == MS_BUF_D ? MS_BUF_G : MS_BUF_PG;
    HIPCHK(c, launch_direction(c->tile0, c->tile1, c->til.nv, c->til.own, c->d_vflags, c->buf[src], c->buf[MS_BUF_GC],
                               c->buf[buffer], c->buf[MS_BUF_PG], c->buf[MS_BUF_PD], c->d_scal, 0, 0, c->d_partials,
                               c->til.n_tiles, 0, c->stream));
    if (buffer == MS_BUF_D) c->carry.dir_implicit = false; else c->carry.pd_neg_pg = false;
  }
  return patch_to_ext(c, c->buf[buffer], out, buffer == MS_BUF_FA ? 2 : 3);
}

int ms_energy_and_gradient(ms_ctx* c, double energies[4], double* grad) {
  if (!c || !energies) return fail(c, MS_ERR_INVALID, "ms_energy_and_gradient: NULL argument");
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_energy_and_gradient: sharded contexts use the phase API");
  int rc = queue_energy_and_gradient(c, MS_STEPPER_GD, false);
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  energies_from_mailbox(c, energies);
  if (grad) return patch_to_ext(c, c->buf[MS_BUF_G], grad, 3);
  return MS_OK;
}

int ms_energy_and_raw_gradient(ms_ctx* c, double energies[4], double* grad) {
  if (!c || !energies) return fail(c, MS_ERR_INVALID, "ms_energy_and_raw_gradient: NULL argument");
  if (c->shard_count != 1)
    return fail(c, MS_ERR_STATE, "ms_energy_and_raw_gradient: sharded contexts use the phase API");
  const uint32_t mods = c->params.modules;
  const bool penalty = (mods & (MS_MOD_VOLUME_PENALTY | MS_MOD_AREA_PENALTY)) != 0;  // K_C reads the reduced volume / body area
  int rc = leaflet_gradient_admit(c, mods);
  if (rc) return rc;
  rc = phase_energy(c, mods, false, 0.0, false, false, true, /*reduce_now=*/penalty);
  if (rc) return rc;
  c->carry.grad_valid = false;  // G receives the raw gradient: no fixed-row zeroing, no KKT projection
  rc = phase_gradient(c, mods, c->buf[MS_BUF_G], false, 0, /*reduce_now=*/false);
  if (rc) return rc;
  rc = reduce_slots(c, (penalty ? 0u : energy_mask(mods)) | MASK_GRAD);
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  energies_from_mailbox(c, energies);
  if (grad) return patch_to_ext(c, c->buf[MS_BUF_G], grad, 3);
  return MS_OK;
}

int ms_energy(ms_ctx* c, double energies[4]) {
  if (!c || !energies) return fail(c, MS_ERR_INVALID, "ms_energy: NULL argument");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_energy: sharded contexts use the phase API");
  if (c->carry.carry_valid) {
    // the last accepted trial (or the pass before a failed search) evaluated exactly this x and its energies are
    // still in the mailbox: no pass, and the carried state survives for the next step
    energies_from_mailbox(c, energies);
    return MS_OK;
  }
  int rc = phase_energy(c, c->params.modules, false, 0.0, false, false, false);
  if (rc) return rc;
  rc = fetch(c);
  if (rc) return rc;
  energies_from_mailbox(c, energies);
  return MS_OK;
}

int ms_reset_stepper(ms_ctx* c) {
  if (!c) return MS_ERR_INVALID;
  // (a pass still queued behind an acceptance has its history until here: D of that pass, if anybody asks later)
  if (c->carry.kc_pending)
    if (int rc = materialize_direction(c, c->kc_dir_unwritten[c->carry.kc_parity])) return rc;
  c->carry.cg_have_history = false;
  c->carry.cg_iter_count = 0;
  c->carry.pd_neg_pg = false;
  c->carry.dir_unwritten = false;  // (its history is gone: the direction nobody stored is nobody's any more)
  return MS_OK;
}

namespace {
int spec_prepare(ms_ctx* c) {
  if (c->d_dec) return MS_OK;
  auto make_box = [&](ms_ctx::Mailbox& m) -> int { return make_mailbox(c, m); };
  if (c->pair_enable) {
    const size_t nvp = (size_t)std::max<int64_t>(1, c->til.nvp);
    // early trial 0 may write outputs of its own (the sharded pair, MS_PAIR_LEAN=0), early trial 1 only in ms_step
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->xt2), sizeof(double) * 3 * nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->fK2), sizeof(double) * 3 * nvp));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->fA2), sizeof(double) * 2 * nvp));
    if (c->shard_count == 1 && !c->pair_lean_enable) {
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->xt3), sizeof(double) * 3 * nvp));
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->fK3), sizeof(double) * 3 * nvp));
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->fA3), sizeof(double) * 2 * nvp));
    }
    const int n_side = c->shard_count == 1 ? ms_ctx::N_SIDE : 1;  // (the sharded driver pairs, no more)
    if (int rc = ensure_side_sets(c, n_side)) return rc;
  }
  for (int p = 0; p < 2; ++p) {
    for (int k = 0; k < ms_ctx::SPEC_STAGES; ++k) {
      int rc = make_box(c->spec[p][k]);
      if (rc) return rc;
    }
    int rc = make_box(c->grad_mb[p]);
    if (rc) return rc;
    rc = make_box(c->first_mb[p]);
    if (rc) return rc;
  }
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_dec), sizeof(uint32_t) * MS_DEC_STRIDE * ms_ctx::N_DEC));
  HIPCHK(c, hipMemset(c->d_dec, 0, sizeof(uint32_t) * MS_DEC_STRIDE * ms_ctx::N_DEC));
  return MS_OK;
}
// the host knows a gated fold stayed out (an earlier stage was accepted, or nothing was): nobody waits for its ticket
inline void forget(ms_ctx::Mailbox& m) {
  for (int sl = 0; sl < MS_MB_WORDS; ++sl) m.expected[sl] = 0;
}
// what the recent searches of a kind say about the acceptance threshold: no alpha above a_hi was accepted, and alphas
// down to r_lo were rejected (INFINITY: nothing was rejected lately -- the step size is still growing)
inline void ls_bounds(const ms_ctx::LsHist& lh, double& a_hi, double& r_lo) {
  a_hi = 0.0;
  r_lo = INFINITY;
  for (int k = 0; k < std::min(lh.n, (int)ms_ctx::LS_HIST); ++k) {
    a_hi = std::max(a_hi, lh.acc[k]);
    r_lo = std::min(r_lo, lh.rej[k]);
  }
}
// the trial energy a queued stage is decided on, from that stage's scalars (surface + bending: ms_step's can_chain)
inline double stage_energy(const ms_ctx* c, const double* v) {
  return ((c->params.modules & MS_MOD_SURFACE) ? v[MS_S_ESURF] : 0.0) +
         ((c->params.modules & MS_MOD_BENDING) ? v[MS_S_EBEND] : 0.0);
}
// the energy scalars of a stage's mailbox become the context's own
inline void adopt_scalars(ms_ctx* c, const double* v) {
  for (int sl = 0; sl < MS_NSCAL; ++sl)
    if (energy_mask(c->params.modules) & (1u << sl)) put_mailbox(c, sl, v[sl]);
}
// the gradient pass behind an acceptance computes a direction with CG history (conjugate_gradient.py:78-82)
inline bool next_use_history(const ms_ctx* c, bool cg, int restart) { return cg && ((c->carry.cg_iter_count + 1) % restart != 0); }
}  // namespace

// ---- line-search rounds (ms_step) ------------------------------------------------------------------------------
// A round = one ungated (or GO-gated) energy launch of n0 trials, n_st single-trial stages gated behind it, and the
// gradient + direction pass of the accepted point gated behind those.
namespace {
// plan a round from `alpha` on (prediction only: the same alphas are tested in the same order whatever is chosen)
void plan_round(ms_ctx* c, const ms_stepper_params* sp, double alpha, int room, int rejected_here, double a_hi,
                double r_lo, bool ls_warm, int pred_trials, int trials_so_far, RoundPlan& plan, bool ahead = false) {
  const bool multi_ok = c->pair_enable && c->side[0].partials != nullptr && (c->params.modules & MS_MOD_BENDING) != 0;
  const int n0_cap = !multi_ok ? 1 : (c->pair_lean_enable ? MS_MAX_TRIALS : (c->fK3 ? 3 : 2));
  double* alphas = plan.alphas;
  int n_alpha = 1;  // alphas of the ladder from here that are still >= 1e-8
  alphas[0] = alpha;
  while (n_alpha < room && n_alpha < MS_MAX_TRIALS + ms_ctx::SPEC_STAGES && alphas[n_alpha - 1] * sp->beta >= 1e-8) {
    alphas[n_alpha] = alphas[n_alpha - 1] * sp->beta;
    ++n_alpha;
  }
  int n0 = 1, n_st = 0;
  // A search that has rejected `escalate_after` alphas already will most likely reject more: from there on a round
  // evaluates as many trials as the search has rejected so far in ONE launch (the early ones of a launch cost an
  // energy-only evaluation each), whatever the history of the earlier searches says.
  const int force = c->pair_force;
  if (!force && c->escalate && multi_ok && rejected_here >= c->escalate_after) {
    n0 = std::max(1, std::min(std::min(n_alpha, n0_cap), rejected_here));
  } else if (!force && !ahead && c->escalate && multi_ok && !ls_warm && room >= 3 && pred_trials - trials_so_far >= room) {
    // no history of accepted alphas, and the last search of this kind ran out of its trials (in the cold phase of the
    // headline run: every search along a CG direction): this one is expected to as well -- as many trials per launch
    // as there are sets.  (One search that needed five trials says little about the next: an early accept in a
    // multi-trial launch costs more than the rounds it saves.  And not in a round queued ahead: whether that search
    // happens at all is a guess already.)
    n0 = std::min(n_alpha, n0_cap);
  } else {
    const bool can_spec = force || (ls_warm ? r_lo < INFINITY : pred_trials > 1);
    int depth = 1;
    if (can_spec) {
      // how many trials to queue: as many as the last search needed (cold), or -- once there is a history --
      // one per alpha that still lies above (most of) the range where alphas were accepted lately
      const int room4 = std::min(1 + ms_ctx::SPEC_STAGES, n_alpha);
      const int want = force ? std::min(std::min(force, 3), room4)
                             : (ls_warm ? room4 : std::min(pred_trials - trials_so_far, room4));
      while (depth < want) {
        if (!force && ls_warm && !(alphas[depth - 1] > 0.9 * a_hi)) break;
        ++depth;
      }
    }
    // two or more trials expected: the first two share one launch (and the ladder stops there for this round)
    // ... and only when the first one is expected to fail: it lies above every alpha accepted lately, and alphas
    // were rejected lately (a wasted evaluation costs more than a saved round trip gains)
    const bool pair = depth > 1 && multi_ok && (force || (ls_warm && alpha > 1.05 * a_hi && r_lo < INFINITY));
    if (pair) {
      depth = std::min(depth, 3);
      // triple launch: trial 1 is expected to fail as well -- its alpha is not below one that was rejected lately
      const bool triple = depth == 3 && n0_cap >= 3 && (force ? force == 4 : alphas[1] > r_lo);
      // otherwise the pair, and one gated trial behind it when trial 1 is as sure to fail as trial 0 (an empty gated
      // stage costs about what the host round trip it saves does, so "probably" is not enough)
      if (depth == 3 && !triple && !force && !(alphas[1] > a_hi)) depth = 2;
      n0 = triple ? 3 : 2;
      n_st = depth - n0;
    } else {
      n0 = 1;
      n_st = depth - 1;
    }
  }
  plan.n0 = n0;
  plan.n_st = n_st;
}

// queue a planned round into the mailboxes / decision records of `parity`.  merged: the round belongs to a step that
// has not started -- its first launch runs right behind the gradient pass of round `go_src`, whose direction scalars
// the round's first fold folds itself; that fold decides first whether the search happens at all (FoldArgs::go_kind)
// and forms the Armijo right-hand sides on the device.
int queue_round(ms_ctx* c, const ms_stepper_params* sp, const RoundPlan& plan, int parity, double energy0,
                double g_dot_d, bool merged, int go_src, bool carry_mode, bool cg, int restart) {
  const bool go_gated = merged;
  const int n0 = plan.n0, n_st = plan.n_st;
  const double* alphas = plan.alphas;
  int rc;
  // first launch: trials 0 .. n0-1, the early ones into the side sets, the last one into the ordinary outputs;
  // its fold decides all of them and writes decision record 0
  {
    StageCtl st;
    st.cur_parity = parity;  // (read by a multi-trial fold only: the gated stages and the gradient pass keep 0)
    st.pair_on = n0 > 1 ? n0 : 0;
    st.pair_lean = n0 > 1 && c->pair_lean_enable;
    for (int j = 0; j + 1 < n0; ++j) st.pair_alpha[j] = alphas[j];
    st.cur_gate_want = DEC_ACCEPT_MAIN;
    st.cur_dec = dec_word(c, parity, 0);
    for (int j = 0; j < n0; ++j) st.cur_rhs[j] = energy0 + sp->c * alphas[j] * g_dot_d;
    if (merged) {
      // the fold (not the energy kernel) is tied to the gradient pass in front: it checks that pass's ran count,
      // and what it tests before it decides the trials (FoldArgs::go_kind) is what queue_ahead put into c->ahead
      const ms_ctx::Ahead& ah = c->ahead;
      st.cur_gate = c->kc_gate[go_src];
      st.cur_gate_fold_only = st.cur_check_ran = true;
      st.cur_extra_mask = c->dir_mask[go_src];
      st.cur_go_kind = ah.go_kind;
      st.cur_go = go_word(c, go_src);
      const double go_val[6] = {ah.tol2p, ah.lim, ah.energy0, ah.c1, ah.alpha0, ah.beta};
      memcpy(st.cur_go_val, go_val, sizeof(go_val));
    }
    swap_mailbox(c, c->first_mb[parity]);
    StageScope scope(c, st);
    rc = phase_energy(c, c->params.modules, true, alphas[n0 - 1], true, false, carry_mode);
    if (merged) c->dir_pending[go_src] = false;
    swap_mailbox(c, c->first_mb[parity]);
    if (rc) return rc;
  }
  // gated stages: stage s runs iff record s-1 says DEC_CONTINUE
  for (int s2 = 1; s2 <= n_st; ++s2) {
    swap_mailbox(c, c->spec[parity][s2 - 1]);
    StageCtl st;
    st.cur_gate = dec_word(c, parity, s2 - 1);
    st.cur_gate_want = DEC_CONTINUE;
    st.cur_check_ran = true;
    st.cur_dec = dec_word(c, parity, s2);
    st.cur_rhs[0] = energy0 + sp->c * alphas[n0 + s2 - 1] * g_dot_d;
    st.cur_rhs_dev = go_gated ? go_rhs(c, go_src) + (n0 + s2 - 1) : nullptr;
    StageScope scope(c, st);
    rc = phase_energy(c, c->params.modules, true, alphas[n0 + s2 - 1], true, false, carry_mode);
    swap_mailbox(c, c->spec[parity][s2 - 1]);
    if (rc) return rc;
  }
  {
    // the next step's gradient pass in the state an acceptance produces (x <-> xt, CG history swapped, factors of
    // the accepted trial), gated on "the accepted trial is the one in the ordinary buffers"; every change of the
    // context is undone afterwards.  Its direction fold can open the round after this one (queue_ahead).
    // (of the carried state the pass writes factors_valid, dir_implicit, pd_neg_pg, last_g and the three flags the
    // pin project lane clears; it never runs with a tilt module -- rounds are queued only without one and without an
    // enforcer, pins next to tilt modules included -- so nothing of it touches the rest)
    const bool next_hist = next_use_history(c, cg, restart);
    const CarryState s_carry = c->carry;
    std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
    if (cg) {
      std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
      std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
      c->carry.pd_neg_pg = c->carry.dir_implicit;
    }
    c->carry.factors_valid = true;
    swap_mailbox(c, c->grad_mb[parity]);
    StageCtl st;
    st.cur_gate = dec_word(c, parity, n_st);
    st.cur_gate_want = DEC_ACCEPT_MAIN;
    st.cur_check_ran = true;
    // inside ms_minimize the direction fold of this pass is left to the first fold of the round after this one
    st.defer_dir = c->ahead_allowed && sp->edge_fraction <= 0.0;
    c->dir_deferred_mask = 0;
    StageScope scope(c, st);
    rc = queue_energy_and_gradient(c, sp->stepper, next_hist, /*skip_energy=*/true);
    c->kc_dir_unwritten[parity] = c->carry.dir_unwritten;  // (the carried copy goes with the restore below)
    c->dir_pending[parity] = st.defer_dir && c->dir_deferred_mask != 0;
    c->dir_mask[parity] = c->dir_deferred_mask;
    c->kc_gate[parity] = dec_word(c, parity, n_st);
    swap_mailbox(c, c->grad_mb[parity]);
    if (cg) {
      std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
      std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
    }
    std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
    c->carry = s_carry;
    if (rc) return rc;
  }
  return MS_OK;
}

// the direction fold of round `parity`'s gradient pass was left out and nobody merged it: launch it on its own
int flush_dir_fold(ms_ctx* c, int parity) {
  if (!c->dir_pending[parity]) return MS_OK;
  c->dir_pending[parity] = false;
  swap_mailbox(c, c->grad_mb[parity]);
  StageCtl st;
  st.cur_gate = c->kc_gate[parity];
  st.cur_gate_want = DEC_ACCEPT_MAIN;
  st.cur_check_ran = true;
  StageScope scope(c, st);
  const int rc = reduce_slots(c, c->dir_mask[parity]);
  swap_mailbox(c, c->grad_mb[parity]);
  return rc;
}

// nobody will take the results of the round queued ahead.  ran 0: none of its kernels ran; 1: its first energy launch
// ran and everything behind it stayed out (the fold said DEC_STOP): the bending factors, the trial positions and the
// device scalars are that launch's now, the host's scalars and G still describe x; 2: any of it may have run (the
// gradient pass behind an acceptance writes the CG history buffers)
void drop_ahead(ms_ctx* c, int ran) {
  if (!c->ahead.valid) return;
  const int p = c->ahead.parity;
  forget(c->first_mb[p]);
  forget(c->grad_mb[p]);
  for (auto& m : c->spec[p]) forget(m);
  for (auto& sd : c->side) forget(sd.mb[p]);
  c->dir_pending[p] = false;
  c->ahead.valid = false;
  ++c->q_dropped;
  if (ran >= 1) c->carry.factors_valid = false;
  if (ran >= 2) {
    c->carry.invalidate();
    c->carry.kc_pending = false;
    c->carry.cg_have_history = false;
    c->carry.cg_iter_count = 0;
    c->carry.pd_neg_pg = false;
    c->carry.dir_unwritten = false;
  }
}

// The step has accepted a trial and the gradient pass of the new x is running (queued with the round, gated on the
// acceptance).  Queue the first round of the NEXT search behind it now: what the host does not know yet -- <g,d> of
// the new gradient, whether the iteration converges, whether the trials need the normal-rotation guard -- the
// direction fold of that pass decides from its own scalars (FoldArgs::go_out) with the parameters handed to it here.
//   kind 1: the pass computes a direction with CG history; in the steady state of the headline workload that is no
//           descent direction, the step fails without a trial, the stepper is reset and the step after it searches
//           along d = -g with the same step size: that search's first round is queued;
//   kind 2: the pass computes d = -g itself (gradient descent, CG restart steps): the next step's own first round.
int queue_ahead(ms_ctx* c, const ms_stepper_params* sp, const ms_step_result* out, double tol, bool carry_mode,
                bool cg, int restart) {
  if (!c->carry.kc_pending || c->ahead.valid) return MS_OK;
  const int src = c->carry.kc_parity;
  if (!c->dir_pending[src]) return MS_OK;  // (the pass was queued with its own direction fold)
  // kind 1: CG history, and the last direction with history was no descent direction; 3: it was one -- the next step
  // searches along the direction this pass writes; 2: the pass writes d = -g itself
  const int kind = c->kc_use_history ? (c->last_hist_descent ? 3 : 1) : 2;
  // (kind 3 searches along the D of a pass that was queued before last_hist_descent turned true and did not store it:
  // that round waits for its step, which writes D out first)
  if (kind == 3 && c->kc_dir_unwritten[src]) return flush_dir_fold(c, src);
  const double alpha0 = out->next_step;
  const double me2 = c->h_scal[MS_S_MINEDGE2];
  if (c->steps_left < (kind == 1 ? 2 : 1) || !(alpha0 >= 1e-8) || sp->edge_fraction > 0.0)
    return flush_dir_fold(c, src);  // (the step it would belong to is not part of this call)
  // line-search history as the consuming step will see it (accept() has just added this search)
  double a_hi, r_lo;
  const ms_ctx::LsHist& lh = c->ls[kind == 3 ? 1 : 0];  // (kinds 1 and 2 search along -g)
  ls_bounds(lh, a_hi, r_lo);
  const int max_iter = sp->max_iter > 0 ? sp->max_iter : 10;
  ms_ctx::Ahead& ah = c->ahead;
  plan_round(c, sp, alpha0, max_iter, 0, a_hi, r_lo, lh.n >= 2, lh.pred_trials, 0, ah.plan, /*ahead=*/true);
  if (ah.plan.n0 + ah.plan.n_st > MS_MAX_TRIALS) return flush_dir_fold(c, src);  // (the fold forms that many right-hand sides)
  ah.kind = kind;
  ah.stepper = sp->stepper;
  ah.implicit = kind == 1;
  ah.alpha0 = alpha0;
  ah.energy0 = out->energy;
  ah.beta = sp->beta;
  ah.c1 = sp->c;
  ah.max_iter = max_iter;
  ah.tol2p = tol * tol * (1.0 + 1e-9);
  ah.lim = (c->til.nf > 0 && me2 > 0.0) ? (0.09 * me2 / (1.0 + 1e-9)) / (alpha0 * alpha0) : INFINITY;
  ah.src = src;
  ah.go = false;
  ah.go_known = false;
  // what the round's first fold tests before it decides the trials (FoldArgs::go_kind, with the parameters above)
  ah.go_kind = kind == 1 ? 1 : 2;
  // the round itself, in the state the consuming step will be in
  // (queueing a trial pass marks the carried state as gone; for a round that belongs to a later step it is not)
  const CarryState s_carry = c->carry;
  if (kind == 1) {  // (after the failed step: ms_reset_stepper, then the steepest-descent restart reads G with -alpha)
    c->carry.cg_have_history = false;
    c->carry.cg_iter_count = 0;
    c->carry.pd_neg_pg = false;
    c->carry.dir_implicit = true;
  } else {
    c->carry.dir_implicit = false;
  }
  c->carry.dir_unwritten = false;  // (kinds 1, 2: D is not read; kind 3: the pass stored it)
  const int parity = c->next_parity;
  c->next_parity ^= 1;
  ah.parity = parity;
  // (host-side right-hand sides are not known yet: the device forms them; the consuming step replays them)
  int rc = queue_round(c, sp, ah.plan, parity, 0.0, 0.0, /*merged=*/true, src, carry_mode, cg, restart);
  c->carry = s_carry;
  if (rc) return rc;
  ah.valid = true;
  ++c->q_ahead;
  return MS_OK;
}
}  // namespace

int ms_step(ms_ctx* c, const ms_stepper_params* sp, double step_size, double tol,
            ms_step_result* out) {
  if (!c || !sp || !out) return fail(c, MS_ERR_INVALID, "ms_step: NULL argument");
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_step: sharded contexts use the phase API");
  memset(out, 0, sizeof(*out));
  c->trial_log.clear();  // (ms_search_trials: this call's trials)
  c->trial_log_cap = (size_t)(sp->max_iter > 0 ? sp->max_iter : 10);
  const bool cg = sp->stepper == MS_STEPPER_CG;
  const int restart = sp->restart_interval > 0 ? sp->restart_interval : 10;
  // conjugate_gradient.py:78-82: steepest descent on first call and every restart
  const bool use_history = cg && c->carry.cg_have_history && (c->carry.cg_iter_count % restart != 0);
  const bool tilt = (c->params.modules & MS_ANY_TILT_MODS) != 0;
  TiltField* tfl[3];
  const int n_tf = active_fields(c, c->params.modules, tfl);
  // A rim source in follow mode takes its center from x when this step's energy pass at x runs, and the trials reuse it
  // (tilt_rim_source_in.py:318 reads the mesh, not the trial positions: without an enforcer the mesh stays at x through
  // the search).  With an enforcer the reference moves the mesh to every trial: that lane is not built.
  // the enforce-only constraints (ms_api_enforce.inc): a flag without its setter is an error, as enforce_area's is
  if (sp->enforce_fixed_plane != 0 && !fplane_set(c))
    return fail(c, MS_ERR_STATE, "ms_stepper_params.enforce_fixed_plane without a plane (ms_set_fixed_plane)");
  if (sp->enforce_perimeter != 0 && !perimeter_set(c))
    return fail(c, MS_ERR_STATE, "ms_stepper_params.enforce_perimeter without loops (ms_set_perimeter)");
  if (sp->enforce_perimeter != 0 && (tilt || tbb_active(c)))
    return fail(c, MS_ERR_STATE, "perimeter together with tilt modules is outside the device path");
  const bool enforce_only = sp->enforce_fixed_plane != 0 || sp->enforce_perimeter != 0;
  for (int k = 0; k < n_tf; ++k)
    if ((c->params.modules & tfl[k]->mod_rs) && tfl[k]->rs_follow && (sp->enforce_volume || sp->enforce_pins || enforce_only))
      return fail(c, MS_ERR_STATE, "tilt_rim_source in follow mode (pin_to_circle_mode: fit) with a constraint enforcer "
                                   "on the line search is outside the device path");
  if ((c->params.modules & MS_MOD_TILT_RIM_SOURCE_BILAYER) && c->rb_follow && (sp->enforce_volume || sp->enforce_pins || enforce_only))
    return fail(c, MS_ERR_STATE, "tilt_rim_source_bilayer in follow mode (pin_to_circle_mode: fit) with a constraint "
                                 "enforcer on the line search is outside the device path");
  // (no reference fixture for the enforcers next to the splay / twist term yet)
  if ((c->params.modules & MS_MOD_TILT_SPLAY_TWIST_IN) && (sp->enforce_volume || (sp->enforce_pins != 0 && pins_set(c))))
    return fail(c, MS_ERR_STATE, "tilt_splay_twist_in together with pin_to_plane / pin_to_circle or the volume enforcer on "
                                 "the line search is outside the device path");
  if ((c->params.modules & MS_MOD_TILT_SPLAY_TWIST_IN) && sp->enforce_fixed_plane != 0)
    return fail(c, MS_ERR_STATE, "tilt_splay_twist_in together with fixed_plane on the line search is outside the device path");
  // (the lane of pins next to a tilt family: a pin program or a fixed plane)
  const bool pin_tilt = ((sp->enforce_pins != 0 && pins_set(c)) || sp->enforce_fixed_plane != 0) && tilt;
  if (pin_tilt && ((c->params.modules & MS_CON_VOLUME) || sp->enforce_volume))
    return fail(c, MS_ERR_STATE, "pin_to_plane / pin_to_circle / fixed_plane next to tilt modules together with the volume "
                                 "constraint are outside the device path");
  // the area lane (ms_api_area_con.inc): the row is projected out behind the gradient pass, the enforcer runs behind the
  // pins' and the volume's on every trial; what has no reference fixture next to it is refused
  const bool area_lane = area_row_active(c) || sp->enforce_area != 0;
  if (sp->enforce_area != 0 && !area_con_set(c))
    return fail(c, MS_ERR_STATE, "ms_stepper_params.enforce_area without an area constraint (ms_set_area_constraint)");
  if (area_lane && tilt)
    return fail(c, MS_ERR_STATE, "the body_area / global_area constraints together with a tilt-family module are outside the device path");
  if (area_lane && pins_set(c))
    return fail(c, MS_ERR_STATE, "the body_area / global_area constraints next to pin_to_plane / pin_to_circle are outside the device path");
  if (area_lane && (c->params.modules & MS_MOD_AREA_PENALTY))
    return fail(c, MS_ERR_STATE, "the body_area / global_area constraints together with body_area_penalty are outside the device path");
  // reuse_energy0 == 2: an accepted trial doubles as the next step's energy/factor pass
  const bool carry_mode = sp->reuse_energy0 >= 2 && !tilt;
  if (c->ahead.valid && !c->ahead.go_known && !(c->carry.kc_pending && carry_mode && c->carry.carry_valid)) {
    // a round was queued ahead, and this step will not read the direction fold that decides about it (something
    // touched the context in between): whatever it did, none of it is used
    drop_ahead(c, /*ran=*/2);
  }
  // the mailbox energies (and G, when grad_valid) describe x ...
  const bool carried_x = carry_mode && c->carry.carry_valid;
  // ... and so do the bending factors in fK / fA (what a gradient pass at x needs)
  const bool carried = carried_x &&
                       (c->carry.factors_valid || !(c->params.modules & (MS_MOD_BENDING | MS_MOD_BENDING_TILT)));
  // the direction cannot ride in the gradient kernel's epilogue when a constraint row has to be projected out first
  // (lambda needs a global reduction) or when a tilt module adds its shape gradient behind K_C
  const bool volrow = (c->params.modules & MS_CON_VOLUME) != 0;
  // conjugate_gradient.py:74-76: the direction comes from the row-normalised gradient -- never an implicit -G, never
  // the fused epilogue, and no queued rounds (their gradient pass carries the fused epilogue)
  const bool precond = cg && sp->precondition != 0;
  c->precond = precond;
  int rc;
  bool restart_sd = false;
  const bool tilt_shape = (c->params.modules & MS_TILT_SHAPE_MODS) != 0;
  if (carried_x && c->carry.grad_valid && !tilt_shape && c->til.T <= 256 &&
      (!volrow || (!use_history && c->carry.maxg2_valid && !precond))) {
    // x has not moved since the last gradient pass (failed search, stepper reset): only the
    // direction changes.  k_direction on the finalized g repeats the fused epilogue's
    // arithmetic and reduction order exactly.  (With a constraint row G is the projected gradient the direction
    // kernel wrote back: a steepest-descent restart reads it as it is; projecting it a second time is not on.)
    restart_sd = !use_history && c->carry.maxg2_valid && !precond;
    if (restart_sd) {
      // steepest-descent restart: d = -g, whose scalars the gradient pass already reduced
      // (|g|^2; <g,d> = -|g|^2 and max|d_i|^2 = max|g_i|^2 exactly) -- no fold, no host round trip
      // -- and no kernel either: the trial passes read G with -alpha (dir_implicit)
      c->carry.dir_implicit = true;
      c->carry.dir_unwritten = false;
      c->carry.last_g = c->buf[MS_BUF_G];
      c->h_scal[MS_S_GDOTD] = -c->h_scal[MS_S_GNORM2];
      c->h_scal[MS_S_MAXD2] = c->h_scal[MS_S_MAXG2];
      rc = MS_OK;
    } else {
      rc = phase_direction(c, sp->stepper, use_history, /*g_finalized=*/true);
    }
  } else if (c->carry.kc_pending && carried_x && !(c->params.modules & MS_TILT_SHAPE_MODS) && c->kc_stepper == sp->stepper &&
             c->kc_use_history == use_history && !precond) {
    // (a queued pass always carries the plain fused direction: a caller that switched precondition on between two
    // steps must not adopt it)
    // the gradient + direction pass of this x was queued behind the line search that accepted it (gated on the
    // acceptance) and has run: take its scalars from its mailbox
    c->carry.kc_pending = false;
    double vals[MS_NSCAL];
    if (c->ahead.valid && !c->ahead.go_known && c->ahead.src == c->carry.kc_parity) {
      // The direction scalars of this pass arrive with the first fold of the round that was queued behind it (its
      // energy launch did not wait for them).  That fold decided first whether the round's search happens at all:
      // replay that from the scalars it was taken on (comparisons only -- the host's outcome is the device's, or
      // the queue is broken).
      ms_ctx::Ahead& ah = c->ahead;
      uint32_t code = DEC_NONE;
      rc = wait_mailbox(c, c->first_mb[ah.parity].h_seq, c->first_mb[ah.parity].expected, vals, &code);
      if (rc) return rc;
      ah.go_known = true;
      {
        const double gn2 = vals[MS_S_GNORM2], gdd = vals[MS_S_GDOTD];
        const bool kind_ok = ah.kind == 1 ? gdd >= 0.0 : gdd < 0.0;
        const bool go = kind_ok && gn2 > ah.tol2p && (ah.kind == 1 ? vals[MS_S_MAXG2] : vals[MS_S_MAXD2]) < ah.lim;
        if (go != (code != DEC_STOP)) {
          rc = verify_decision(c, go ? DEC_GO : DEC_STOP, code, "the fold that opens a round queued ahead");
          if (rc) return rc;
        }
        ah.go = go;
      }
      // its energy launch has run in any case: without the search, the factors and the trial positions are scrap
      if (!ah.go) drop_ahead(c, /*ran=*/1);
    } else {
      rc = flush_dir_fold(c, c->carry.kc_parity);  // (nobody merged the direction fold: launch it now)
      if (rc) return rc;
      rc = wait_mailbox(c, c->grad_mb[c->carry.kc_parity].h_seq, c->grad_mb[c->carry.kc_parity].expected, vals, nullptr);
      if (rc) return rc;
    }
    for (int sl = 0; sl < MS_NSCAL; ++sl)
      if (MASK_DIR & (1u << sl)) put_mailbox(c, sl, vals[sl]);
    c->carry.last_g = c->buf[MS_BUF_G];
    c->carry.dir_implicit = false;
    c->carry.dir_unwritten = c->kc_dir_unwritten[c->carry.kc_parity];  // (as the queued pass left D)
    c->carry.maxg2_valid = true;  // (the fused epilogue and the direction kernel both reduce max|g_i|^2)
  } else {
    c->carry.kc_pending = false;
    rc = queue_energy_and_gradient(c, sp->stepper, use_history, carried);
    c->carry.maxg2_valid = true;  // the fused epilogue / the direction kernel reduced max|g_i|^2 as well
    // (the edge modules: never the kernel-free steepest-descent restart -- the direction kernel runs again on the completed G)
    if (c->params.modules & MS_EDGE_MODS) c->carry.maxg2_valid = false;
  }
  if (rc) return rc;
  if (!restart_sd) {
    rc = fetch(c);
    if (rc) return rc;
  }
  if (c->carry.dir_unwritten) ++c->dir_skipped;  // (this step's gradient pass, queued or direct, left D to k_direction)
  // factors, mailbox energies and G now describe x (until a trial pass overwrites them)
  c->carry.carry_valid = carry_mode;
  c->carry.grad_valid = carry_mode && !tilt_shape;
  double e[4];
  energies_from_mailbox(c, e);
  const double E_eval = e[0] + e[1] + e[2] + e[3];
  const double grad_norm = std::sqrt(c->h_scal[MS_S_GNORM2]);
  const double g_dot_d = c->h_scal[MS_S_GDOTD];
  const double max_dir = std::sqrt(c->h_scal[MS_S_MAXD2]);
  out->energy_eval = E_eval;
  out->grad_norm = grad_norm;
  out->g_dot_d = g_dot_d;
  out->volume = c->h_scal[MS_S_VOL];
  out->next_step = step_size;
  out->energy = E_eval;
  if (use_history) c->last_hist_descent = g_dot_d < 0.0;  // (what queue_ahead expects of the next direction with history)
  if (grad_norm < tol) {  // minimizer.py:1324
    out->converged = 1;
    out->success = 1;
    return MS_OK;
  }
  // ---- backtracking_line_search_array (line_search.py:267-426) -------------
  double energy0 = E_eval;
  double min_edge = std::sqrt(c->h_scal[MS_S_MINEDGE2]);
  // energy_fn projects the stored tilts first (minimizer.py:581-588).  With leaflet bending_tilt the energy pass below
  // launches the normals of x anyway: the projections ride in that launch (same normals, same arithmetic)
  // (not next to pins: there the projection at x is what a rejected search must leave behind bit for bit, and it is
  // taken by the kernel that projects every trial and that ms_project_tilts_to_tangent launches)
  const bool proj_in_normals = tilt && (c->params.modules & MS_LEAFLET_BT) != 0 && !(c->params.modules & MS_TILT_MODS) && !pin_tilt;
  for (int k = 0; k < n_tf && !proj_in_normals; ++k) {
    rc = tilt_pass_f(c, *tfl[k], 2, false, 0.0);
    if (rc) return rc;
  }
  if (!sp->reuse_energy0 || tilt) {
    StageCtl st;
    st.proj_at_x_in_normals = proj_in_normals;
    // (reuse levels 1, 2: the surface / bending / volume terms and the bending_tilt records of THIS x were evaluated by
    // the gradient assembly above; level 0 re-runs every pass the reference re-runs)
    st.energy_tilt_only = tilt && sp->reuse_energy0 >= 1 && c->tenergy_enable &&
                          (c->carry.bt_valid || !(c->params.modules & (MS_MOD_BENDING_TILT | MS_LEAFLET_BT)));
    {
      StageScope scope(c, st);
      rc = phase_energy(c, c->params.modules, false, 0.0, false, false, false);
    }
    if (rc) return rc;
    rc = fetch(c);
    if (rc) return rc;
    energies_from_mailbox(c, e);
    energy0 = e[0] + e[1] + e[2] + e[3];
    min_edge = std::sqrt(c->h_scal[MS_S_MINEDGE2]);
  }
  if (c->til.nf == 0) min_edge = 0.0;
  out->energy = energy0;
  const double safe_step_limit = min_edge > 0.0 ? 0.3 * min_edge : INFINITY;
  if (g_dot_d >= 0.0) return MS_OK;  // :325-328 non-descent: (False, step_size, energy0)
  // a descent direction after all, and the gradient pass did not store it (it expected the line above to return):
  // k_direction writes it from G / PG / PD before the first trial launch reads D
  rc = materialize_direction(c);
  if (rc) return rc;
  double alpha = step_size;
  if (sp->edge_fraction > 0.0 && min_edge > 0.0 && max_dir > 0.0)
    alpha = std::min(alpha, sp->edge_fraction * min_edge / max_dir);
  const double alpha_max = sp->alpha_max_factor * step_size;
  const int max_iter = sp->max_iter > 0 ? sp->max_iter : 10;
  bool kc_queued = false;  // the next step's gradient pass is in the queue, gated on an acceptance
  double min_rejected = INFINITY;  // smallest alpha this search has rejected
  double a_hi, r_lo;
  ms_ctx::LsHist& lh = c->ls[use_history ? 1 : 0];
  ls_bounds(lh, a_hi, r_lo);
  const bool ls_warm = lh.n >= 2;
  // what an accepted trial at `alpha` does (positions, carry flags, CG history, result fields)
  auto accept = [&](double alpha_acc, double E_t) {
    std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
    // carry mode: the trial pass evaluated exactly the accepted x (it wrote those very
    // doubles to xt) with the factor outputs on -> it IS the next step's energy pass
    c->carry.factors_valid = carry_mode;
    c->carry.carry_valid = carry_mode;
    c->carry.grad_valid = false;
    // minimizer.py:1415 re-projects the stored tilts onto the accepted surface: that is
    // exactly the trial projection computed above
    for (int k = 0; k < n_tf; ++k) std::swap(tfl[k]->tilts, tfl[k]->trial);
    c->carry.bt_valid = (c->params.modules & MS_MOD_BENDING_TILT) != 0;  // the trial's record is x's now
    if (cg) {  // conjugate_gradient.py:114-117 history on success only
      std::swap(c->buf[MS_BUF_G], c->buf[MS_BUF_PG]);
      std::swap(c->buf[MS_BUF_D], c->buf[MS_BUF_PD]);
      c->carry.pd_neg_pg = c->carry.dir_implicit;  // the accepted direction was -G = -PG from now on
      c->carry.last_g = c->buf[MS_BUF_PG];
      c->carry.cg_have_history = true;
      ++c->carry.cg_iter_count;
    }
    out->success = 1;
    out->alpha = alpha_acc;
    out->energy = E_t;
    out->volume = c->h_scal[MS_S_VOL];
    out->next_step = std::min(alpha_acc * sp->gamma, alpha_max);
    lh.pred_trials = std::max(1, out->trials);
    // an alpha far below everything accepted lately: the step-size regime has changed, the history predicts nothing
    if (c->ls_reset && lh.n > 0 && alpha_acc < 0.5 * a_hi) lh.n = 0;
    lh.acc[lh.n % ms_ctx::LS_HIST] = alpha_acc;
    lh.rej[lh.n % ms_ctx::LS_HIST] = min_rejected;
    ++lh.n;
    c->carry.kc_pending = kc_queued;
  };
  // the queue needs: carry mode (a trial is a complete energy pass), energies the device can add up the way the
  // host does (surface + bending only), no tilt projections between trials.  The gradient + direction pass of the
  // accepted point follows in the same queue, gated on the acceptance (with a constraint row: K_C, the fold of
  // <g,gC> / <gC,gC>, the direction kernel and its fold, all four behind the same decision word).
  // the enforcer lane (ms_stepper_params.enforce_volume): every trial is projected onto the target volume before its
  // energy is taken -- three more passes per trial, one trial at a time
  // pins (ms_stepper_params.enforce_pins): the pin program on every trial first, then the volume projection if that
  // is on as well (constraint_manager.enforce_all runs the modules in their order; the pins are listed first)
  // pins next to a tilt family (single field or leaflets): per trial the positions (and the guard) alone, the pin
  // program on them, the stored tilts projected onto the ENFORCED surface, the energy passes there; a rejected trial
  // puts the tilts back as well (line_search.py:475-481: needs_tilt_restore is on whenever there is an enforcer)
  const bool enforce_vol = sp->enforce_volume != 0 && volrow && !tilt;
  const bool enforce_pin = sp->enforce_pins != 0 && pins_set(c);
  const bool enforce_tilt = pin_tilt;
  // (ms_stepper_params.enforce_area: behind both, constraint_manager.enforce_all's order pins -> volume -> area)
  const bool enforce_area = sp->enforce_area != 0;
  // (enforce_fixed_plane / enforce_perimeter: the device's one order is fixed_plane -> pins -> perimeter -> volume -> area,
  // enforce_all's listed order for the lists the reference's decks and parser produce)
  const bool enforce_fplane = sp->enforce_fixed_plane != 0, enforce_perim = sp->enforce_perimeter != 0;
  const bool enforce = enforce_vol || enforce_pin || enforce_area || enforce_only;
  bool tbb_lane = false;  // the tilt constraint's ring is set and the inner leaflet's field is among the active ones
  for (int k = 0; k < n_tf; ++k) tbb_lane = tbb_lane || (tfl[k] == &c->tf[1] && tbb_active(c));
  const bool can_chain = c->speculate && carry_mode && !tilt &&
                         !(c->params.modules & (MS_MOD_VOLUME_PENALTY | MS_MOD_AREA_PENALTY | MS_EDGE_MODS)) && !enforce && !precond &&
                         !area_lane;  // (its kernels are not gated: every Armijo decision of the lane is the host's)
  // a round queued by the step before (while its gradient pass was running): the round of THIS search's first
  // iteration if it was queued for exactly what this step has computed by itself
  bool adopted = false;
  if (c->ahead.valid) {
    const ms_ctx::Ahead& ah = c->ahead;
    const bool same = ah.go && can_chain && ah.stepper == sp->stepper && ah.implicit == c->carry.dir_implicit &&
                      ah.alpha0 == alpha && ah.energy0 == energy0 && ah.beta == sp->beta && ah.c1 == sp->c &&
                      ah.max_iter == max_iter && alpha * max_dir < safe_step_limit;
    if (same) {
      adopted = true;
    } else {
      // its kernels ran for a search that is not this one: the factors, trial positions and device scalars of x are
      // theirs now -- once more from x, without it
      drop_ahead(c, /*ran=*/2);
      return ms_step(c, sp, step_size, tol, out);
    }
  }
  // ms_search_trials: one row per alpha of the ladder (launch: trials of the energy launch that evaluated it)
  auto log_trial = [&](double a, double E_t, double rhs_t, int launch, int slot, int flags) {
    if (c->trial_log.size() < c->trial_log_cap) c->trial_log.push_back({a, E_t, rhs_t, launch, slot, flags});
  };
  int it = 0;
  bool unchained_ran = false;  // a trial went through the context's own mailbox (its scalars replaced x's there)
  const bool s_maxg2_x = c->carry.maxg2_valid;
  while (it < max_iter) {
    const bool safe_small = alpha * max_dir < safe_step_limit;
    kc_queued = false;  // (a gradient pass queued behind an earlier, fully rejected round found its gate closed)
    if (!(can_chain && safe_small)) {
      unchained_ran = true;
      if (enforce_tilt) {
        // the un-enforced trial is never evaluated: the shape kernel with an empty module word leaves x + alpha d in
        // the trial buffer and the guard's partials (StageCtl::positions_only: no energy term, no projection, no tilt
        // pass, nothing the context carries changes); the host waits for the fold only when it has to see the guard
        StageCtl st;
        st.positions_only = true;
        StageScope scope(c, st);
        rc = phase_energy(c, 0u, true, alpha, true, !safe_small, false, /*reduce_now=*/!safe_small);
        if (rc == MS_OK && !safe_small) rc = fetch(c);
      } else {
        rc = phase_energy(c, c->params.modules, true, alpha, true, !safe_small, carry_mode && !enforce);
        if (rc) return rc;
        rc = fetch(c);
      }
      if (rc) return rc;
      if (!safe_small && c->h_scal[MS_S_GUARD] > 0.0) {
        ++out->guard_rejects;
        log_trial(alpha, 0.0, energy0 + sp->c * alpha * g_dot_d, 1, 0, MS_TRIAL_GUARD);
        min_rejected = alpha;
        alpha *= sp->beta;
        ++it;
        if (alpha < 1e-8) break;
        continue;
      }
      if (enforce) {
        // line_search.py:448-452: constraint_enforcer(mesh) on the trial positions, then energy_fn() there.  The
        // projection works on buffer X: the trial takes that place for its duration.
        std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);
        rc = MS_OK;
        if (enforce_only) ++c->enforce_only_trials;
        if (enforce_fplane) rc = fplane_run(c);
        if (rc == MS_OK && enforce_pin) {
          rc = pin_enforce_run(c);
          ++c->pin_trials;
        }
        // (perimeter.enforce_constraint's defaults, which enforce_all never overrides: tol 1e-10, 3 passes)
        if (rc == MS_OK && enforce_perim) rc = perimeter_run(c, 1e-10, 3);
        int vol_iters = 3;
        if (rc == MS_OK && enforce_vol) rc = ms_project_volume_cached(c, c->params.target_volume, 1e-12, 3, 0, &vol_iters, nullptr);
        // (a volume projection that ended on an evaluation leaves Body's cache looking current: ms_project_area_cached)
        if (rc == MS_OK && enforce_area)
          rc = ms_project_area_cached(c, 1e-12, sp->enforce_area_iters > 0 ? sp->enforce_area_iters : 20,
                                      enforce_vol && vol_iters < 3, nullptr, nullptr);
        // energy_fn on the enforced trial projects the stored tilts onto it first (minimizer.py:581-588): into `trial`,
        // which takes the field's place for the evaluation -- the tilts of x stay where they are, bit for bit
        for (int k = 0; k < n_tf && rc == MS_OK && enforce_tilt; ++k)
          rc = tilt_pass_f(c, *tfl[k], 2, false, 0.0, tfl[k]->tilts, tfl[k]->trial);
        // tilt_thetaB_boundary_in behind the pins (minimizer.py:1103-1120, then energy_fn's projection): the directions
        // of the enforced trial, then P(enforce(t)) of the ring rows over what the projection above left there; the
        // tilts of x are read, never written
        if (rc == MS_OK && enforce_tilt && tbb_lane) {
          rc = tbb_geom_run(c, nullptr, false, 0.0, false);
          if (rc == MS_OK) rc = tbb_apply_run(c, 1, c->tf[1].tilts, c->tf[1].trial, true);
        }
        for (int k = 0; k < n_tf && enforce_tilt; ++k) std::swap(tfl[k]->tilts, tfl[k]->trial);
        if (rc == MS_OK) rc = phase_energy(c, c->params.modules, false, 0.0, false, false, carry_mode);
        if (rc == MS_OK) rc = fetch(c);
        for (int k = 0; k < n_tf && enforce_tilt; ++k) std::swap(tfl[k]->tilts, tfl[k]->trial);  // (accept() swaps them in)
        std::swap(c->buf[MS_BUF_X], c->buf[MS_BUF_XT]);  // (the projected trial is the trial buffer again)
        if (rc) return rc;
        if (enforce_tilt) c->carry.bt_valid = false;  // (the bending_tilt records describe the trial until it is accepted)
        if (carry_mode) c->carry.factors_valid = false;  // (they belong to the trial point until it is accepted)
      }
      ++out->trials;
      energies_from_mailbox(c, e);
      const double E_t = e[0] + e[1] + e[2] + e[3];
      log_trial(alpha, E_t, energy0 + sp->c * alpha * g_dot_d, 1, 0, 0);
      if (E_t <= energy0 + sp->c * alpha * g_dot_d) {
        accept(alpha, E_t);
        return MS_OK;
      }
      // a rejected trial restores the positions, not the tilts: energy_fn stored their projection
      // onto the trial surface (line_search.py:456-487 without an enforcer; DESIGN.md section 4)
      // (with an enforcer the tilts go back with the positions, line_search.py:475-481: they were never moved)
      for (int k = 0; k < n_tf && !enforce_tilt; ++k) std::swap(tfl[k]->tilts, tfl[k]->trial);
      min_rejected = alpha;
      alpha *= sp->beta;
      ++it;
      if (alpha < 1e-8) break;
      continue;
    }
    rc = spec_prepare(c);
    if (rc) return rc;
    RoundPlan plan;
    int parity;
    if (adopted) {
      plan = c->ahead.plan;
      parity = c->ahead.parity;
      c->ahead.valid = false;
      adopted = false;
      kc_queued = true;  // (queue_round queued it with the round)
      c->kc_stepper = sp->stepper;
      c->kc_use_history = next_use_history(c, cg, restart);
      ++c->q_adopted;
    } else {
      plan_round(c, sp, alpha, max_iter - it, out->trials + out->guard_rejects, a_hi, r_lo, ls_warm, lh.pred_trials,
                 out->trials, plan);
      parity = c->next_parity;
      c->next_parity ^= 1;
      rc = queue_round(c, sp, plan, parity, energy0, g_dot_d, /*merged=*/false, 0, carry_mode, cg, restart);
      if (rc) return rc;
      kc_queued = true;
      c->kc_stepper = sp->stepper;
      c->kc_use_history = next_use_history(c, cg, restart);
    }
    c->carry.kc_parity = parity;
    const int n0 = plan.n0, n_st = plan.n_st, n_round = n0 + n_st;
    const double* const alphas = plan.alphas;
    double rhs[MS_MAX_TRIALS + ms_ctx::SPEC_STAGES];
    for (int j = 0; j < n_round; ++j) rhs[j] = energy0 + sp->c * alphas[j] * g_dot_d;
    ++c->q_rounds;
    ++c->first_launch_hist[n0 - 1];
    // ---- take the results in order, replaying the device's decisions from the same doubles --------------------
    // first launch: every set was folded by ONE k_reduce launch, so they land together
    double v[MS_MAX_TRIALS][MS_NSCAL];
    uint32_t dev_code = DEC_NONE;
    for (int j = 0; j + 1 < n0; ++j) {
      rc = wait_mailbox(c, c->side[j].mb[parity].h_seq, c->side[j].mb[parity].expected, v[j], nullptr);
      if (rc) return rc;
    }
    rc = wait_mailbox(c, c->first_mb[parity].h_seq, c->first_mb[parity].expected, v[n0 - 1], &dev_code);
    if (rc) return rc;
    int acc = -1;
    double E_acc = 0.0;
    for (int j = 0; j < n0 && acc < 0; ++j) {
      ++out->trials;
      const double E_t = stage_energy(c, v[j]);
      log_trial(alphas[j], E_t, rhs[j], n0, j, 0);
      if (E_t <= rhs[j]) {
        acc = j;
        E_acc = E_t;
      } else {
        min_rejected = alphas[j];
      }
    }
    // (the trials of the launch behind its accepted one are not part of the search: evaluated, never looked at)
    for (int j = acc + 1; acc >= 0 && j < n0; ++j) log_trial(alphas[j], stage_energy(c, v[j]), rhs[j], n0, j, MS_TRIAL_BEHIND);
    rc = verify_decision(c, acc < 0 ? DEC_CONTINUE : (acc == n0 - 1 ? DEC_ACCEPT_MAIN : DEC_ACCEPT_SIDE), dev_code,
                         "the first launch of a round");
    if (rc) return rc;
    if (n0 > 1) {
      ++c->q_multi;
      c->q_wasted += acc < 0 ? 0 : n0 - 1 - acc;
    }
    if (acc >= 0)
      for (int s2 = 0; s2 < n_st; ++s2) forget(c->spec[parity][s2]);  // (the gated stages stay out)
    if (acc >= 0 && acc < n0 - 1) {
      // the unexpected case: an early trial was accepted.  The gradient pass queued behind stays out (DEC_ACCEPT_SIDE).
      ++c->q_side_accepts;
      kc_queued = false;
      forget(c->grad_mb[parity]);
      c->dir_pending[parity] = false;
      if (c->pair_lean_enable) {
        // it was evaluated for its energies only -- evaluate it again, alone and with every output.  With fixed-order
        // sums the energies come out bit for bit as before; with LDS atomics in their last bits, like any
        // re-evaluation.
        rc = phase_energy(c, c->params.modules, true, alphas[acc], true, false, carry_mode);
        if (rc) return rc;
        rc = fetch(c);
        if (rc) return rc;
      } else {
        // (MS_PAIR_LEAN=0) this trial's positions and factors are in a side set
        const size_t nvp = (size_t)c->til.nvp;
        const double* sx = acc == 0 ? c->xt2 : c->xt3;
        const double* sk = acc == 0 ? c->fK2 : c->fK3;
        const double* sa = acc == 0 ? c->fA2 : c->fA3;
        HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_XT], sx, sizeof(double) * 3 * nvp, hipMemcpyDeviceToDevice, S(c)));
        HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_FK], sk, sizeof(double) * 3 * nvp, hipMemcpyDeviceToDevice, S(c)));
        HIPCHK(c, hipMemcpyAsync(c->buf[MS_BUF_FA], sa, sizeof(double) * 2 * nvp, hipMemcpyDeviceToDevice, S(c)));
        adopt_scalars(c, v[acc]);
      }
      accept(alphas[acc], E_acc);
      return MS_OK;
    }
    if (acc == n0 - 1) {
      adopt_scalars(c, v[acc]);
      accept(alphas[acc], E_acc);
      if (c->ahead_allowed) {
        rc = queue_ahead(c, sp, out, tol, carry_mode, cg, restart);
        if (rc) return rc;
      }
      return MS_OK;
    }
    // gated stages, in order
    bool accepted = false;
    for (int s2 = 1; s2 <= n_st && !accepted; ++s2) {
      double vals[MS_NSCAL];
      uint32_t code = DEC_NONE;
      rc = wait_mailbox(c, c->spec[parity][s2 - 1].h_seq, c->spec[parity][s2 - 1].expected, vals, &code);
      if (rc) return rc;
      ++out->trials;
      const double E_t = stage_energy(c, vals);
      log_trial(alphas[n0 + s2 - 1], E_t, rhs[n0 + s2 - 1], 1, 0, 0);
      const bool ok = E_t <= rhs[n0 + s2 - 1];
      rc = verify_decision(c, ok ? DEC_ACCEPT_MAIN : DEC_CONTINUE, code, "a gated stage");
      if (rc) return rc;
      if (ok) {  // the device took the same decision from the same doubles: later stages stay out
        for (int s3 = s2; s3 < n_st; ++s3) forget(c->spec[parity][s3]);
        adopt_scalars(c, vals);
        accept(alphas[n0 + s2 - 1], E_t);
        accepted = true;
      } else {
        min_rejected = alphas[n0 + s2 - 1];
      }
    }
    if (accepted) {
      if (c->ahead_allowed) {
        rc = queue_ahead(c, sp, out, tol, carry_mode, cg, restart);
        if (rc) return rc;
      }
      return MS_OK;
    }
    forget(c->grad_mb[parity]);  // every trial of the round was rejected: the gradient pass behind it stayed out
    c->dir_pending[parity] = false;
    it += n_round;
    alpha = alphas[n_round - 1] * sp->beta;
    if (alpha < 1e-8) break;
  }
  const double reduced = std::max(alpha * sp->beta, 0.0);  // :425-426
  out->next_step = std::max(reduced, step_size * sp->beta);
  if (c->ls_reset) lh.n = 0;  // a search that ran out of trials: same
  lh.pred_trials = std::max(1, out->trials + out->guard_rejects);
  if (carry_mode && !unchained_ran) {
    // every trial was rejected and x has not moved: G and the host's scalars still describe x (the queued rounds post
    // to mailboxes of their own); only the bending factors in fK / fA and the device scalars are the last trial's
    c->carry.carry_valid = true;
    c->carry.grad_valid = !tilt_shape;
    c->carry.maxg2_valid = s_maxg2_x;
    c->carry.factors_valid = false;
  }
  return MS_OK;
}

int ms_project_volume_cached(ms_ctx* c, double target, double tol, int max_iter, int first_step_cached,
                             int* iters_out, double* volume_out) {
  if (!c) return MS_ERR_INVALID;
  if (c->shard_count != 1) return fail(c, MS_ERR_STATE, "ms_project_volume: single shard only");
  const size_t row_bytes = sizeof(double) * 3 * (size_t)c->til.nvp;
  if (!c->d_volgrad_cache) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_volgrad_cache), row_bytes));
    HIPCHK(c, hipMemsetAsync(c->d_volgrad_cache, 0, row_bytes, S(c)));
  }
  int it = 0;
  double V = 0.0;
  for (; it < max_iter; ++it) {
    int rc = phase_energy(c, MS_CON_VOLUME, false, 0.0, false, false, false);
    if (rc) return rc;
    rc = fetch(c);
    if (rc) return rc;
    V = c->h_scal[MS_S_VOL];
    const double delta = V - target;
    // compute_volume_and_gradient (body.py:386-470): the gradient comes with the volume -- from Body's cache on the
    // first pass when the caller says the cached volume is current (a compute_volume at this mesh version preceded,
    // which refreshes the cached volume and version but not the gradient), freshly evaluated (and cached) otherwise
    const bool stale = it == 0 && first_step_cached != 0 && c->volgrad_cache_valid;
    const double* g = c->d_volgrad_cache;
    double norm2 = c->volgrad_cache_norm2;
    if (!stale) {
      rc = phase_gradient(c, MS_CON_VOLUME, nullptr, false);
      if (rc) return rc;
      rc = fetch(c);
      if (rc) return rc;
      norm2 = c->h_scal[MS_S_GCGC];
      HIPCHK(c, hipMemcpyAsync(c->d_volgrad_cache, c->buf[MS_BUF_GC], row_bytes, hipMemcpyDeviceToDevice, S(c)));
      c->volgrad_cache_norm2 = norm2;
      c->volgrad_cache_valid = true;
    }
    if (std::fabs(delta) < tol) break;
    const double lam = delta / (norm2 + 1e-12);
    HIPCHK(c, launch_axpy_masked(c->til.nv, c->d_vflags, c->buf[MS_BUF_X], g, -lam, c->stream));
    c->carry.factors_valid = false;
    c->carry.invalidate_with_bt();
  }
  if (iters_out) *iters_out = it;
  if (volume_out) *volume_out = V;
  return MS_OK;
}

int ms_project_volume(ms_ctx* c, double target, double tol, int max_iter, int* iters_out,
                      double* volume_out) {
  return ms_project_volume_cached(c, target, tol, max_iter, 0, iters_out, volume_out);
}

namespace {
constexpr int RES_CHUNK = 4096;  // steps per launch (rows of the device step log)

// can the steps of this ms_minimize call run in the resident kernel?  (surface + volume row, gradient descent, plain
// Armijo search with evaluation reuse; everything else keeps the kernel-per-phase path)
bool resident_eligible(ms_ctx* c, const ms_minimize_params* mp) {
  const uint32_t mods = c->params.modules;
  const ms_stepper_params& sp = mp->stepper;
  if (!c->resident_enable || c->profiling || c->exec_on) return false;
  if (c->shard_count != 1 || c->comm || c->allgather_cb || c->peer_on) return false;
  if (c->til.T != 256 || c->til.own != 256 || !c->d_tile_facets32 || c->til.n_tiles < 2 || c->til.n_tiles > 2048) return false;
  if (!(mods & MS_MOD_SURFACE) || (mods & ~(MS_MOD_SURFACE | MS_CON_VOLUME | MS_TRACK_VOLUME))) return false;
  if (sp.stepper != MS_STEPPER_GD || sp.precondition || sp.enforce_volume || sp.reuse_energy0 < 2 || sp.edge_fraction > 0.0)
    return false;
  if (pins_set(c)) return false;  // (the pin program and the project lane run outside the resident kernel)
  if (area_row_active(c) || sp.enforce_area) return false;  // (so do the area row and its enforcer)
  // (and the enforce-only constraints: inside the kernel their projections would be dropped without a word)
  if (sp.enforce_fixed_plane || sp.enforce_perimeter || fplane_set(c) || perimeter_set(c)) return false;
  if (mp->relax_tilts || mp->fixed_step_mode) return false;
  if (c->resident_ok < 0) {
    c->resident_lds = resident_lds_bytes(c->cap, c->til.max_ent, c->til.max_tile_facets, false);
    int ok = 0;
    if (resident_fits(c->til.n_tiles, c->resident_lds, c->device, &ok) != hipSuccess) {
      (void)hipGetLastError();
      ok = 0;
    }
    c->resident_ok = ok;
    if (trace_steps())
      fprintf(stderr, "[mss] resident step kernel: %d tiles, %zu bytes of LDS per workgroup -> co-resident: %d\n",
              c->til.n_tiles, c->resident_lds, ok);
  }
  return c->resident_ok == 1;
}

struct ResidentOutcome {
  int steps = 0, reason = RES_DONE;
  double step_size = 0.0, energy = 0.0, volume = 0.0;
};

// up to max_steps steps in one launch; the step log rows land in c->h_res_log
int resident_run(ms_ctx* c, const ms_minimize_params* mp, int max_steps, double step_size, ResidentOutcome* ro) {
  const Tiling& t = c->til;
  const ms_stepper_params& sp = mp->stepper;
  const int n = std::min(max_steps, RES_CHUNK);
  if (!c->d_res_partials) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_res_partials), sizeof(double) * 4 * MS_NPART * (size_t)t.n_tiles));
    HIPCHK(c, hipMemset(c->d_res_partials, 0, sizeof(double) * 4 * MS_NPART * (size_t)t.n_tiles));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_res_bar), sizeof(unsigned int) * RESIDENT_BAR_WORDS));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_res_log), sizeof(double) * 8 * RES_CHUNK));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_res_result), sizeof(double) * 16));
  }
  ResidentArgs a;
  a.m = device_mesh(c);
  a.x = c->buf[MS_BUF_X];
  a.d = c->buf[MS_BUF_D];
  a.g = c->buf[MS_BUF_G];
  a.gC = c->buf[MS_BUF_GC];
  a.partials = c->d_res_partials;
  a.bar = c->d_res_bar;
  a.log = c->d_res_log;
  a.result = c->d_res_result;
  a.n_steps = n;
  a.volrow = (c->params.modules & MS_CON_VOLUME) ? 1 : 0;
  a.want_vol = (c->params.modules & (MS_CON_VOLUME | MS_TRACK_VOLUME)) ? 1 : 0;
  a.atomic = c->deterministic ? 0 : 1;
  a.max_iter = sp.max_iter > 0 ? sp.max_iter : 10;
  a.step_size = step_size;
  a.tol = mp->tol;
  a.c1 = sp.c;
  a.beta = sp.beta;
  a.gamma = sp.gamma;
  a.alpha_max_factor = sp.alpha_max_factor;
  a.drift_check = mp->drift_check;
  a.target_volume = mp->target_volume;
  a.volume_tolerance = mp->volume_tolerance;
  a.cap = c->cap;
  a.max_ent = t.max_ent;
  HIPCHK(c, hipMemsetAsync(c->d_res_bar, 0, sizeof(unsigned int) * RESIDENT_BAR_WORDS, S(c)));
  HIPCHK(c, launch_resident(a, c->resident_lds, c->stream));
  double res[16];
  HIPCHK(c, hipMemcpyAsync(res, c->d_res_result, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ro->steps = (int)res[0];
  ro->reason = (int)res[1];
  ro->step_size = res[2];
  ro->energy = res[3];
  ro->volume = res[4];
  ++c->resident_launches;
  c->resident_steps += ro->steps;
  if (trace_steps())
    fprintf(stderr, "[mss] resident launch: asked %d steps from step size %.3e -> took %d, reason %d, %d barriers\n", n,
            step_size, ro->steps, ro->reason, (int)res[7]);
  if (trace_steps() && ro->steps > 0)
    fprintf(stderr, "[mss]   per step (us, workgroup 0): gradient %.2f | barrier %.2f | lambda+rows+direction %.2f | trial energies "
                    "%.2f | barrier %.2f | fold %.2f\n", res[8] / ro->steps, res[9] / ro->steps, res[10] / ro->steps,
            res[11] / ro->steps, res[12] / ro->steps, res[13] / ro->steps);
  if (ro->steps > 0) {
    c->h_res_log.resize((size_t)8 * ro->steps);
    HIPCHK(c, hipMemcpy(c->h_res_log.data(), c->d_res_log, sizeof(double) * 8 * (size_t)ro->steps, hipMemcpyDeviceToHost));
  }
  // x may have moved, and the launch used the G / GC / D buffers for its own (raw) rows even when it declined its first
  // step: nothing the step logic carries from earlier evaluations is valid any more
  c->carry.carry_valid = c->carry.grad_valid = c->carry.factors_valid = c->carry.maxg2_valid = c->carry.bt_valid = false;
  c->carry.kc_pending = false;
  c->carry.dir_implicit = false;
  c->carry.dir_unwritten = false;
  if (ro->reason == RES_TIMEOUT) return fail(c, MS_ERR_STATE, "resident step kernel: a grid barrier timed out");
  return MS_OK;
}
}  // namespace

int ms_minimize(ms_ctx* c, const ms_minimize_params* mp, int n_steps, ms_minimize_result* out,
                double* step_log) {
  if (!c || !mp || !out) return fail(c, MS_ERR_INVALID, "ms_minimize: NULL argument");
  memset(out, 0, sizeof(*out));
  double step_size = mp->step_size;
  int zero_steps = 0;
  out->step_success = 1;
  out->step_size = step_size;
  const bool resident = resident_eligible(c, mp);
  int resident_cooldown = 0;       // iterations to leave to the ordinary path after the kernel declined a step
  bool res_energy_valid = false;   // the last step taken was the resident kernel's: its energy is the current x's
  double res_energy = 0.0;
  for (int i = 0; i < n_steps; ++i) {
    int rc;
    if (resident && resident_cooldown == 0 && n_steps - i >= 2) {
      // ---- as many steps as it will take in ONE launch (ms_resident.inc); bookkeeping per step as below ------------
      drop_ahead(c, /*ran=*/2);
      ResidentOutcome ro;
      rc = resident_run(c, mp, n_steps - i, step_size, &ro);
      if (rc) return rc;
      for (int k = 0; k < ro.steps; ++k) {
        const double* row = c->h_res_log.data() + 8 * (size_t)k;
        out->iterations = i + k + 1;
        out->energy_eval = row[3];
        out->grad_norm = row[4];
        if (step_log) memcpy(step_log + 8 * (size_t)(i + k), row, sizeof(double) * 8);
        out->step_success = 1;
        out->volume_cache_current = mp->drift_check ? 1 : 0;
        out->trials += (int)row[7];
        step_size = row[1];
        ++out->accepted;
        out->moved = 1;
        out->step_size = step_size;
        zero_steps = 0;
      }
      if (ro.steps > 0) {
        res_energy_valid = true;
        res_energy = ro.energy;
      }
      i += ro.steps;
      if (ro.reason == RES_DRIFT) {  // :1478-1513, for the step just taken
        if (mp->project_on_drift) {
          int iters = 0;
          rc = pin_enforce_run(c);  // enforce_all(context="mesh_operation"): the pins, then the volume
          if (rc) return rc;
          rc = ms_project_volume_cached(c, mp->target_volume, 1e-12, 12, 1, &iters, nullptr);
          if (rc) return rc;
          out->volume_cache_current = 0;
          res_energy_valid = false;
        }
        ms_reset_stepper(c);
      } else if (ro.reason != RES_DONE) {
        // convergence, guard range, an exhausted search, a non-descent direction: this iteration through the ordinary
        // path (x is as the last completed step left it), and a few more before the kernel is asked again
        resident_cooldown = ro.reason == RES_CONVERGED ? 0 : 8;
        ++c->resident_bails;
      }
      if (i >= n_steps) break;
      if (ro.reason == RES_DONE || ro.reason == RES_DRIFT) {
        --i;  // (the loop increment: the next iteration is i)
        continue;
      }
    } else if (resident_cooldown > 0) {
      --resident_cooldown;
    }
    res_energy_valid = false;
    if (mp->relax_tilts) {  // minimizer.py:1237-1307: before the convergence check
      rc = (c->params.modules & MS_LEAFLET_MODS) ? ms_relax_leaflet_tilts(c, &mp->relax, nullptr, nullptr)
                                                  : ms_relax_tilts(c, &mp->relax, nullptr, nullptr);
      if (rc) return rc;
      out->moved = 1;
    }
    const double step_in = mp->fixed_step_mode ? mp->fixed_step : step_size;
    ms_step_result r;
    // rounds may be queued ahead of the step they belong to while this loop is the only thing touching the context
    c->steps_left = n_steps - 1 - i;
    c->ahead_allowed = c->ahead_enable && i + 1 < n_steps && !mp->relax_tilts && !mp->fixed_step_mode &&
                       c->shard_count == 1 && !c->comm && !c->allgather_cb && !c->peer_on;
    rc = (c->shard_count > 1 || c->comm || c->allgather_cb || c->peer_on) ? ms_shard_step(c, &mp->stepper, step_in, mp->tol, &r)
                                                            : ms_step(c, &mp->stepper, step_in, mp->tol, &r);
    c->ahead_allowed = false;
    if (rc) return rc;
    if (trace_steps()) {
      static double t_prev = 0.0;
      struct timespec ts;
      clock_gettime(CLOCK_MONOTONIC, &ts);
      const double t_now = 1e6 * (double)ts.tv_sec + 1e-3 * (double)ts.tv_nsec;
      fprintf(stderr, "[mss] %3d ok %d trials %2d alpha %.3e g.d %+.2e  %7.0f us  rounds %lld multi %lld wasted %lld side %lld ahead %lld adopted %lld dropped %lld\n",
              i, r.success, r.trials, r.alpha, r.g_dot_d, t_prev > 0.0 ? t_now - t_prev : 0.0, (long long)c->q_rounds,
              (long long)c->q_multi, (long long)c->q_wasted, (long long)c->q_side_accepts, (long long)c->q_ahead,
              (long long)c->q_adopted, (long long)c->q_dropped);
      t_prev = t_now;
    }
    out->iterations = i + 1;
    out->energy_eval = r.energy_eval;
    out->grad_norm = r.grad_norm;
    if (step_log) {
      double* row = step_log + 8 * (size_t)i;
      row[0] = r.success;
      row[1] = r.next_step;
      row[2] = r.energy;
      row[3] = r.energy_eval;
      row[4] = r.grad_norm;
      row[5] = r.g_dot_d;
      row[6] = r.alpha;
      row[7] = r.trials;
    }
    if (r.converged) {  // :1324-1337
      out->converged = 1;
      out->step_success = 1;
      out->step_size = step_size;
      drop_ahead(c, /*ran=*/2);
      return MS_OK;
    }
    out->step_success = r.success;
    out->volume_cache_current = 0;  // minimizer.py:1415-1416: project_tilts_to_tangent + increment_version
    out->trials += r.trials;
    out->guard_rejects += r.guard_rejects;
    step_size = r.next_step;
    if (r.success) {
      ++out->accepted;
      out->moved = 1;
    }
    if (mp->fixed_step_mode) step_size = mp->fixed_step;
    out->step_size = step_size;
    if (!r.success) {  // :1425-1476
      if (step_size <= mp->step_size_floor) {
        if (++zero_steps >= mp->max_zero_steps) {
          out->zero_step_exit = 1;
          drop_ahead(c, /*ran=*/2);
          return MS_OK;
        }
      } else {
        zero_steps = 0;
      }
      ms_reset_stepper(c);
    } else {
      zero_steps = 0;
      if (mp->drift_check) {  // :1478-1513
        out->volume_cache_current = 1;  // body.compute_volume: Body's cached volume is current again
        const double denom = std::max(std::fabs(mp->target_volume), 1.0);
        if (std::fabs(r.volume - mp->target_volume) / denom > mp->volume_tolerance) {
          if (mp->project_on_drift) {
            int iters = 0;
            drop_ahead(c, /*ran=*/2);  // (the projection moves x: a round queued for the next step is void)
            // enforce_all(context="mesh_operation"): fixed_plane, the pins, perimeter, then the volume
            if (mp->stepper.enforce_fixed_plane) {
              rc = fplane_run(c);
              if (rc) return rc;
            }
            rc = pin_enforce_run(c);
            if (rc) return rc;
            if (mp->stepper.enforce_perimeter) {
              rc = perimeter_run(c, 1e-10, 3);
              if (rc) return rc;
            }
            rc = ms_project_volume_cached(c, mp->target_volume, 1e-12, 12, 1, &iters, nullptr);
            if (rc) return rc;
            if (mp->stepper.enforce_area) {  // (body_area / global_area: listed behind volume)
              rc = ms_project_area_cached(c, 1e-12, mp->stepper.enforce_area_iters > 0 ? mp->stepper.enforce_area_iters : 20,
                                          iters < 12, nullptr, nullptr);
              if (rc) return rc;
            }
            out->volume_cache_current = 0;  // enforce_constraints_after_mesh_ops bumps the mesh version
            // minimizer.py:1505-1507: enforce, then mesh.project_tilts_to_tangent() on the projected surface
            if (c->params.modules & MS_ANY_TILT_MODS) {
              rc = ms_project_tilts_to_tangent(c);
              if (rc) return rc;
            }
          }
          ms_reset_stepper(c);
        }
      }
    }
  }
  drop_ahead(c, /*ran=*/2);
  if (res_energy_valid) {  // (surface energy of the x the resident kernel ended at: the accepted trial's)
    out->energy_current = res_energy;
    out->energy_current_valid = 1;
  } else if (c->carry.carry_valid && !(c->params.modules & MS_ANY_TILT_MODS)) {
    // the mailbox energies describe the positions the loop ended at: the caller's final energy needs no pass
    double e[4];
    energies_from_mailbox(c, e);
    out->energy_current = e[0] + e[1] + e[2] + e[3];
    out->energy_current_valid = 1;
  }
  return MS_OK;
}
