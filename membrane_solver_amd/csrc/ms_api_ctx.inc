// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): the context: everything a ms_ctx holds.
// What describes the launch or fold being queued: the launchers (phase_energy, phase_gradient, phase_direction,
// reduce_slots) read it through ms_ctx::stage(); only a StageScope changes it.  Default: an ungated single-trial launch,
// parity 0, nothing deferred.
struct StageCtl {
  const uint32_t* cur_gate = nullptr;  // decision word the launches being queued test (nullptr: unconditional)
  uint32_t cur_gate_want = 0;
  bool cur_gate_fold_only = false;        // the gate (and the ran check) belongs to the fold, not to the energy kernel
  bool cur_check_ran = false;          // the tile kernel in front of the fold being queued is gated by cur_gate
  uint32_t* cur_dec = nullptr;         // the fold being queued closes a stage: its decision goes here
  double cur_rhs[MS_MAX_TRIALS] = {0}; // ... taken against these Armijo right-hand sides (trial order)
  const double* cur_rhs_dev = nullptr; // the fold being queued takes its right-hand sides from the device
  uint32_t cur_extra_mask = 0;            // reduce_slots: fold these slots of the ordinary partials as well
  int cur_go_kind = 0;                    // ... and take the GO decision first (FoldArgs::go_kind and its parameters)
  uint32_t* cur_go = nullptr;          // the direction fold being queued may open the next round: its GO word
  double cur_go_val[6] = {0};             // tol^2 (1+1e-9), guard bound, energy0, c, alpha_0, beta
  int cur_parity = 0;            // which of a side set's two mailboxes the early trials of a multi-trial fold post to
  int pair_on = 0;               // phase_energy / reduce_slots: the launch being queued evaluates this many trials
  // the early trials of a multi-trial launch (the ones expected to fail) are evaluated for their energies only:
  // no trial positions, no bending factors written for them (ms_step; the sharded driver needs the factor rows)
  bool pair_lean = false;
  double pair_alpha[MS_MAX_TRIALS] = {0};  // alphas of the early trials
  double* pair_scal2 = nullptr;    // where a pair launch's second fold goes (nullptr: d_scal2)
  bool multi_any_slot = false;   // reduce_slots: a multi-trial fold of ANY slot mask (the tilt search pass), not only the core energies
  bool defer_dir = false;                 // reduce_slots: do not launch a direction fold, remember its mask
  // phase_energy at x right behind an evaluation of the same x (ms_step's energy0 with tilt modules: only the tilts were
  // re-projected in between): the shape kernels are not launched again -- their energies are in the mailbox, the
  // bending_tilt records in place -- only the tilt modules' passes run and only their slots are folded
  bool energy_tilt_only = false;
  bool positions_only = false;  // phase_energy: the launch is wanted for x + alpha d and the guard alone (ms_step, pins next to tilt modules): no module is evaluated, and what the context remembers of its factor buffers stays
  bool proj_at_x_in_normals = false;  // phase_energy: the normals launch also projects the leaflets' stored tilts onto x in place (ms_step)
};
// What the step logic carries from one evaluation to the next.  "Queue something in the state a later step will be in"
// copies it out, changes it, queues, and copies it back whole.
struct CarryState {
  // steepest-descent restart on an unchanged gradient (ms_step): the direction is -G and is not written out;
  // trial passes then read G with -alpha (bitwise the same x + alpha d).  After such a step is accepted the
  // CG history's previous direction is -PG, which the next fused direction pass derives instead of loading.
  bool dir_implicit = false;
  // the last fused direction pass (CG history) formed its rows for the scalars only and did not store them: the host
  // expected <g,d> >= 0, after which nobody reads D.  Whoever does want D first has k_direction write it from the
  // stored G / PG / PD (materialize_direction); a stepper reset or a new gradient pass clears the flag.
  bool dir_unwritten = false;
  bool pd_neg_pg = false;
  bool kc_pending = false;       // the gradient pass queued behind a round ran for the accepted x: the next ms_step takes its result
  int kc_parity = 0;
  bool bt_valid = false;          // d_bt_vert describes the current x
  double* last_g = nullptr;   // buffer holding the most recent finalized gradient
  bool cg_have_history = false;
  int cg_iter_count = 0;
  bool factors_valid = false;
  // true while the mailbox energies / min edge / volume AND the factor buffers describe the
  // current x: set when ms_step accepts a trial that also wrote the factors, cleared by
  // every other energy pass and by every mutator
  bool carry_valid = false;
  // true while buffer G holds the finalized gradient of the current x (set by ms_step's fused
  // gradient pass, survives a failed line search, cleared together with carry_valid)
  bool grad_valid = false;
  bool maxg2_valid = false;  // the mailbox holds |g|^2 and max|g_i|^2 of the gradient in buffer G
  // a mutator's part: the energies, the gradient and its reductions held describe what was there before ...
  void invalidate() { carry_valid = grad_valid = maxg2_valid = false; }
  // ... and, where positions or tilts moved, so does d_bt_vert
  void invalidate_with_bt() { carry_valid = grad_valid = bt_valid = maxg2_valid = false; }
};
struct ms_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Tiling til;
  int shard_rank = 0, shard_count = 1;
  int tile0 = 0, tile1 = 0;
  int cap = 0;
  // connectivity in HBM
  int32_t* d_perm = nullptr;
  int32_t* d_tile_facet_off = nullptr;
  TileFacet* d_tile_facets = nullptr;
  uint32_t* d_tile_facets32 = nullptr;  // packed copy (DeviceMesh::tile_facets32), or nullptr
  uint32_t* d_tile_facets_lean = nullptr;  // packed Tiling::tile_facets_lean (the lean k_energy instances' lane order), or nullptr
  bool lane_order_on = false;           // they read it (MS_LANE_ORDER=0 at ms_create: they read the common array)
  double* d_tf_gamma = nullptr;
  // Body's cached volume gradient (geometry/body.py:386-407): what the last fresh evaluation inside
  // ms_project_volume computed, and its squared norm
  double* d_volgrad_cache = nullptr;
  double volgrad_cache_norm2 = 0.0;
  bool volgrad_cache_valid = false;
  bool gamma_uniform = true, kc_uniform = true;  // ms_set_surface_tension / ms_set_bending_params decide
  double gamma_const = 1.0, kappa_const = 0.0, c0_const = 0.0;
  int32_t* d_tile_halo_off = nullptr;
  int32_t* d_halo_ids = nullptr;
  int32_t* d_tile_ent_off = nullptr;
  uint16_t* d_tile_voff = nullptr;
  uint16_t* d_vent = nullptr;
  uint8_t* d_vflags = nullptr;
  double* d_kappa = nullptr;
  double* d_c0 = nullptr;
  // vertex tilt fields: [0] the single field (ms_set_tilts), [1]/[2] inner / outer leaflet
  // (ms_set_leaflet_tilts).  All arrays (nvp,3) in patch order.
  struct TiltField {
    double* tilts = nullptr;   // current tangent tilts
    double* trial = nullptr;   // tilts projected onto a trial surface / relaxation trial
    double* grad = nullptr;    // dE/dt of the last tilt-gradient evaluation
    double* dir = nullptr;     // relaxation: CG direction
    double* minv = nullptr;    // relaxation: Jacobi M^-1 (nvp)
    double k_tilt = 0.0;       // tilt modulus (0 = magnitude module contributes nothing)
    int consistent = 0;        // tilt_mass_mode: consistent P1 mass instead of lumped
    double k_smooth = 0.0;     // smoothness rigidity of the energy
    double k_smooth_precond = 0.0;  // rigidity entering the Jacobi diagonal
    uint8_t fixed_bit = 0;     // vertex flag bit that clamps a row of this field
    uint8_t absent_bit = 0;    // vertex flag bit of the rows this leaflet is absent on; 0 while no row carries it
                               // (ms_set_leaflet_absent)
    uint32_t mod_tilt = 0, mod_smooth = 0, mod_bt = 0;  // module bits that read this field
    int s_etilt = 0, s_ets = 0, s_gn2 = 0, s_rz = 0, s_ebt = 0;  // reduction slots
    // leaflet bending_tilt: per-vertex (kappa, c0), the per-vertex record of the last energy pass
    // {base, A_eff, kappa*ratio*H, 0} and the sign of the divergence term
    double* kappa = nullptr;
    double* c0 = nullptr;
    double* bt_vert = nullptr;
    double div_sign = 1.0;
    // disk tilt target (tilt_disk_target_in/out): tagged rows, parameters, the difference field
    uint8_t* disk = nullptr;
    double* diff = nullptr;
    double* dt_target = nullptr;   // theta(r) r_hat of the tagged rows on the frozen surface of a running relaxation
    bool dt_target_valid = false;
    ms_disk_target_params dt = {};
    uint32_t mod_dt = 0;
    int s_edt = 0, s_dtr = 0;
    // rim source (tilt_rim_source_in/out, ms_set_leaflet_rim_source): one allocation holds the CSR, the coefficients,
    // the follow mode's center, the per-workgroup sums and the module's energy
    uint32_t mod_rs = 0;
    void* d_rim = nullptr;
    RimArgs rs{};
    bool rs_set = false;
    bool rs_follow = false;
    bool rs_coef_valid = false;    // rs.coef holds c of the frozen surface of a running relaxation
    double* rs_center = nullptr;   // (inside d_rim)
    long rs_launches[3] = {0, 0, 0};  // k_rim_frame, k_rim_coef, k_rim_apply
    // the add-on modules that read this leaflet's field (ms_slot_writers.h: addon_readers; mod_rs among them).
    // rim_slope_match_out reads the inner one only with a disk ring: ms_set_rim_match sets that field's bit only then
    uint32_t mod_addons = 0;
    // every module bit that reads this leaflet field
    uint32_t mods() const { return mod_tilt | mod_smooth | mod_bt | mod_dt | mod_addons; }
    // every module bit whose sums land in this field's tilt-magnitude / smoothness slot: its own module and the
    // add-ons riding there (what the readers of the slot ask)
    uint32_t etilt_mods() const { return mod_tilt | (mod_addons & slot_writers(s_etilt, true)); }
    uint32_t ets_mods() const { return mod_smooth | (mod_addons & slot_writers(s_ets, true)); }
    bool any_free = true;     // some row of this field is not clamped (kept current by the flag setters)
    double* va = nullptr;      // relaxation: barycentric vertex areas of the frozen positions
  } tf[3];
  // tilt_coupling (ms_set_tilt_coupling): modulus, sign (-1 difference / +1 sum / 0 off); d_cpl holds the
  // per-workgroup sums of the last launch (the module's own energy is their sum)
  double cpl_k = 0.0;
  int cpl_sign = 0;
  void* d_cpl = nullptr;
  long cpl_launches[3] = {0, 0, 0};  // k_couple<0>, k_couple<1>, k_couple_vec
  bool cpl_force_tile = false;       // MS_COUPLE_VEC=0: the frozen form through the tile kernel as well (A/B)
  // tilt_rim_source_bilayer (ms_set_rim_source_bilayer): ONE table for both leaflet fields -- the allocation, arguments,
  // followed center and cached coefficients of TiltField::rs, kept per context
  void* d_rimb = nullptr;
  RimArgs rb{};
  bool rb_set = false;
  bool rb_follow = false;
  bool rb_coef_valid = false;    // rb.coef holds c of the frozen surface of a running relaxation
  double* rb_center = nullptr;   // (inside d_rimb)
  long rb_launches[3] = {0, 0, 0};  // k_rim_frame, k_rim_coef, k_rim_apply2
  // tilt_thetaB_contact_in (ms_set_thetab_contact): one allocation holds the per-row table, the record, the scalars, the
  // module's energy and the rows; theta_B is the host's (ms_set_thetab_value) and goes to every apply launch by value
  void* d_tb = nullptr;
  ThetabArgs tb{};
  bool tb_set = false;
  double tb_theta = 0.0;
  bool tb_relax = false;        // a relaxation is running: x is frozen ...
  bool tb_geom_valid = false;   // ... and the table holds its ring (the first evaluation's geometry pass)
  long tb_launches[2] = {0, 0};  // k_thetab_geom, k_thetab_apply
  // rim_slope_match_out (ms_set_rim_match): one allocation holds the three row tables, the tables k_rsm_geom writes, the
  // record and the module's energy.  While a relaxation runs (tb_relax: x is frozen) the first evaluation's geometry
  // pass serves the others
  void* d_rsm = nullptr;
  RsmArgs rsm{};
  bool rsm_set = false;
  bool rsm_geom_valid = false;
  long rsm_launches[2] = {0, 0};  // k_rsm_geom, k_rsm_apply
  // tilt_thetaB_boundary_in (ms_set_thetab_boundary): one allocation holds the per-row table (d, N_v, keep), the rows
  // and the row -> facet CSR; theta_B is tb_theta.  The constraint acts on the inner leaflet's field only.
  void* d_tbb = nullptr;
  TbbArgs tbb{};
  bool tbb_set = false;
  bool tbb_geom_valid = false;   // a relaxation is running (x frozen) and the table holds its directions
  long tbb_launches[3] = {0, 0, 0};  // k_tbb_geom, k_tbb_apply<0/1>, k_tbb_apply<2>
  // tilt_projection_cadence / tilt_projection_interval (ms_set_tilt_projection): when a relaxation re-enforces the tilt
  // constraint after an accepted step
  int tilt_proj_cadence = 0;     // 0 per_step, 1 per_pass
  int tilt_proj_interval = 1;
  // tilt_splay_twist_in (ms_set_tilt_splay_twist): the two moduli; d_st holds the per-workgroup sums of the last launch
  double st_k_splay = 0.0, st_k_twist = 0.0;
  bool st_set = false;
  void* d_st = nullptr;
  long st_launches[2] = {0, 0};  // k_splay<0>, k_splay<1>
  CarryState carry;
  bool precond = false;      // ms_stepper_params.precondition of the step in progress (CG only)
  // speculative line-search ladder (ms_step): when the last accepted step needed n > 1 Armijo trials, the next
  // n trials are queued at once; stage k > 0 runs only if the device-side Armijo test of stage k-1 failed
  // (k_armijo_gate).  Each stage posts its scalars to its own mailbox; the host takes the same decisions from the
  // same doubles, so the trajectory does not change -- only the host round trips between trials disappear.
  static constexpr int SPEC_STAGES = 3;  // extra mailboxes (stage 0 uses the main one)
  struct Mailbox {
    double* h_scal = nullptr;              // host copy of the values (filled by fetch)
    unsigned long long* h_seq = nullptr;   // pinned, mapped: 2*MS_MB_WORDS words, {value bits, sequence word} per entry
    unsigned long long* d_h_seq = nullptr;
    unsigned long long expected[MS_MB_WORDS] = {0};
  } spec[2][SPEC_STAGES];        // (everything a round posts to exists twice: a round can be queued while the one
                                 // before it has not been read yet -- see Ahead)
  Mailbox first_mb[2];           // mailbox of a round's first launch
  Mailbox grad_mb[2];            // mailbox of the gradient pass queued behind a round
  int next_parity = 0;
  // a round queued for a step that has not started yet (queue_ahead)
  struct RoundPlanT {
    int n0 = 1, n_st = 0;
    double alphas[MS_MAX_TRIALS + SPEC_STAGES] = {0};
  };
  struct Ahead {
    bool valid = false;
    bool go_known = false, go = false;  // the device's answer (FoldArgs::go_out) has been read / was DEC_GO
    int kind = 0, go_kind = 0, parity = 0, src = 0, stepper = 0, max_iter = 0;
    bool implicit = false;
    double alpha0 = 0, energy0 = 0, beta = 0, c1 = 0, tol2p = 0, lim = 0;
    RoundPlanT plan;
  } ahead;
  bool ahead_enable = true;      // MS_AHEAD=0 switches the rounds queued ahead off
  int steps_left = 0;            // ... steps that follow the current one in this ms_minimize call
  bool ahead_allowed = false;    // set by ms_minimize: the caller is the library's own loop (nothing else touches the
                                 // context between two steps), and another step follows
  // The direction fold of a round's gradient pass can be left out when the round is queued (StageCtl::defer_dir) and merged
  // into the first fold of the round after it: that round's energy launch then starts right behind the gradient pass
  uint32_t dir_deferred_mask = 0;         // reduce_slots' answer: the mask of the fold it left out
  bool dir_pending[2] = {false, false};   // the round's gradient pass has run (if its gate was open) without its fold
  uint32_t dir_mask[2] = {0, 0};
  uint32_t* kc_gate[2] = {nullptr, nullptr};  // decision word that pass was gated on
  bool last_hist_descent = false;         // the last direction with CG history was a descent direction
  long q_ahead = 0, q_adopted = 0, q_dropped = 0;
  int kc_stepper = 0;
  bool kc_use_history = false;
  // the gradient pass queued with the round of that parity did not store D (CarryState::dir_unwritten as that pass left
  // it: the queueing code restores the carried state, the step that adopts the pass takes the flag from here)
  bool kc_dir_unwritten[2] = {false, false};
  long dir_skipped = 0, dir_materialized = 0;  // ms_direction_stats
  long ka_lean = 0, ka_general = 0;            // ms_energy_stats: k_energy launches (or k_exec records) by instance
  uint32_t ka_lean_off = 0;                    // EnergyArgs::lean_off of this context (MS_KA_LEAN=0 at ms_create, a one-tile mesh)
  // Decision records (ms_internal.h DEC_*): one 128-byte line each, written by the head workgroup of the fold that
  // closes a line-search stage, read by every kernel queued behind that stage.  Record k belongs to stage k of the
  // round being queued; the stream orders a record's readers between its writers.
  uint32_t* d_dec = nullptr;
  static constexpr int N_DEC = 16;
  unsigned long long* h_err = nullptr; // pinned word a fold sets when a gated launch ran on part of its workgroups
  unsigned long long* d_h_err = nullptr;
  long queue_mismatches = 0;           // host and device decisions that differed (every one is also a hard error)
  long q_rounds = 0, q_multi = 0, q_wasted = 0, q_side_accepts = 0;  // queue statistics (ms_queue_stats)
  int escalate_after = 3;              // rejections after which a search goes to multi-trial launches (MS_ESCALATE=n)
  // ms_search_trials: the trials of the most recent ms_step call in the order line_search.py's loop sees them (read
  // only: what the step had waited for anyway), and how many trials the first launch of every round evaluated
  struct TrialRow {
    double alpha, energy, rhs;
    int launch, slot, flags;
  };
  std::vector<TrialRow> trial_log;
  size_t trial_log_cap = 0;            // that call's max_iter
  long first_launch_hist[MS_MAX_TRIALS] = {0};
  // multi-trial launch: trials 0 .. n-2 of a ladder are evaluated in the same energy launch as trial n-1
  // (k_energy<MULTI>); the last trial uses the ordinary outputs, early trial j the side set j
  bool pair_enable = true;       // MS_PAIR=0 switches it off
  bool escalate = true;          // MS_ESCALATE=0: a search that keeps rejecting stays with what the history suggests
  int pair_force = 0;            // MS_PAIR=2 / 3: pair (/ pair + a gated third trial) whenever possible, whatever
                                 // the history predicts (tests)
  bool lbt_normals_current = false;  // phase_energy (leaflet bending_tilt): d_tn already holds the unit vertex normals of x
  // tilt relaxations: the search pass (ms_tsearch.inc; MS_TSEARCH=0: one launch per module, field and trial)
  bool tenergy_enable = true;    // the tilt modules' energy-only evaluations as one launch (every context; MS_TSEARCH=0 off)
  bool tsearch_enable = true;
  bool tsearch_first_single = true;  // the last search accepted its first step size: try one first again
  int64_t tsearch_launches = 0, tsearch_trials = 0;
  bool tsearch_all_failed = false;   // the last search rejected its whole ladder: both of its passes are queued at once
  Mailbox tsearch_mb;                // the last trial's mailbox of the second pass queued that way
  bool no_fast = false;          // MS_NO_FAST=1 (variant builds only)
  bool pair_lean_enable = true;  // MS_PAIR_LEAN=0: write the first two early trials' outputs (copied back if one is accepted)
  static constexpr int N_SIDE = MS_MAX_TRIALS - 1;
  struct SideSet {
    double* partials = nullptr;
    double* scal = nullptr;
    Mailbox mb[2];
  } side[N_SIDE];
  double* xt3 = nullptr;         // full outputs of early trial 1 (MS_PAIR_LEAN=0)
  double* fK3 = nullptr;
  double* fA3 = nullptr;
  double* xt2 = nullptr;         // ... of early trial 0 (MS_PAIR_LEAN=0, the sharded pair)
  double* fK2 = nullptr;
  double* fA2 = nullptr;
  // line-search history (prediction only -- never changes a result), kept per kind of direction: [0] searches along
  // d = -g (gradient descent, CG restarts), [1] along a direction with CG history.  In the steady state of the
  // headline workload the two alternate and behave nothing alike (the second kind is no descent direction or runs out
  // of trials); one shared record would have every search predict the other kind.
  //   pred_trials: trials the last search of the kind spent (an exhausted one: all of them)
  //   acc / rej: of the last LS_HIST accepted steps the accepted alpha and the smallest alpha rejected on the way to
  //   it (INFINITY: accepted at once)
  static constexpr int LS_HIST = 8;
  struct LsHist {
    int pred_trials = 1;
    double acc[LS_HIST] = {0};
    double rej[LS_HIST] = {0};
    int n = 0;
  } ls[2];
  bool ls_reset = true;          // MS_LS_RESET=0: never forget the history on a regime change
  bool speculate = true;         // MS_SPECULATE=0 switches the ladder off
  bool relax_va_valid = false;  // a leaflet relaxation is running: tf[l].va describes the current x
  bool tilt_module_form = false;  // tilt_eval: the magnitude modules in their own mass mode (the plugin API's form,
                                  // tilt_leaflet.py:101-150) instead of the relaxation's vertex-area form
  int factors_leaflet = 0;  // which leaflet's back-prop factors fK/fA hold (1 in, 2 out; 0: not a leaflet's)
  double* d_bt_vert = nullptr;    // (nvp,4) bending_tilt per-vertex record of the last energy pass
  // tilt relaxation work space (positions frozen): unit vertex normals, CG direction, Jacobi M^-1
  double* d_tn = nullptr;
  std::vector<uint8_t> h_vflags;  // host copy of the vertex flag bytes (patch order)
  // per-vertex state (one allocation), patch order, nvp rows
  double* state = nullptr;
  bool own_state = true;
  double* buf[MS_BUF_COUNT] = {nullptr};
  double* d_partials = nullptr;
  double* d_scal = nullptr;
  double* h_scal = nullptr;    // host copy of the mailbox values (fetch() fills it once every slot has arrived)
  // pinned, device-mapped mailbox: one 16-byte {value bits, sequence word} entry per slot, written by k_reduce
  // in a single store
  unsigned long long* h_seq = nullptr;
  unsigned long long* d_h_seq = nullptr;
  unsigned long long ticket = 0;          // ticket of the latest reduce launch
  unsigned long long expected[MS_MB_WORDS] = {0};  // latest ticket that folds each slot (+ the decision entry)
  bool has_boundary = false;
  double* d_stage = nullptr;  // nv*3 staging in external row order
  ms_params params{};
  double area_stiffness = 0.0, target_area = 0.0;  // ms_set_area_penalty (MS_MOD_AREA_PENALTY)
  // shard boundary exchange: rows each rank owns that other ranks' tiles read as halo
  std::vector<int32_t> bnd_off;  // shard_count + 1
  int32_t* d_bnd_rows = nullptr;
  int32_t* d_bnd_off = nullptr;
  int bnd_max = 0;               // longest per-rank list (message stride)
  int32_t* d_halo_rows = nullptr;  // rows of other ranks that THIS rank's tiles read
  int n_halo_rows = 0;
  double* d_scal_all = nullptr;    // shard_count x MS_NSCAL, filled by unpack
  // library-side sharded driver (ms_shard_*): RCCL communicator or a caller-supplied all-gather,
  // message buffers, pinned mailbox for the gathered scalar headers
  void* comm = nullptr;
  ms_allgather_fn allgather_cb = nullptr;
  void* allgather_user = nullptr;
  double* d_xsend = nullptr;
  double* d_xrecv = nullptr;
  // ms_shard_step, peer-to-peer transport: the Armijo decision of a trial is ALSO taken on the device (shard_decide,
  // from the headers in the slab), and the commit, the gradient + direction pass of the accepted point and its exchange
  // are queued behind it, gated on "the main trial was accepted" -- the host replays the decision, and the next step
  // takes the pass's results instead of queueing it (MS_SHARD_CHAIN=0: every decision on the host first)
  bool shard_chain_enable = true;
  uint32_t* d_sh_dec = nullptr;
  unsigned long long* h_sh_post = nullptr;
  unsigned long long* d_h_sh_post = nullptr;
  unsigned long long sh_post_ticket = 0;
  struct ShardChain {
    bool valid = false;
    int stepper = 0;
    bool use_history = false;
    unsigned long long xticket = 0;
  } sh_chain;
  int64_t sh_chained = 0, sh_chain_ran = 0, sh_chain_adopted = 0, sh_chain_dropped = 0;
  int sh_widx = 0;                 // decision word / post pair in use (two of each, in turn)
  unsigned long long sh_post_expect[2] = {0, 0};
  double* h_scal_all = nullptr;    // pinned + mapped, 2 (exchange parity) x shard_count x MS_NSCAL
  double* d_h_scal_all = nullptr;
  unsigned long long* h_xseq = nullptr;
  unsigned long long* d_h_xseq = nullptr;
  unsigned long long xticket = 0;
  // peer-to-peer exchange (ms_shard_peer_*): two receive slabs (the exchanges alternate between them) and one flag
  // word per (slab, peer) on this rank; the peers' slabs / flag words as this process sees them
  double* d_peer_slab = nullptr;            // 2 x shard_count x stride doubles
  unsigned long long* d_peer_flag = nullptr;  // 2 x 16 words
  size_t peer_stride = 0;                   // doubles per (slab, rank) slot
  std::vector<double*> peer_slabs;          // [rank]: base of that rank's slabs (own: d_peer_slab)
  std::vector<unsigned long long*> peer_flags;
  std::vector<void*> peer_opened;           // hipIpcOpenMemHandle results to close
  bool peer_on = false;
  int peer_mem_kind = -1;                   // 0 uncached, 1 fine-grained, 2 plain hipMalloc (peer_alloc)
  unsigned long long peer_ticket = 0;
  PeerFlags* d_peer_flagtab = nullptr;      // [2]: per exchange parity, the peers' flag rows (read by the pack kernel)
  unsigned int* d_peer_arrived = nullptr;   // 16 block counters of the pack kernel
  ms_barrier_fn peer_barrier = nullptr;     // contexts of one process: host-side wait instead of the waiting wave
  void* peer_barrier_user = nullptr;
  double sh_scal[MS_NSCAL] = {0};  // rank-ordered fold of the last exchanges
  double sh_scal2[MS_NSCAL] = {0}; // ... of a pair launch's other trial (header slots SH_ALT + slot)
  bool sh_carry_valid = false, sh_grad_valid = false;
  bool sh_maxg2_valid = false;  // the last direction exchange also carried the gradient rows and max|g_i|^2
  long sh_exchanges = 0;
  bool deterministic = false;  // ms_set_deterministic: staged CSR gather instead of LDS atomics
  // optional per-kernel timing (ms_profile_*)
  bool profiling = false;
  struct ProfRec {
    hipEvent_t a, b;
    int kind;
    int ran_idx;  // gated launch: entry of d_prof_ran that says whether its gate was open (-1: not gated)
  };
  static constexpr int PROF_RAN_CAP = 1 << 16;
  uint32_t* d_prof_ran = nullptr;
  int prof_ran_next = 0;
  std::vector<ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[MS_PROF_KINDS] = {0};
  int64_t prof_n[MS_PROF_KINDS] = {0};
  std::string err;
  // one-tile meshes: launches are recorded and run by ONE workgroup, pack by pack (ms_internal.h: ExecRecorder)
  // the resident step kernel (ms_resident.inc): meshes whose tiles all fit on the chip at once
  bool resident_enable = true;   // MS_RESIDENT=0 switches it off
  int resident_ok = -1;          // -1 not asked yet; 0 / 1: every tile's workgroup can be co-resident
  size_t resident_lds = 0;
  double* d_res_partials = nullptr;
  unsigned int* d_res_bar = nullptr;
  double* d_res_log = nullptr;
  double* d_res_result = nullptr;
  std::vector<double> h_res_log;
  long resident_launches = 0, resident_steps = 0, resident_bails = 0;
  ExecRecorder exec;
  bool exec_relax = true;    // tilt relaxations run as a device program (CK_RELAX); MS_EXEC_RELAX=0: host-driven
  bool exec_fused = true;    // leaflet relaxations with the frozen geometry on the CU (CK_RELAX_FUSED); MS_EXEC_FUSED=0:
                             // the generic program (always, with fixed-order sums: it is bit for bit the kernels)
  bool exec_pins = true;     // k_pin_enforce / k_pin_grad as records of the pack (CK_PIN_*); MS_EXEC_PINS=0: launches behind a flush
  long relax_fused_runs = 0;
  double* d_relax_cells = nullptr;           // [0] trial coefficient, [1] Fletcher-Reeves beta (written by the program)
  unsigned long long* h_relax_box = nullptr; // pinned result mailbox of the program: {iterations, evaluations, parity, done}
  unsigned long long* d_h_relax_box = nullptr;
  unsigned long long relax_ticket = 0;
  long relax_programs = 0;
  bool exec_on = false;      // the recorder is attached to `stream`
  bool exec_wanted = false;  // ... and is to be re-attached when profiling (which needs one launch per kernel) ends
  // pin_to_plane / pin_to_circle (ms_set_pins): one allocation holds every table; pin_lane -1 = none set
  void* d_pins = nullptr;
  PinEnforceArgs pin_enf{};
  PinGradArgs pin_grad{};
  int pin_lane = -1;
  // the hard area constraints (ms_api_area_con.inc): kind and target of ms_set_area_constraint; area_row: MS_CON_BODY_AREA
  // was in the module word of the last ms_set_params (the row takes part in the gradient projection); gA, the lane's
  // partial rows and its result cells (AP_*), allocated on first use
  int area_con_kind = MS_AREA_NONE;
  double area_con_target = 0.0;
  bool area_row = false;
  double* d_area_ga = nullptr;
  double* d_area_part = nullptr;
  double* d_area_res = nullptr;
  // Body's cached area and area gradient (geometry/body.py:347-384): what the last fresh evaluation inside
  // ms_project_area computed
  double* d_area_cache = nullptr;
  double area_cache_area = 0.0, area_cache_norm2 = 0.0;
  bool area_cache_valid = false;
  long area_launches[4] = {0, 0, 0, 0};  // k_area_row, k_area_dots, k_area_fold, k_area_apply
  // the enforce-only constraints (ms_api_enforce.inc): fixed_plane's plane (ms_set_fixed_plane), perimeter's tables, targets,
  // scratch and result cells in one allocation (ms_set_perimeter); launches of the two kernels, trials that ran either
  bool fplane_set = false;
  double fplane_n[3] = {0.0, 0.0, 1.0}, fplane_q[3] = {0.0, 0.0, 0.0};
  void* d_perim = nullptr;
  PerimeterArgs perim{};
  long enforce_only_launches[2] = {0, 0}, enforce_only_trials = 0;
  long pin_enforce_launches = 0, pin_grad_launches = 0, pin_trials = 0;
  // the edge lane (ms_api_edge.inc): edge[t] is the state of kEdgeTerms[t] -- line_tension, then edge_length_penalty.
  // One allocation holds every table of a term, the per-workgroup sums and the module's energy
  struct EdgeLane {
    void* d_blob = nullptr;
    EdgeEnergyArgs en{};
    EdgeGradArgs gr{};
    bool set = false;
    long launches[2] = {0, 0};  // energy kernel, gradient kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof[2];  // event brackets while profiling (ms_line_stats, ...)
  };
  EdgeLane edge[2];
  const StageCtl& stage() const { return stage_; }
 private:
  friend struct StageScope;
  StageCtl stage_;  // (written by StageScope alone)
};
// installs a stage record for the launches queued in its scope; puts back the one that was there before
struct StageScope {
  ms_ctx* c;
  const StageCtl prev;
  StageScope(ms_ctx* ctx, const StageCtl& st) : c(ctx), prev(ctx->stage_) { c->stage_ = st; }
  ~StageScope() { c->stage_ = prev; }
  StageScope(const StageScope&) = delete;
};
