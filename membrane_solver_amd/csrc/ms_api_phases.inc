// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): pass launchers, folds, mailboxes, the energy / gradient / direction phases.
namespace {

// The stream for an operation that is NOT one of the library's recorded kernel launches (copies, memsets, stream
// synchronisation, collectives): whatever the one-workgroup interpreter has recorded so far is launched first, so the
// operation finds the stream in the state the launch-per-kernel path would have left it in.
inline hipStream_t S(ms_ctx* c) {
  if (c->exec_on) (void)c->exec.flush();
  return c->stream;
}
int pin_grad_run(ms_ctx* c, bool volrow);  // (ms_api_pins.inc)
int area_project_gradient(ms_ctx* c);      // (ms_api_area_con.inc: the area row projected out of G, with the volume row if set)
inline bool area_row_active(const ms_ctx* c);
// the edge lane (ms_api_edge.inc): its terms in launch order, kEdgeTerms[t] going with c->edge[t]
struct EdgeTableMsgs {
  const char *row, *first, *second, *perm;
};
struct EdgeTerm {
  uint32_t bit;        // MS_MOD_*
  const char* name;    // the module's
  const char* setter;  // as messages name it
  bool second;         // the term's column is the tables' second one (el0 / ol0), not the first (eg / og)
  EdgeTableMsgs msgs;
};
extern const EdgeTerm kEdgeTerms[2];
int edge_energy_run(ms_ctx* c, int term, bool use_dir, double alpha);
int edge_grad_run(ms_ctx* c, int term, double* g, bool volrow);
// The leaflet add-on passes of one evaluation, in the table's order (ms_slot_writers.h), each with the cell mode the
// table gives it.  tilt_eval, phase_energy and phase_gradient call this once, behind their base passes: the slots'
// base modules have written the cells, every pass that writes the fields' grad rows (tilt_eval) or G (phase_gradient)
// has run.  Behind a gradient pass nothing runs without g_out.
struct AddonCall {
  Phase phase;
  bool use_dir;         // at x + alpha d ...
  double alpha;
  bool trial_tilts;     // ... reading the fields' `trial` rows
  bool tilt_gradients;  // dE/dt added into the fields' grad
  double* g_out;        // the shape gradients' rows added there (phase_gradient), or nullptr
};
int addon_passes(ms_ctx* c, uint32_t modules, const AddonCall& k);  // (ms_api_addons.inc)
// CellMode as the kernels' `cell_mode` fields take it: 0 left alone, 1 added to, 2 defined
constexpr int kernel_cell_mode(CellMode m) { return m == CellMode::DEFINE ? 2 : (m == CellMode::ADD ? 1 : 0); }
// tilt_thetaB_boundary_in (ms_api_thetab_bnd.inc): the ring's table on x (nullptr: the context's positions) or on
// x + alpha d, kept while `frozen` holds; and k_tbb_apply<mode> on it (0 enforce in place, 1 P(enforce(t)) into out,
// 2 project the gradient `field`).  Both return at once when no table with a row is set.
int tbb_geom_run(ms_ctx* c, const double* x, bool use_dir, double alpha, bool frozen);
int tbb_apply_run(ms_ctx* c, int mode, double* field, double* out, bool project);
bool tbb_active(const ms_ctx* c);
inline int exec_flush(ms_ctx* c) {
  if (!c->exec_on) return MS_OK;
  const hipError_t e = c->exec.flush();
  if (e == hipSuccess) return MS_OK;
  c->err = std::string("k_exec launch: ") + hipGetErrorString(e);
  return MS_ERR_HIP;
}

// zero-fill in stream order (a record of its own in a one-tile context: no flush)
inline int zero_doubles(ms_ctx* c, double* p, size_t bytes) {
  if (c->exec_on) {
    ExecMemsetArgs a;
    a.p = p;
    a.n = (int64_t)(bytes / sizeof(double));
    const hipError_t e = c->exec.push(CK_MEMSET, 0, 0, 0, 1, 0, 0, &a, sizeof(a));
    if (e == hipSuccess) return MS_OK;
    c->err = std::string("k_exec record: ") + hipGetErrorString(e);
    return MS_ERR_HIP;
  }
  const hipError_t e = hipMemsetAsync(p, 0, bytes, c->stream);
  if (e == hipSuccess) return MS_OK;
  c->err = std::string("hipMemsetAsync: ") + hipGetErrorString(e);
  return MS_ERR_HIP;
}

inline const double* trial_dir(const ms_ctx* c) { return c->carry.dir_implicit ? c->buf[MS_BUF_G] : c->buf[MS_BUF_D]; }
inline double trial_alpha(const ms_ctx* c, double alpha) { return c->carry.dir_implicit ? -alpha : alpha; }

int fail(ms_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  g_last_error = msg;
  return code;
}

int fail_hip(ms_ctx* c, hipError_t e, const char* what) {
  return fail(c, MS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, call)                                   \
  do {                                                    \
    hipError_t e_ = (call);                               \
    if (e_ != hipSuccess) return fail_hip((c), e_, #call); \
  } while (0)

DeviceMesh device_mesh(const ms_ctx* c) {
  DeviceMesh m;
  m.nv = c->til.nv;
  m.T = c->til.T;
  m.own = c->til.own;
  m.n_tiles = c->til.n_tiles;
  m.has_boundary = c->has_boundary ? 1 : 0;
  m.tile_facet_off = c->d_tile_facet_off;
  m.tile_facets = c->d_tile_facets;
  m.tile_facets32 = c->d_tile_facets32;
  m.tile_facets_lean = c->lane_order_on ? c->d_tile_facets_lean : c->d_tile_facets32;
  m.no_fast = c->no_fast ? 1 : 0;
  m.tf_gamma = c->d_tf_gamma;
  m.gamma_uniform = c->gamma_uniform ? 1 : 0;
  m.gamma_const = c->gamma_const;
  m.kc_uniform = c->kc_uniform ? 1 : 0;
  m.kappa_const = c->kappa_const;
  m.c0_const = c->c0_const;
  m.tile_halo_off = c->d_tile_halo_off;
  m.halo_ids = c->d_halo_ids;
  m.tile_ent_off = c->d_tile_ent_off;
  m.tile_voff = c->d_tile_voff;
  m.vent = c->d_vent;
  m.vflags = c->d_vflags;
  m.kappa = c->d_kappa;
  m.c0 = c->d_c0;
  return m;
}

// RAII-free event bracket: begin() before a launch, end() after it.
// MS_HOST_TIMING=1 (diagnostic): host time from "a fetch found its mailbox complete" to "the next k_energy launch call
// returned" (what the GPU idles through, minus its own dispatch latency), and the launch call alone; printed by
// ms_destroy
struct HostTiming {
  bool on = getenv("MS_HOST_TIMING") != nullptr && atoi(getenv("MS_HOST_TIMING")) != 0;
  double t_fetch = 0.0;
  bool armed = false;
  double sum_gap = 0.0, sum_launch = 0.0, max_gap = 0.0;
  long n = 0;
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
  }
};
static HostTiming g_host_timing;

// A gated launch that found its gate closed returns at once: not a sample of the kernel.  Whether it ran is what the
// decision word said when the launch read it; with profiling on, a one-lane kernel behind the launch (outside its event
// bracket) records exactly that comparison -- the word cannot change in between, only a later fold rewrites it.  (Rounds
// 1-3 guessed from the duration, "< 12 us = empty", which discarded every real launch of a 131 k-facet mesh.)
struct ProfScope {
  ms_ctx* c;
  hipEvent_t a = nullptr, b = nullptr;
  int kind;
  const uint32_t* gate = nullptr;
  uint32_t want = 0;
  ProfScope(ms_ctx* ctx, int k, const uint32_t* gate_word = nullptr, uint32_t gate_want = 0)
      : c(ctx), kind(k), gate(gate_word), want(gate_want) {
    if (!c->profiling || k < 0) return;
    auto get = [&]() {
      hipEvent_t e = nullptr;
      if (!c->prof_pool.empty()) {
        e = c->prof_pool.back();
        c->prof_pool.pop_back();
      } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
      }
      return e;
    };
    a = get();
    b = get();
    if (a && b) (void)hipEventRecord(a, c->stream);
  }
  ~ProfScope() {
    if (!c->profiling || kind < 0 || !a || !b) return;
    (void)hipEventRecord(b, c->stream);
    int ran_idx = -1;
    if (gate != nullptr && c->d_prof_ran != nullptr && c->prof_ran_next < ms_ctx::PROF_RAN_CAP) {
      ran_idx = c->prof_ran_next++;
      (void)launch_gate_probe(gate, want, c->d_prof_ran + ran_idx, c->stream);
    }
    c->prof_pending.push_back({a, b, kind, ran_idx});
  }
};

constexpr uint32_t MASK_ENERGY = (1u << MS_S_ESURF) | (1u << MS_S_VOL) | (1u << MS_S_EBEND) |
                                 (1u << MS_S_MINEDGE2) | (1u << MS_S_GUARD) | (1u << MS_S_ETILT) |
                                 (1u << MS_S_EBT) | (1u << MS_S_ETS) | (1u << MS_S_ETILT_IN) |
                                 (1u << MS_S_ETILT_OUT) | (1u << MS_S_ETS_IN) | (1u << MS_S_ETS_OUT) |
                                 (1u << MS_S_EBT_IN) | (1u << MS_S_EBT_OUT) | (1u << MS_S_EDT_IN) | (1u << MS_S_EDT_OUT);
constexpr uint32_t MS_TILT_MODS = MS_MOD_TILT | MS_MOD_BENDING_TILT | MS_MOD_TILT_SMOOTH;  // modules reading the single tilt field
constexpr uint32_t MS_LEAFLET_BT = MS_MOD_BENDING_TILT_IN | MS_MOD_BENDING_TILT_OUT;
constexpr uint32_t MS_LEAFLET_DT = MS_MOD_TILT_DISK_TARGET_IN | MS_MOD_TILT_DISK_TARGET_OUT;
// the rim sources: no slot of their own (MS_NSCAL is full) -- their sums ride in the leaflet's tilt-magnitude slot -- and no
// shape gradient, so they are not in MS_TILT_SHAPE_MODS
constexpr uint32_t MS_LEAFLET_RS = MS_MOD_TILT_RIM_SOURCE_IN | MS_MOD_TILT_RIM_SOURCE_OUT;
// (tilt_rim_source_bilayer is NOT part of MS_LEAFLET_RS: that mask selects the per-field tables.)  Every module that rides
// in another one's slot, these among them; the lanes that cannot carry one decline them all
constexpr uint32_t MS_LEAFLET_ADDONS = addon_mask();  // (ms_slot_writers.h)
constexpr uint32_t MS_LEAFLET_MODS = MS_MOD_TILT_IN | MS_MOD_TILT_OUT | MS_MOD_TILT_SMOOTH_IN | MS_MOD_TILT_SMOOTH_OUT | MS_LEAFLET_BT | MS_LEAFLET_DT | MS_LEAFLET_ADDONS;
constexpr uint32_t MS_ANY_TILT_MODS = MS_TILT_MODS | MS_LEAFLET_MODS;
// the edge modules: energy added into the MS_S_ESURF partials behind the energy pass, gradient into G behind K_C; they
// share one lane of the step (one trial per launch, every Armijo decision the host's, the separate direction pass)
constexpr uint32_t MS_EDGE_MODS = MS_MOD_LINE_TENSION | MS_MOD_EDGE_LENGTH_PENALTY;
// modules whose shape gradient is added into g by a pass after K_C (so the direction cannot be fused)
constexpr uint32_t MS_TILT_SHAPE_MODS = MS_MOD_TILT | MS_MOD_TILT_IN | MS_MOD_TILT_OUT | MS_LEAFLET_BT | MS_LEAFLET_DT | MS_MOD_TILT_COUPLING | MS_MOD_RIM_SLOPE_MATCH_OUT;
using TiltField = ms_ctx::TiltField;
using RoundPlan = ms_ctx::RoundPlanT;

// the tilt fields the module set reads: [0] single field, [1] inner, [2] outer leaflet
int active_fields(ms_ctx* c, uint32_t mods, TiltField* out[3]) {
  int n = 0;
  for (int k = 0; k < 3; ++k) {
    TiltField& f = c->tf[k];
    const uint32_t reads = k == 0 ? MS_TILT_MODS : f.mods();
    if (mods & reads) out[n++] = &f;
  }
  return n;
}

// mode 0 energy / 1 energy+gradients read `src`; mode 2 projects `src` onto the tangent
// planes of x (+ alpha d) and writes `dst`.
int tilt_pass_f(ms_ctx* c, TiltField& f, int mode, bool use_dir, double alpha, const double* src = nullptr,
                double* dst = nullptr, bool shape_gradient = true, bool lumped = false, double k_override = -1.0,
                int slot_override = -1, bool tg_accumulate = false, bool masked = true) {
  if (!f.tilts) return fail(c, MS_ERR_STATE, "tilt module active but its tilt field was never set (ms_set_tilts / ms_set_leaflet_tilts)");
  TiltArgs a;
  a.fields = nullptr;
  a.fields_rows = 0;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.tilts = src ? src : f.tilts;
  a.tilts_out = dst ? dst : f.tilts;
  a.k_tilt = k_override >= 0.0 ? k_override : f.k_tilt;
  a.g = shape_gradient ? c->buf[MS_BUF_G] : nullptr;
  a.tilt_grad = f.grad;
  a.minv = nullptr;
  a.partials = c->d_partials;
  a.e_slot = slot_override >= 0 ? slot_override : f.s_etilt;
  a.consistent = (f.consistent && !lumped) ? 1 : 0;
  a.tg_accumulate = tg_accumulate ? 1 : 0;
  a.cons_tilt_grad = (a.consistent && c->tilt_module_form) ? 1 : 0;
  a.va_out = nullptr;
  a.absent_bit = (masked && mode != 2) ? f.absent_bit : 0;  // (the magnitude module's facets; the projection reads none)
  {
    ProfScope ps(c, 4);
    HIPCHK(c, launch_tilt(a, mode, c->cap, c->til.max_ent, c->stream));
  }
  return MS_OK;
}
int tilt_pass(ms_ctx* c, int mode, bool use_dir, double alpha, const double* src = nullptr,
              double* dst = nullptr, bool shape_gradient = true) {
  return tilt_pass_f(c, c->tf[0], mode, use_dir, alpha, src, dst, shape_gradient);
}
// bending_tilt facet pass (mode 0 energy / 1 + factors / 2 + tilt gradient) on the positions of
// the preceding energy pass; `tilts` = the tangent tilts belonging to those positions
int bt_pass_f(ms_ctx* c, TiltField& f, int mode, bool use_dir, double alpha, const double* tilts,
              bool with_tilt_energy = false);
int bt_pass(ms_ctx* c, int mode, bool use_dir, double alpha, const double* tilts, bool with_tilt_energy = false) {
  return bt_pass_f(c, c->tf[0], mode, use_dir, alpha, tilts, with_tilt_energy);
}
// with_tilt_energy (mode 0): the kernel also sums the field's tilt-magnitude energy (per-facet form) from the rows it
// stages anyway -- same operations as k_tilt's energy-only launch, which the caller then leaves out
int bt_pass_f(ms_ctx* c, TiltField& f, int mode, bool use_dir, double alpha, const double* tilts, bool with_tilt_energy) {
  if (!f.tilts) return fail(c, MS_ERR_STATE, "bending_tilt module active but its tilt field was never set");
  const bool leaflet = &f != &c->tf[0];
  if (leaflet && (!f.kappa || !f.bt_vert))
    return fail(c, MS_ERR_STATE, "bending_tilt_in/out active but ms_set_leaflet_bending was never called");
  BtArgs a;
  a.m = device_mesh(c);
  if (leaflet) {
    a.m.kappa = f.kappa;
    a.m.kc_uniform = 0;  // per-leaflet arrays
    a.m.c0 = f.c0;
  }
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.tilts = tilts;
  a.bt_vert = leaflet ? f.bt_vert : c->d_bt_vert;
  a.fK = c->buf[MS_BUF_FK];
  a.fA = c->buf[MS_BUF_FA];
  a.tilt_grad = f.grad;
  a.partials = c->d_partials;
  a.g = c->buf[MS_BUF_G];
  a.div_sign = f.div_sign;
  a.e_slot = f.s_ebt;
  a.k_tilt_fused = (with_tilt_energy && mode == 0) ? f.k_tilt : 0.0;
  a.e_tilt_slot = f.s_etilt;
  {
    ProfScope ps(c, 5);
    HIPCHK(c, launch_bt(a, mode, c->cap, c->til.max_ent, c->stream));
  }
  return MS_OK;
}
// tilt smoothness pass (mode 0 energy / 1 + tilt gradient / 2 Jacobi diagonal into `diag`)
int ts_pass_f(ms_ctx* c, TiltField& f, int mode, bool use_dir, double alpha, const double* tilts,
              double* diag = nullptr, double k_override = -1.0) {
  if (!f.tilts) return fail(c, MS_ERR_STATE, "tilt_smoothness module active but its tilt field was never set");
  TsArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.tilts = tilts;
  a.k_smooth = k_override >= 0.0 ? k_override : f.k_smooth;
  a.tilt_grad = f.grad;
  a.diag = diag;
  a.partials = c->d_partials;
  a.e_slot = f.s_ets;
  a.absent_bit = mode == 2 ? 0 : f.absent_bit;  // (the Jacobi diagonal keeps every facet: preconditioners.py:121-140)
  {
    ProfScope ps(c, 11);
    HIPCHK(c, launch_ts(a, mode, c->cap, c->til.max_ent, c->stream));
  }
  return MS_OK;
}
int ts_pass(ms_ctx* c, int mode, bool use_dir, double alpha, const double* tilts, double* diag = nullptr) {
  return ts_pass_f(c, c->tf[0], mode, use_dir, alpha, tilts, diag);
}
// tilt_disk_target_in/out on the positions x (+ alpha d) and `tilts`: (radius reduction ->) difference field ->
// tilt magnitude kernel on it with k = strength.  mode 0 energy / 1 energy + shape gradient (+ tilt gradient
// ADDED to f.grad when tilt_gradient).
int reduce_slots(ms_ctx* c, uint32_t mask);
int disk_target_pass(ms_ctx* c, TiltField& f, int mode, bool use_dir, double alpha, const double* tilts,
                     bool shape_gradient, bool tilt_gradient) {
  if (!f.disk || !f.diff) return fail(c, MS_ERR_STATE, "tilt_disk_target active but ms_set_leaflet_disk_target was never called");
  DiskTargetArgs a;
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.nv = c->til.nv;
  a.T = c->til.own;  // (row stride of the streaming kernels)
  a.n_tiles = c->til.n_tiles;
  a.vflags = c->d_vflags;
  a.disk = f.disk;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.tilts = tilts;
  a.diff = f.diff;
  a.theta_b = f.dt.theta_b;
  a.lambda = f.dt.lambda;
  a.radius = f.dt.radius;
  for (int k = 0; k < 3; ++k) {
    a.center[k] = f.dt.center[k];
    a.normal[k] = f.dt.normal[k];
  }
  a.scal = c->d_scal;
  a.partials = c->d_partials;
  a.r_slot = f.s_dtr;
  a.target = nullptr;
  // a relaxation in progress: x is frozen, so the disk radius and the target profile theta(r) r_hat are computed ONCE
  // (relax_fields primes them) and every evaluation of the relaxation only takes the difference
  const bool frozen = c->relax_va_valid && !use_dir;
  {
    ProfScope ps(c, 6);
    if (frozen && !f.dt_target) {
      const size_t b3 = sizeof(double) * 3 * (size_t)c->til.nvp;
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&f.dt_target), b3));
      HIPCHK(c, hipMemset(f.dt_target, 0, b3));
    }
    a.target = frozen ? f.dt_target : nullptr;
    if (!frozen || !f.dt_target_valid) {
      if (!(f.dt.radius > 0.0)) {
        HIPCHK(c, launch_disk_target(a, 0, c->stream));
        int rc = reduce_slots(c, 1u << f.s_dtr);
        if (rc) return rc;
      }
      if (frozen) {
        HIPCHK(c, launch_disk_target(a, 2, c->stream));
        f.dt_target_valid = true;
      }
    }
    HIPCHK(c, launch_disk_target(a, frozen ? 3 : 1, c->stream));
  }
  return tilt_pass_f(c, f, mode, use_dir, alpha, f.diff, nullptr, shape_gradient, /*lumped=*/true, f.dt.strength,
                     f.s_edt, tilt_gradient, /*masked=*/false);  // (tilt_disk_target_in/out never read the absence mask)
}
constexpr uint32_t MASK_GRAD = (1u << MS_S_GGC) | (1u << MS_S_GCGC);
constexpr uint32_t MASK_DIR = (1u << MS_S_GNORM2) | (1u << MS_S_GDOTD) | (1u << MS_S_MAXD2) | (1u << MS_S_MAXG2);

// MS_TRACE_STEPS=1: one stderr line per step of ms_minimize (what the search did, host time since the step before,
// running queue statistics)
bool trace_steps() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("MS_TRACE_STEPS");
    v = (e && atoi(e) != 0) ? 1 : 0;
  }
  return v == 1;
}
// MS_TRACE_QUEUE=1: one stderr line per fold launch / mailbox swap / fetch (debugging the line-search queue)
bool trace_queue() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("MS_TRACE_QUEUE");
    v = (e && atoi(e) != 0) ? 1 : 0;
  }
  return v != 0;
}
const char* box_name(ms_ctx* c, const void* h_seq) {
  // (the mailboxes are swapped in and out of the context: name them by allocation)
  static std::map<const void*, std::string> names;
  auto it = names.find(h_seq);
  if (it == names.end()) it = names.emplace(h_seq, "box" + std::to_string(names.size())).first;
  (void)c;
  return it->second.c_str();
}

inline uint32_t* dec_word(ms_ctx* c, int parity, int k) { return c->d_dec + (size_t)MS_DEC_STRIDE * (parity * 4 + k); }
inline uint32_t* go_word(ms_ctx* c, int parity) { return c->d_dec + (size_t)MS_DEC_STRIDE * (8 + parity); }
inline const double* go_rhs(ms_ctx* c, int parity) { return reinterpret_cast<const double*>(go_word(c, parity) + 2); }

// energy slots whose sum is the energy the Armijo test compares (the ladder only runs for module sets whose energy
// is surface + bending: ms_step's can_chain)
uint32_t armijo_slots(const ms_ctx* c) {
  return ((c->params.modules & MS_MOD_SURFACE) ? (1u << MS_S_ESURF) : 0u) |
         ((c->params.modules & MS_MOD_BENDING) ? (1u << MS_S_EBEND) : 0u);
}

// slots an energy pass of `modules` leaves partials in: the core five, and the tilt families' only when one of them is on
uint32_t energy_mask(uint32_t modules) {
  constexpr uint32_t core = (1u << MS_S_ESURF) | (1u << MS_S_VOL) | (1u << MS_S_EBEND) | (1u << MS_S_MINEDGE2) |
                            (1u << MS_S_GUARD);
  // (body_area_penalty and the tilt families exclude each other: ms_set_params)
  return (modules & MS_ANY_TILT_MODS) ? MASK_ENERGY : ((modules & MS_MOD_AREA_PENALTY) ? (core | (1u << MS_S_AREA)) : core);
}

// a pinned, device-mapped mailbox of its own (stage mailboxes of the line-search queue, the side sets' boxes)
int make_mailbox(ms_ctx* c, ms_ctx::Mailbox& m) {
  if (m.h_seq) return MS_OK;
  m.h_scal = static_cast<double*>(calloc(MS_NSCAL, sizeof(double)));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&m.h_seq), sizeof(unsigned long long) * 2 * MS_MB_WORDS,
                          hipHostMallocMapped));
  memset(m.h_seq, 0, sizeof(unsigned long long) * 2 * MS_MB_WORDS);
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&m.d_h_seq), m.h_seq, 0));
  return MS_OK;
}
// make stage mailbox `m` the context's mailbox (and back: the swap is its own inverse)
void swap_mailbox(ms_ctx* c, ms_ctx::Mailbox& m) {
  if (trace_queue()) fprintf(stderr, "[msq] swap %s <-> %s\n", box_name(c, c->h_seq), box_name(c, m.h_seq));
  std::swap(c->h_scal, m.h_scal);
  std::swap(c->h_seq, m.h_seq);
  std::swap(c->d_h_seq, m.d_h_seq);
  for (int sl = 0; sl < MS_MB_WORDS; ++sl) std::swap(c->expected[sl], m.expected[sl]);
}
// partial sets, device scalars and mailboxes of the EARLY trials of a multi-trial launch (the last trial uses the
// context's own): ms_step's Armijo ladder and the tilt relaxations' search pass share them
int ensure_side_sets(ms_ctx* c, int n_side) {
  const size_t pb = sizeof(double) * MS_NPART * (size_t)std::max(1, c->til.n_tiles);
  for (int k = 0; k < n_side && k < ms_ctx::N_SIDE; ++k) {
    ms_ctx::SideSet& sd = c->side[k];
    if (!sd.partials) {
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sd.partials), pb));
      HIPCHK(c, hipMemset(sd.partials, 0, pb));
    }
    if (!sd.scal) {
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sd.scal), sizeof(double) * MS_NSCAL));
      HIPCHK(c, hipMemset(sd.scal, 0, sizeof(double) * MS_NSCAL));
    }
    for (auto& m : sd.mb)
      if (int rc = make_mailbox(c, m)) return rc;
  }
  return MS_OK;
}

int reduce_slots(ms_ctx* c, uint32_t mask) {
  const StageCtl& st = c->stage();
  if (st.defer_dir && (mask & (1u << MS_S_GDOTD)) && st.cur_dec == nullptr) {
    c->dir_deferred_mask = mask;  // (queue_round: the fold of the round after this one takes these slots along)
    return MS_OK;
  }
  mask |= st.cur_extra_mask;
  ProfScope ps(c, 3, st.cur_gate, st.cur_gate_want);
  ++c->ticket;
  if (trace_queue())
    fprintf(stderr, "[msq] fold ticket %llu mask %#x -> %s gate %p want %u dec %p trials %d\n",
            (unsigned long long)(c->ticket), mask, box_name(c, c->h_seq), (const void*)st.cur_gate, st.cur_gate_want,
            (const void*)st.cur_dec, (int)st.pair_on);
  // a multi-trial launch has no tilt module: only the core slots carry anything (and the sharded driver parks the other
  // trial's fold in the tilt slots of the device scalars, which the full mask would overwrite)
  const int n_multi = st.pair_on > 1 ? st.pair_on : 1;
  if (n_multi > 1 && !st.multi_any_slot) {
    const uint32_t core = (1u << MS_S_ESURF) | (1u << MS_S_VOL) | (1u << MS_S_EBEND) | (1u << MS_S_MINEDGE2) |
                          (1u << MS_S_GUARD) | st.cur_extra_mask;
    // (nobody is to wait for the dropped slots: an older, gated-out launch may have left a ticket there)
    for (int sl = 0; sl < MS_NSCAL; ++sl)
      if (mask & ~core & (1u << sl)) {
        c->expected[sl] = 0;
        for (int k = 0; k + 1 < n_multi; ++k) c->side[k].mb[st.cur_parity].expected[sl] = 0;
      }
    mask &= core;
  }
  FoldArgs f;
  memset(&f, 0, sizeof(f));
  f.n_tiles = c->til.n_tiles;
  f.tile0 = c->tile0;
  f.tile1 = c->tile1;
  f.slot_mask = mask;
  f.ticket = c->ticket;
  f.n_sets = n_multi;
  f.gate = st.cur_gate;
  f.gate_want = st.cur_gate_want;
  f.check_ran = (st.cur_gate != nullptr && st.cur_check_ran) ? 1 : 0;
  f.dec_out = st.cur_dec;
  f.counter = c->d_dec ? c->d_dec + (size_t)MS_DEC_STRIDE * (ms_ctx::N_DEC - 1) : nullptr;  // (the last record's line)
  f.e_mask = armijo_slots(c);
  f.host_err = c->d_h_err;
  for (int j = 0; j < MS_MAX_TRIALS; ++j) f.rhs[j] = st.cur_rhs[j];
  // an energy-only early trial needs nothing but its energy slots (the head workgroup folds those); an early trial
  // with outputs of its own (MS_PAIR_LEAN=0, the sharded pair) can be accepted as it is and needs every slot
  f.side_full = (n_multi > 1 && (!st.pair_lean || !f.dec_out)) ? 1 : 0;
  for (int j = 0; j + 1 < n_multi; ++j) {
    ms_ctx::SideSet& sd = c->side[j];
    f.set[j].partials = sd.partials;
    f.set[j].scal = (j == 0 && st.pair_scal2) ? st.pair_scal2 : sd.scal;
    f.set[j].host_box = sd.mb[st.cur_parity].d_h_seq;
    const uint32_t posted = (f.side_full || !f.dec_out) ? mask : (mask & f.e_mask);
    for (int sl = 0; sl < MS_NSCAL; ++sl)
      if (posted & (1u << sl)) sd.mb[st.cur_parity].expected[sl] = c->ticket;
  }
  f.set[n_multi - 1].partials = c->d_partials;
  f.set[n_multi - 1].scal = c->d_scal;
  f.set[n_multi - 1].host_box = c->d_h_seq;
  for (int sl = 0; sl < MS_NSCAL; ++sl)
    if (mask & (1u << sl)) c->expected[sl] = c->ticket;
  f.rhs_dev = st.cur_rhs_dev;
  if (st.cur_go_kind && f.dec_out && (mask & (1u << MS_S_GDOTD))) {  // merged: direction scalars + GO + Armijo decision
    f.go_out = st.cur_go;
    f.go_kind = st.cur_go_kind;
    f.go_tol2 = st.cur_go_val[0];
    f.go_lim = st.cur_go_val[1];
    f.go_e0 = st.cur_go_val[2];
    f.go_c = st.cur_go_val[3];
    f.go_alpha0 = st.cur_go_val[4];
    f.go_beta = st.cur_go_val[5];
  }
  if (f.dec_out) c->expected[MS_MB_DEC] = c->ticket;
  HIPCHK(c, launch_reduce(f, c->stream));
  return MS_OK;
}

// The tilt-module energies of an energy-only evaluation (a shape trial, the energy at x) in ONE pass over the facets
// instead of one launch per module and field (k_bt<0>, k_tilt<0>, k_tsmooth<0>): the search pass of the relaxations
// (ms_tsearch.inc) with one "step size", the evaluated positions and the fields' rows as they are.  *used = false: this
// module set keeps its own launches (disk targets, consistent mass, a lone tilt module on the single field, three fields).
// skip_bt: the bending_tilt modules keep their own facet passes (an evaluation that writes their back-propagation
// factors); the pass then covers the other tilt modules only.
int tilt_energy_pass(ms_ctx* c, uint32_t modules, bool use_dir, double alpha, bool* used, bool dry = false,
                     bool skip_bt = false) {
  *used = false;
  if (!c->tenergy_enable) return MS_OK;
  if (modules & MS_MOD_RIM_SLOPE_MATCH_OUT) return MS_OK;  // (the rim matching term keeps the launch-per-module evaluation)
  TsearchArgs a;
  int nf = 0;
  for (int l = 0; l < 3; ++l) {
    TiltField& f = c->tf[l];
    const bool single = l == 0;
    const bool tilt_on = single ? (modules & MS_MOD_TILT) != 0 : (modules & f.mod_tilt) != 0;
    const bool bt_on = !skip_bt && (single ? (modules & MS_MOD_BENDING_TILT) != 0 : (modules & f.mod_bt) != 0);
    const bool ts_on = single ? (modules & MS_MOD_TILT_SMOOTH) != 0 : (modules & f.mod_smooth) != 0;
    // (a disk target keeps its own passes -- the difference field and the magnitude kernel on it -- next to this one)
    if (!(tilt_on || bt_on || ts_on)) continue;
    if (nf == 2 || !f.tilts) return MS_OK;
    if (f.absent_bit && (tilt_on || ts_on)) return MS_OK;  // an absence mask: k_tilt<0> / k_tsmooth<0> honour it, this pass does not
    if (tilt_on && (f.consistent || (single && !(bt_on && f.k_tilt != 0.0)))) return MS_OK;
    TsearchField& o = a.f[nf++];
    o.tilts = use_dir ? f.trial : f.tilts;
    o.src = o.tilts;
    o.bt_vert = bt_on ? (single ? c->d_bt_vert : f.bt_vert) : nullptr;
    o.kappa = bt_on ? (single ? device_mesh(c).kappa : f.kappa) : nullptr;
    if (bt_on && (!o.bt_vert || !o.kappa)) return MS_OK;
    o.va = nullptr;
    o.div_sign = f.div_sign;
    o.k_tilt = f.k_tilt;
    o.k_smooth = f.k_smooth;
    o.tilt_form = tilt_on ? 1 : 0;
    o.s_ebt = bt_on ? f.s_ebt : -1;
    o.s_etilt = f.s_etilt;
    o.s_ets = ts_on ? f.s_ets : -1;
    o.fixed_bit = 0;
    o.trial_out = nullptr;
  }
  if (nf == 0) return MS_OK;
  if (nf == 1) a.f[1] = a.f[0];
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.normals = nullptr;
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.plain = 1;
  a.n_fields = nf;
  a.n_trials = 1;
  for (int j = 0; j < MS_MAX_TRIALS; ++j) {
    a.coef[j] = 0.0;
    a.partials[j] = j == 0 ? c->d_partials : nullptr;
  }
  if (!tsearch_fits(c->cap, nf, 1)) return MS_OK;
  if (dry) {  // (the caller only asks whether the pass will cover this evaluation)
    *used = true;
    return MS_OK;
  }
  {
    ProfScope ps(c, 12);
    HIPCHK(c, launch_tsearch(a, c->cap, c->stream));
  }
  *used = true;
  return MS_OK;
}

int phase_energy(ms_ctx* c, uint32_t modules, bool use_dir, double alpha, bool write_trial,
                 bool guard, bool write_factors, bool reduce_now = true) {
  const StageCtl& st = c->stage();
  c->carry.invalidate_with_bt();
  c->sh_carry_valid = c->sh_grad_valid = false;
  EnergyArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.d = use_dir ? trial_dir(c) : nullptr;
  a.alpha = trial_alpha(c, alpha);
  a.xt = write_trial ? c->buf[MS_BUF_XT] : nullptr;
  const bool bt = (modules & MS_MOD_BENDING_TILT) != 0;
  const bool lbt = (modules & MS_LEAFLET_BT) != 0;
  // energy-only evaluation: the tilt modules' facet passes as one launch behind the shape kernels (tilt_energy_pass)
  bool fused_tilt = false;
  if (!write_factors && (modules & MS_ANY_TILT_MODS))
    if (int rc_p = tilt_energy_pass(c, modules, use_dir, alpha, &fused_tilt, /*dry=*/true)) return rc_p;
  // ... and in an evaluation that writes the leaflet bending_tilt factors: the OTHER leaflet modules (tilt magnitude,
  // smoothness) as one launch
  bool fused_rest = false;
  if (write_factors && lbt && !(modules & MS_TILT_MODS))
    if (int rc_p = tilt_energy_pass(c, modules, use_dir, alpha, &fused_rest, /*dry=*/true, /*skip_bt=*/true)) return rc_p;
  const bool bend = (modules & MS_MOD_BENDING) != 0 || bt || lbt;
  a.fK = (bend && write_factors) ? c->buf[MS_BUF_FK] : nullptr;
  a.fA = (bend && write_factors) ? c->buf[MS_BUF_FA] : nullptr;
  a.bt_vert = bt ? c->d_bt_vert : nullptr;
  a.bt_normals = nullptr;
  a.gate = st.cur_gate_fold_only ? nullptr : st.cur_gate;
  a.gate_want = st.cur_gate_want;
  a.atomic = c->deterministic ? 0 : 1;
  a.lean_off = c->ka_lean_off;
  a.pair = 0;
  for (int j = 0; j < MS_MAX_TRIALS - 1; ++j) {
    a.alpha_side[j] = 0.0;
    a.partials_side[j] = nullptr;
  }
  for (int j = 0; j < 2; ++j) a.xt_side[j] = a.fK_side[j] = a.fA_side[j] = nullptr;
  if (st.pair_on > 1) {
    if (!use_dir || guard || !write_factors || !(modules & MS_MOD_BENDING) || bt || lbt || !c->side[0].partials)
      return fail(c, MS_ERR_STATE, "multi-trial launch: not an ordinary bending trial");
    if (st.pair_on > MS_MAX_TRIALS || !c->side[st.pair_on - 2].partials)
      return fail(c, MS_ERR_STATE, "multi-trial launch: side sets not allocated");
    a.pair = st.pair_on;
    for (int j = 0; j + 1 < st.pair_on; ++j) {
      a.alpha_side[j] = trial_alpha(c, st.pair_alpha[j]);
      a.partials_side[j] = c->side[j].partials;
    }
    if (!st.pair_lean) {  // the first two early trials write their own positions / factors
      double* const sx[2] = {c->xt2, c->xt3};
      double* const sk[2] = {c->fK2, c->fK3};
      double* const sa[2] = {c->fA2, c->fA3};
      for (int j = 0; j < 2 && j + 1 < st.pair_on; ++j) {
        if (!sk[j]) return fail(c, MS_ERR_STATE, "multi-trial launch: output side set not allocated");
        a.xt_side[j] = write_trial ? sx[j] : nullptr;
        a.fK_side[j] = sk[j];
        a.fA_side[j] = sa[j];
      }
      if (st.pair_on > 3) return fail(c, MS_ERR_STATE, "multi-trial launch: only two early trials can write outputs");
    }
  }
  if (bt && !c->d_bt_vert) return fail(c, MS_ERR_STATE, "bending_tilt: ms_set_params did not allocate its buffers");
  // the edge modules take the penalties' lane: one trial per launch, every Armijo decision the host's
  if (st.pair_on > 1 || st.cur_gate != nullptr || lbt)
    for (const EdgeTerm& t : kEdgeTerms)
      if (modules & t.bit)
        return fail(c, MS_ERR_STATE, std::string(t.name) + ": the energy pass was queued on the device-decided lane");
  a.partials = c->d_partials;
  a.bending_model = c->params.bending_model;
  a.modules = modules;
  const bool tilt_only = st.energy_tilt_only && !use_dir && !write_factors && !write_trial && fused_tilt;
  if (tilt_only && !lbt) {
    // (nothing: the shape kernel's results for this x are where they were left)
  } else if (!lbt) {
    ProfScope ps(c, a.pair > 3 ? 10 : (a.pair == 3 ? 8 : (a.pair ? 7 : 0)), a.gate, a.gate_want);
    const double t_l0 = g_host_timing.on ? HostTiming::now() : 0.0;
    EnergyInst ran{};
    HIPCHK(c, launch_energy(a, guard && use_dir, c->cap, c->til.max_ent, c->stream, &ran));
    ++(ran.lean ? c->ka_lean : c->ka_general);
    if (g_host_timing.on && g_host_timing.armed) {
      const double t1 = HostTiming::now();
      g_host_timing.armed = false;
      g_host_timing.sum_gap += t1 - g_host_timing.t_fetch;
      g_host_timing.max_gap = std::max(g_host_timing.max_gap, t1 - g_host_timing.t_fetch);
      g_host_timing.sum_launch += t1 - t_l0;
      ++g_host_timing.n;
    }
  } else {
    // leaflet bending_tilt: the tilt projections and the unit vertex normals of the evaluated positions come
    // first, then per leaflet an energy pass with that leaflet's (kappa, c0) (signed curvature, K_dir = n)
    // directly followed by its facet pass, because the factor buffers serve one leaflet at a time
    // (the projections onto the trial surface ride in the normals launch below: same normals, same arithmetic)
    if (!c->d_tn) {
      const size_t b3 = sizeof(double) * 3 * (size_t)c->til.nvp;
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_tn), b3));
      HIPCHK(c, hipMemset(c->d_tn, 0, b3));
    }
    if (!(c->lbt_normals_current && !use_dir)) {
      TiltArgs ta;
      ta.m = device_mesh(c);
      ta.tile0 = c->tile0;
      ta.tile1 = c->tile1;
      ta.x = c->buf[MS_BUF_X];
      ta.d = use_dir ? trial_dir(c) : nullptr;
      ta.alpha = trial_alpha(c, alpha);
      ta.tilts = c->tf[1].tilts ? c->tf[1].tilts : c->tf[2].tilts;
      ta.tilts_out = c->d_tn;
      ta.k_tilt = 0.0;
      ta.g = nullptr;
      ta.tilt_grad = nullptr;
      ta.minv = nullptr;
      ta.partials = c->d_partials;
      ta.e_slot = MS_S_ETILT;
      ta.consistent = 0;
      ta.tg_accumulate = 0;
      ta.cons_tilt_grad = 0;
      ta.va_out = nullptr;
      if (!ta.tilts) return fail(c, MS_ERR_STATE, "bending_tilt_in/out active but ms_set_leaflet_tilts was never called");
      // (use_dir: the stored tilts onto the TRIAL surface, kept aside in `trial`; proj_at_x_in_normals: ms_step's
      // projection of the stored tilts onto x itself, in place)
      for (int l = 1, k = 0; l <= 2 && (use_dir || st.proj_at_x_in_normals); ++l) {
        TiltField& f = c->tf[l];
        if (!(modules & f.mods())) continue;
        if (!f.tilts) return fail(c, MS_ERR_STATE, "tilt module active but its tilt field was never set (ms_set_tilts / ms_set_leaflet_tilts)");
        ta.fld_in[k] = f.tilts;
        ta.fld_out[k] = use_dir ? f.trial : f.tilts;
        ++k;
      }
      ProfScope ps(c, 4);
      HIPCHK(c, launch_tilt(ta, 3, c->cap, c->til.max_ent, c->stream));
    }
    // energy-only evaluation with both leaflets' bending_tilt (their facet passes ride in the one launch below): ONE
    // energy launch leaves both per-vertex records -- the curvature sums are the same, only (kappa, c0) differ
    const bool dual = fused_tilt && (modules & c->tf[1].mod_bt) && (modules & c->tf[2].mod_bt) && !a.fK &&
                      c->tf[1].kappa && c->tf[2].kappa && c->tf[1].bt_vert && c->tf[2].bt_vert;
    for (int l = 1; l <= 2; ++l) {
      TiltField& f = c->tf[l];
      if (!(modules & f.mod_bt)) continue;
      if (dual && l == 2) continue;
      if (tilt_only) continue;  // (the records of this x are in place)
      if (!f.kappa || !f.bt_vert || !f.tilts)
        return fail(c, MS_ERR_STATE, "bending_tilt_in/out active but ms_set_leaflet_tilts / ms_set_leaflet_bending were not called");
      EnergyArgs al = a;
      if (dual) {
        al.bt_vert2 = c->tf[2].bt_vert;
        al.kappa2 = c->tf[2].kappa;
        al.c02 = c->tf[2].c0;
      }
      al.m.kappa = f.kappa;
      al.m.kc_uniform = 0;  // per-leaflet arrays
      al.m.c0 = f.c0;
      al.bt_vert = f.bt_vert;
      al.bt_normals = c->d_tn;
      al.bending_model = MS_BEND_HELFRICH;  // bending_tilt_leaflet.py:448-450
      al.modules = (modules & ~MS_LEAFLET_MODS & ~MS_TILT_MODS) | MS_MOD_BENDING_TILT;
      {
        ProfScope ps(c, 0);
        HIPCHK(c, launch_energy(al, guard && use_dir, c->cap, c->til.max_ent, c->stream));
        ++c->ka_general;  // (bt_vert / bt_normals: never lean)
      }
      if (fused_tilt) continue;  // (its facet pass rides in the one launch below)
      int rc = bt_pass_f(c, f, write_factors ? 1 : 0, use_dir, alpha, use_dir ? f.trial : f.tilts);
      if (rc) return rc;
      if (write_factors) c->factors_leaflet = l;
    }
  }
  // the edge terms: gamma |e| of the tagged edges, then 0.5 k (|e| - L0)^2 of the charged ones, added into the
  // MS_S_ESURF partials the launch above has just written (k_energy stores that slot's partial for every tile of the
  // range whatever the module mask -- 0.0 without MS_MOD_SURFACE -- so the cell is defined before the add); the fold
  // below then carries surface + edge energy.  The order of the two adds into a cell is the table's
  for (int t = 0; t < 2; ++t)
    if (modules & kEdgeTerms[t].bit)
      if (int rc_e = edge_energy_run(c, t, use_dir, alpha)) return rc_e;
  if (modules & MS_TILT_MODS) {
    int rc = MS_OK;
    const double* tilts = c->tf[0].tilts;
    if (use_dir) {
      // minimizer.py:723-733: the trial energy is taken with the tilts projected onto the
      // TRIAL surface's vertex tangent planes (kept aside; they become the stored tilts
      // only if this trial is accepted)
      rc = tilt_pass(c, 2, true, alpha, c->tf[0].tilts, c->tf[0].trial);
      if (rc) return rc;
      tilts = c->tf[0].trial;
    }
    // energy only, both modules: the bending_tilt kernel sums the tilt-magnitude energy as well (tilt_eval does the same)
    const bool fuse = (modules & MS_MOD_TILT) && bt && !write_factors && c->tf[0].k_tilt != 0.0 && !c->tf[0].consistent;
    if (!fused_tilt) {
      if ((modules & MS_MOD_TILT) && !fuse) rc = tilt_pass(c, 0, use_dir, alpha, tilts);
      if (rc) return rc;
      if (bt) rc = bt_pass(c, write_factors ? 1 : 0, use_dir, alpha, tilts, fuse);
      if (rc) return rc;
      if (modules & MS_MOD_TILT_SMOOTH) rc = ts_pass(c, 0, use_dir, alpha, tilts);
      if (rc) return rc;
    }
  }
  for (int l = 1; l <= 2 && (modules & MS_LEAFLET_MODS); ++l) {  // leaflet fields, same protocol
    TiltField& f = c->tf[l];
    // (an add-on that reads the field is reason enough: the coupling's trial energy is taken with BOTH leaflets projected
    // onto the trial surface; bending_tilt alone is not: its passes ran above)
    if (!(modules & f.mods() & ~f.mod_bt)) continue;
    int rc = MS_OK;
    const double* tilts = f.tilts;
    if (use_dir) {
      if (!lbt) rc = tilt_pass_f(c, f, 2, true, alpha, f.tilts, f.trial);  // (done above otherwise)
      if (rc) return rc;
      tilts = f.trial;
    }
    if (modules & f.mod_dt) rc = disk_target_pass(c, f, 0, use_dir, alpha, tilts, false, false);
    if (rc) return rc;
    if (fused_tilt || fused_rest) continue;
    if (modules & f.mod_tilt) rc = tilt_pass_f(c, f, 0, use_dir, alpha, tilts);
    if (rc) return rc;
    if (modules & f.mod_smooth) rc = ts_pass_f(c, f, 0, use_dir, alpha, tilts);
    if (rc) return rc;
  }
  if (fused_tilt || fused_rest) {
    bool used = false;
    int rc = tilt_energy_pass(c, modules, use_dir, alpha, &used, /*dry=*/false, /*skip_bt=*/fused_rest);
    if (rc) return rc;
    if (!used) return fail(c, MS_ERR_STATE, "tilt energy pass: planned but not launched");
  }
  // the add-ons, behind whichever pass above wrote their slots' cells (k_tilt / k_tsmooth, or the one launch of
  // tilt_energy_pass); on a trial with the tilts projected onto it, the rings ordered on THIS evaluation's positions
  if (int rc_a = addon_passes(c, modules, {Phase::ENERGY, use_dir, alpha, /*trial_tilts=*/use_dir, false, nullptr})) return rc_a;
  if (reduce_now) {
    constexpr uint32_t core = (1u << MS_S_ESURF) | (1u << MS_S_VOL) | (1u << MS_S_EBEND) | (1u << MS_S_MINEDGE2) |
                              (1u << MS_S_GUARD);
    int rc = reduce_slots(c, tilt_only ? (energy_mask(modules) & ~core) : energy_mask(modules));
    if (rc) return rc;
  }
  if (bend && write_factors) c->carry.factors_valid = !use_dir;
  if (st.positions_only) return MS_OK;  // (no factor was written and no record: fK / fA and their owner are as they were)
  if (!lbt) c->factors_leaflet = 0;
  c->carry.bt_valid = (bt || lbt) && !use_dir;
  return MS_OK;
}

// The leaflet bending_tilt instance of k_gradient stages 12 doubles per patch row where the instances ms_create admits
// stage 8: on a patch that large the shape gradient of bending_tilt_in/out is refused here, by every entry point that
// would run it and before its first launch (the runtime would refuse the launch itself).  Everything else on the
// context -- energies, tilt gradients, the relaxations, other module sets -- does not use the instance and stays.
int leaflet_gradient_admit(ms_ctx* c, uint32_t modules) {
  if (!(modules & MS_LEAFLET_BT)) return MS_OK;
  const size_t need =
      leaflet_gradient_lds_bytes(c->til.T, c->cap, c->til.max_ent, (modules & MS_CON_VOLUME) != 0, !c->deterministic);
  if (need <= MS_LDS_CU) return MS_OK;
  return fail(c, MS_ERR_TILE_CAPACITY,
              "bending_tilt_in/out shape gradient: a vertex patch (tile + halo) of " + std::to_string(c->cap) +
                  " rows needs " + std::to_string(need) + " bytes of LDS, above the 160 KiB of a CU; "
                  "use a smaller tile_vertices");
}

// dir_mode: 0 = plain gradient pass (+ <g,gC> partials); 1/2 = fused direction (GD / CG history)
// may_skip_d: the caller reads D only after it has seen the direction scalars (ms_step) -- the pass may leave D unstored
int phase_gradient(ms_ctx* c, uint32_t modules_in, double* g_out, bool accumulate, int dir_mode = 0,
                   bool reduce_now = true, bool may_skip_d = false) {
  uint32_t modules = modules_in;
  if ((modules & (MS_MOD_BENDING | MS_MOD_BENDING_TILT | MS_LEAFLET_BT)) && !c->carry.factors_valid)
    return fail(c, MS_ERR_STATE, "gradient pass needs the bending factors of an energy pass at x");
  if (modules & MS_MOD_BENDING_TILT)  // k_bt finished the factors: K_C is the plain bending back-prop
    modules = (modules & ~MS_MOD_BENDING_TILT) | MS_MOD_BENDING;
  // leaflet bending_tilt: one back-propagation per leaflet (per-corner area factors), starting with the
  // leaflet whose factors the energy pass left in fK/fA; the other leaflet's energy + facet pass is redone
  int lbt_order[2] = {0, 0}, n_lbt = 0;
  if (modules & MS_LEAFLET_BT) {
    if (dir_mode) return fail(c, MS_ERR_STATE, "bending_tilt_in/out cannot use the fused direction pass");
    if (modules & MS_MOD_BENDING) return fail(c, MS_ERR_STATE, "bending together with bending_tilt_in/out is outside the device path");
    if (c->params.bending_grad_mode != MS_GRAD_ANALYTIC)
      return fail(c, MS_ERR_STATE, "bending_tilt_in/out: only bending_gradient_mode=analytic is on the device path");
    if (int rc_a = leaflet_gradient_admit(c, modules)) return rc_a;
    for (int l = 2; l >= 1; --l)
      if (modules & c->tf[l].mod_bt) lbt_order[n_lbt++] = l;
    if (n_lbt == 2 && c->factors_leaflet == lbt_order[1]) std::swap(lbt_order[0], lbt_order[1]);
    modules |= MS_MOD_BENDING;
  }
  GradientArgs a;
  a.m = device_mesh(c);
  a.tile0 = c->tile0;
  a.tile1 = c->tile1;
  a.x = c->buf[MS_BUF_X];
  a.fK = c->buf[MS_BUF_FK];
  a.fA = c->buf[MS_BUF_FA];
  a.g = g_out;
  a.gC = (modules & MS_CON_VOLUME) ? c->buf[MS_BUF_GC] : nullptr;
  a.partials = c->d_partials;
  a.scal = c->d_scal;
  a.modules = modules;
  a.bending_grad_mode = c->params.bending_grad_mode;
  a.volume_stiffness = c->params.volume_stiffness;
  a.target_volume = c->params.target_volume;
  a.area_stiffness = c->area_stiffness;
  a.target_area = c->target_area;
  a.accumulate = accumulate ? 1 : 0;
  a.dir_mode = dir_mode;
  // A direction with CG history right after one that was no descent direction is, in the steady state of the headline
  // workload, none either: the step fails without a trial and the stepper restarts along -g, so nobody reads D.  Such
  // a pass forms its rows for the scalars only (24 nv bytes less to store); ms_step and the buffer getter write D out
  // with k_direction in the rare case it is wanted after all (materialize_direction).  Only on the fused-epilogue lane
  // of a single context: no constraint row, no tilt shape module, no preconditioned direction.
  const bool skip_d = may_skip_d && dir_mode == 2 && c->shard_count == 1 && !c->last_hist_descent && !c->precond &&
                      !(modules & (MS_CON_VOLUME | MS_TILT_SHAPE_MODS)) && c->pin_lane != MS_PIN_LANE_PROJECT;
  a.d = skip_d ? nullptr : c->buf[MS_BUF_D];
  a.pg = c->buf[MS_BUF_PG];
  a.pd = c->buf[MS_BUF_PD];
  a.pd_neg_pg = (dir_mode == 2 && c->carry.pd_neg_pg) ? 1 : 0;
  a.gate = c->stage().cur_gate;
  a.gate_want = c->stage().cur_gate_want;
  a.atomic = c->deterministic ? 0 : 1;
  a.bt_vert = nullptr;
  a.tilts = nullptr;
  a.div_sign = 1.0;
  if (n_lbt == 0) {
    ProfScope ps(c, gradient_lean_instance(a) ? 9 : 1, a.gate, a.gate_want);
    HIPCHK(c, launch_gradient(a, c->cap, c->til.max_ent, c->stream));
  }
  // the edge terms: their rows added into the G that K_C has just written (before pin_grad_run projects the full gradient),
  // and the <g,gC> partials corrected by the change.  The direction scalars of K_C's fused epilogue would predate the
  // addition: the callers take the separate direction pass (queue_energy_and_gradient)
  if ((modules_in & MS_EDGE_MODS) && g_out) {
    // (both terms add into the same rows of G and the same <g,gC> cells, in the table's order)
    for (int t = 0; t < 2; ++t) {
      if (!(modules_in & kEdgeTerms[t].bit)) continue;
      if (dir_mode || a.gate != nullptr)
        return fail(c, MS_ERR_STATE, std::string(kEdgeTerms[t].name) + " cannot use the fused direction pass or a gated gradient pass");
      if (int rc_e = edge_grad_run(c, t, g_out, a.gC != nullptr)) return rc_e;
    }
  }
  for (int k = 0; k < n_lbt; ++k) {
    TiltField& f = c->tf[lbt_order[k]];
    if (c->factors_leaflet != lbt_order[k]) {
      // redo this leaflet's energy + facet pass at x (factors on): its own module only -- the other tilt modules'
      // energies are in their slots already -- and on the vertex normals the evaluation before left in d_tn (same x)
      c->lbt_normals_current = c->d_tn != nullptr;
      int rc = phase_energy(c, (modules_in & ~(MS_LEAFLET_MODS | MS_TILT_MODS)) | f.mod_bt, false, 0.0, false, false, true, false);
      c->lbt_normals_current = false;
      if (rc) return rc;
    }
    GradientArgs al = a;
    al.m.kappa = f.kappa;
    al.m.kc_uniform = 0;  // per-leaflet arrays
    al.m.c0 = f.c0;
    al.bt_vert = f.bt_vert;
    al.tilts = f.tilts;
    al.div_sign = f.div_sign;
    if (k > 0) {  // the other modules' gradient went in with the first leaflet
      al.modules = MS_MOD_BENDING;
      al.gC = nullptr;
      al.accumulate = 1;
    }
    {
      ProfScope ps(c, 1);
      HIPCHK(c, launch_gradient(al, c->cap, c->til.max_ent, c->stream));
    }
    int rc = bt_pass_f(c, f, 3, false, 0.0, f.tilts);  // + s dE/ddiv d(div)/dx
    if (rc) return rc;
  }
  if (dir_mode) {
    c->carry.last_g = g_out;
    c->carry.dir_implicit = false;  // D was written ...
    c->carry.dir_unwritten = skip_d;  // ... or is k_direction's to write from G / PG / PD
  }
  bool added_after = n_lbt > 0;
  for (int k = 0; k < 3 && g_out; ++k) {  // module loop: the tilt magnitude modules add their shape gradient into g
    TiltField& f = c->tf[k];
    if (modules & f.mod_tilt) {
      int rc = tilt_pass_f(c, f, 1, false, 0.0);
      if (rc) return rc;
      added_after = true;
    }
    if (k > 0 && (modules & f.mod_dt)) {
      int rc = disk_target_pass(c, f, 1, false, 0.0, f.tilts, true, false);
      if (rc) return rc;
      added_after = true;
    }
  }
  // the add-ons: where k_tilt<1> above has written a slot's partials again (the energy fold of this evaluation may still
  // be ahead: queue_energy_and_gradient) their sums go in once more, and the ones with a shape gradient add it into g
  if (int rc = addon_passes(c, modules, {Phase::GRADIENT, false, 0.0, false, false, g_out})) return rc;
  added_after = added_after || (g_out && (modules & MS_LEAFLET_ADDONS & MS_TILT_SHAPE_MODS));
  // the gradient kernel's <g, gC> partials predate those additions: take them again of the complete gradient
  if (added_after && g_out && (modules & MS_CON_VOLUME))
    HIPCHK(c, launch_row_dot(c->tile0, c->tile1, c->til.nv, c->til.own, g_out, c->buf[MS_BUF_GC], c->d_partials,
                             c->til.n_tiles, c->stream));
  if (reduce_now) return reduce_slots(c, dir_mode ? MASK_DIR : MASK_GRAD);
  return MS_OK;
}

int phase_direction(ms_ctx* c, int stepper, bool use_history, bool g_finalized = false) {
  // (pins in the skip lane: the reference's KKT solve returned before touching g, the volume row included)
  // (the area lane: G was projected against every row behind the gradient pass, area_project_gradient)
  const bool use_con = (c->params.modules & MS_CON_VOLUME) != 0 && c->pin_lane != MS_PIN_LANE_SKIP && !area_row_active(c);
  const StageCtl& st = c->stage();
  c->carry.dir_implicit = false;
  c->carry.dir_unwritten = false;
  {
  ProfScope ps(c, 2, st.cur_gate, st.cur_gate_want);
  HIPCHK(c, launch_direction(c->tile0, c->tile1, c->til.nv, c->til.own, c->d_vflags, c->buf[MS_BUF_G],
                             c->buf[MS_BUF_GC], c->buf[MS_BUF_D], c->buf[MS_BUF_PG],
                             c->buf[MS_BUF_PD], c->d_scal, use_con ? 1 : 0,
                             (stepper == MS_STEPPER_CG && use_history) ? 1 : 0, c->d_partials,
                             c->til.n_tiles, (g_finalized && !use_con) ? 0 : 1, c->stream, st.cur_gate,
                             st.cur_gate_want,
                             // (the previous direction was an implicit -PG: the kernel derives it, as the fused epilogue does)
                             (stepper == MS_STEPPER_CG && use_history && c->carry.pd_neg_pg) ? 1 : 0,
                             (stepper == MS_STEPPER_CG && c->precond) ? 1 : 0));
  }
  c->carry.last_g = c->buf[MS_BUF_G];
  return reduce_slots(c, MASK_DIR);
}

// The last fused direction pass left D unstored (CarryState::dir_unwritten) and somebody wants the rows after all:
// k_direction on the finalized G, with the history that pass had, repeats the epilogue's arithmetic row for row.  No
// fold: the pass's scalars are the host's already (the partials this launch writes are the same sums again).
// `flag` is the carried one, or the one of a pass still queued behind an acceptance (ms_ctx::kc_dir_unwritten).
int materialize_direction(ms_ctx* c, bool& flag) {
  if (!flag) return MS_OK;
  HIPCHK(c, launch_direction(c->tile0, c->tile1, c->til.nv, c->til.own, c->d_vflags, c->buf[MS_BUF_G], c->buf[MS_BUF_GC],
                             c->buf[MS_BUF_D], c->buf[MS_BUF_PG], c->buf[MS_BUF_PD], c->d_scal, 0, /*cg_history=*/1,
                             c->d_partials, c->til.n_tiles, /*write_g=*/0, c->stream, nullptr, 0,
                             c->carry.pd_neg_pg ? 1 : 0, 0));
  flag = false;
  ++c->dir_materialized;
  return MS_OK;
}
int materialize_direction(ms_ctx* c) { return materialize_direction(c, c->carry.dir_unwritten); }

// host-side write of a slot (a stage mailbox's result moved into the main one): both the host copy and the value
// word, so a later take_mailbox() keeps it
void put_mailbox(ms_ctx* c, int sl, double v) {
  c->h_scal[sl] = v;
  unsigned long long bits;
  memcpy(&bits, &v, sizeof(double));
  __atomic_store_n(&c->h_seq[2 * sl], bits, __ATOMIC_RELAXED);
  // (the entry keeps validating against the ticket it carried: tag = value XOR ticket, see wait_mailbox)
  __atomic_store_n(&c->h_seq[2 * sl + 1], bits ^ c->expected[sl], __ATOMIC_RELAXED);
}

const char* box_name(ms_ctx* c, const void* h_seq);
bool trace_queue();

// a fold found that a gated launch had run on part of its workgroups only (FoldArgs::check_ran): never continue
int check_queue_error(ms_ctx* c) {
  if (!c->h_err) return MS_OK;
  const unsigned long long e = __atomic_load_n(c->h_err, __ATOMIC_ACQUIRE);
  if (e == 0) return MS_OK;
  __atomic_store_n(c->h_err, 0ull, __ATOMIC_RELEASE);  // reported once (the caller gets MS_ERR_STATE for this call)
  char msg[256];
  snprintf(msg, sizeof(msg),
           "line-search queue: a gated launch ran on %llu of its %d workgroups (fold ticket %llu): the workgroups of one "
           "launch did not read the same decision word",
           e & 0xffffffull, c->tile1 - c->tile0, (e >> 24) & 0xffffffffull);
  return fail(c, MS_ERR_STATE, msg);
}

// wait until every entry of a mailbox carries the ticket of the latest fold queued for it; *vals (optional) receives
// the MS_NSCAL slot values, *code the decision entry
int wait_mailbox(ms_ctx* c, unsigned long long* h_seq, const unsigned long long* expected, double* vals,
                 uint32_t* code) {
  // an entry has arrived when value XOR tag is the ticket waited for (k_reduce: post_entry); the value word read for
  // that test is the one handed out
  unsigned long long bits[MS_MB_WORDS];
  auto arrived = [&]() {
    for (int sl = 0; sl < MS_MB_WORDS; ++sl) {
      if (expected[sl] == 0) continue;
      const unsigned long long tag = __atomic_load_n(&h_seq[2 * sl + 1], __ATOMIC_ACQUIRE);
      bits[sl] = __atomic_load_n(&h_seq[2 * sl], __ATOMIC_ACQUIRE);
      if ((bits[sl] ^ tag) != expected[sl]) return false;
    }
    return true;
  };
  // (an empty shard -- 9 tiles over 8 ranks leave ranks 5..7 without one -- waits like any other: k_reduce posts the
  // neutral value of every slot for an empty tile range, and `bits` is only ever filled by arrived())
  bool done = false;
  if (int rc_f = exec_flush(c)) return rc_f;  // (one-tile contexts: what was recorded runs now)
  for (long spin = 0; !done && spin < 20000000L; ++spin) {
    done = arrived();
    if (done) {
      if (g_host_timing.on && spin > 0) {  // (only when the host really waited: the GPU was the one ahead)
        g_host_timing.t_fetch = HostTiming::now();
        g_host_timing.armed = true;
      }
      break;
    }
    __builtin_ia32_pause();
  }
  if (!done) {
    HIPCHK(c, hipStreamSynchronize(S(c)));
    // everything queued has run: an entry that is still behind belongs to a gated fold that found its gate closed
    // although the host expected it to run -- host and device disagreed on an Armijo test.  Never continue on that.
    if (!arrived()) {
      int rc = check_queue_error(c);
      if (rc) return rc;
      int sl = 0;
      while (sl < MS_MB_WORDS - 1 && (expected[sl] == 0 || ((__atomic_load_n(&h_seq[2 * sl], __ATOMIC_ACQUIRE) ^
                                                              __atomic_load_n(&h_seq[2 * sl + 1], __ATOMIC_ACQUIRE)) == expected[sl])))
        ++sl;
      char msg[384];
      snprintf(msg, sizeof(msg),
               "line-search queue: a gated launch the host waited for did not run (mailbox %s, entry %d: ticket %llu "
               "found, %llu expected; latest ticket %llu)",
               box_name(c, h_seq), sl,
               (unsigned long long)(__atomic_load_n(&h_seq[2 * sl], __ATOMIC_ACQUIRE) ^ __atomic_load_n(&h_seq[2 * sl + 1], __ATOMIC_ACQUIRE)),
               (unsigned long long)expected[sl], (unsigned long long)c->ticket);
      ++c->queue_mismatches;
      return fail(c, MS_ERR_STATE, msg);
    }
  }
  int rc = check_queue_error(c);
  if (rc) return rc;
  if (vals)
    for (int sl = 0; sl < MS_NSCAL; ++sl) {
      // (entries nobody waited for keep whatever an earlier fold or put_mailbox left in their value word)
      const unsigned long long b = expected[sl] ? bits[sl] : __atomic_load_n(&h_seq[2 * sl], __ATOMIC_RELAXED);
      memcpy(&vals[sl], &b, sizeof(double));
    }
  if (code) *code = expected[MS_MB_DEC] ? (uint32_t)bits[MS_MB_DEC] : (uint32_t)__atomic_load_n(&h_seq[2 * MS_MB_DEC], __ATOMIC_RELAXED);
  return MS_OK;
}

// k_reduce mirrors every slot it folds into the pinned mailbox and then bumps that slot's
// sequence word; fetching = spinning on those words (a few microseconds less than waking up
// from hipStreamSynchronize).  Falls back to a stream sync after ~50 ms of spinning.
int fetch(ms_ctx* c, uint32_t* code = nullptr) {
  if (trace_queue()) {
    unsigned long long mx = 0;
    for (int sl = 0; sl < MS_MB_WORDS; ++sl) mx = std::max<unsigned long long>(mx, c->expected[sl]);
    fprintf(stderr, "[msq] fetch %s (latest expected ticket %llu)\n", box_name(c, c->h_seq), mx);
  }
  return wait_mailbox(c, c->h_seq, c->expected, c->h_scal, code);
}

// the host's decision against the device's (the code the fold posted next to the energies it decided on)
int verify_decision(ms_ctx* c, uint32_t host_code, uint32_t dev_code, const char* where) {
  if (host_code == dev_code) return MS_OK;
  ++c->queue_mismatches;
  char msg[256];
  snprintf(msg, sizeof(msg), "line-search queue: host and device took different decisions at %s (host %u, device %#x)",
           where, host_code, dev_code);
  return fail(c, MS_ERR_STATE, msg);
}

// volume penalty (modules/energy/volume.py:94-128) + body-area penalty (modules/energy/body_area_penalty.py:136-137)
double penalty_energy(const ms_ctx* c, double V, double A) {
  double e = 0.0;
  if (c->params.modules & MS_MOD_VOLUME_PENALTY) {
    const double delta = V - c->params.target_volume;
    e = 0.5 * c->params.volume_stiffness * (delta * delta);
  }
  if (c->params.modules & MS_MOD_AREA_PENALTY) {
    const double delta = A - c->target_area;
    const double ea = 0.5 * c->area_stiffness * delta * delta;
    e = (c->params.modules & MS_MOD_VOLUME_PENALTY) ? e + ea : ea;
  }
  return e;
}

// energies from the pinned mailbox: {surface, bending, penalty, tilt}
void energies_from_mailbox(const ms_ctx* c, double e[4]) {
  // (the edge modules' energies ride in the surface slot: their energy kernels add into that slot's partials)
  e[0] = (c->params.modules & (MS_MOD_SURFACE | MS_EDGE_MODS)) ? c->h_scal[MS_S_ESURF] : 0.0;
  e[1] = (c->params.modules & MS_MOD_BENDING) ? c->h_scal[MS_S_EBEND] : 0.0;
  if (c->params.modules & MS_MOD_BENDING_TILT) e[1] += c->h_scal[MS_S_EBT];
  e[2] = penalty_energy(c, c->h_scal[MS_S_VOL], c->h_scal[MS_S_AREA]);
  e[3] = (c->params.modules & MS_MOD_TILT) ? c->h_scal[MS_S_ETILT] : 0.0;
  if (c->params.modules & MS_MOD_TILT_SMOOTH) e[3] += c->h_scal[MS_S_ETS];
  for (int l = 1; l <= 2; ++l) {
    const TiltField& f = c->tf[l];
    if (c->params.modules & f.etilt_mods()) e[3] += c->h_scal[f.s_etilt];  // (the slot's add-ons ride in it)
    if (c->params.modules & f.ets_mods()) e[3] += c->h_scal[f.s_ets];
    if (c->params.modules & f.mod_bt) e[1] += c->h_scal[f.s_ebt];
    if (c->params.modules & f.mod_dt) e[3] += c->h_scal[f.s_edt];
  }
}

// gradient assembly at x: energy pass (+factors), gradient pass, finalize via
// the direction kernel (projection + fixed rows), everything queued async.
// skip_energy: the accepted trial of the previous step already was this energy pass (same
// kernel, same x: its factors are in fK/fA, its scalars in d_scal and in the mailbox).
int queue_energy_and_gradient(ms_ctx* c, int stepper, bool use_history, bool skip_energy = false) {
  const uint32_t mods = c->params.modules;
  // lambda needs a global reduction first; the tilt module adds into g after K_C
  // (and a preconditioned direction -- conjugate_gradient.py:74-76 -- is the direction kernel's)
  // (the edge modules add into g after K_C as well: |g|^2, <g,d> and max|g_i|^2 are taken over the completed G)
  const bool constraint = (mods & (MS_CON_VOLUME | MS_TILT_SHAPE_MODS | MS_EDGE_MODS)) != 0 ||
                          (stepper == MS_STEPPER_CG && c->precond) || c->pin_lane == MS_PIN_LANE_PROJECT || area_row_active(c);
  // K_C reads the reduced volume / body area (already reduced when the energy pass is skipped)
  const bool penalty = skip_energy || (mods & (MS_MOD_VOLUME_PENALTY | MS_MOD_AREA_PENALTY)) != 0;
  int rc = leaflet_gradient_admit(c, mods);  // (before the energy pass: a refusal launches nothing)
  if (rc) return rc;
  if (!skip_energy) rc = phase_energy(c, mods, false, 0.0, false, false, true, /*reduce_now=*/penalty);
  if (rc) return rc;
  if (!constraint) {
    // no row to project out: the direction pass rides in K_C's epilogue, one reduce for all
    const int dir_mode = (stepper == MS_STEPPER_CG && use_history) ? 2 : 1;
    rc = phase_gradient(c, mods, c->buf[MS_BUF_G], false, dir_mode, /*reduce_now=*/false, /*may_skip_d=*/true);
    if (rc) return rc;
    return reduce_slots(c, (penalty ? 0u : energy_mask(mods)) | MASK_DIR);
  }
  rc = phase_gradient(c, mods, c->buf[MS_BUF_G], false, 0, /*reduce_now=*/false);
  if (rc) return rc;
  rc = pin_grad_run(c, (mods & MS_CON_VOLUME) != 0);  // (project lane only)
  if (rc) return rc;
  if (area_row_active(c)) {  // (the area lane: one or two rows projected out here, none by k_direction)
    rc = area_project_gradient(c);
    if (rc) return rc;
  }
  // (<g,gC> / <gC,gC> exist only with a row or a tilt module behind K_C)
  const uint32_t gmask = (mods & (MS_CON_VOLUME | MS_TILT_SHAPE_MODS)) ? MASK_GRAD : 0u;
  const uint32_t fmask = (penalty ? 0u : energy_mask(mods)) | gmask;
  if (fmask) rc = reduce_slots(c, fmask);
  if (rc) return rc;
  return phase_direction(c, stepper, use_history);
}

template <typename Tp>
int upload(ms_ctx* c, Tp** dst, const std::vector<Tp>& src, size_t min_elems = 1) {
  size_t n = src.size() > min_elems ? src.size() : min_elems;
  HIPCHK(c, hipMalloc(reinterpret_cast<void**>(dst), n * sizeof(Tp)));
  if (!src.empty())
    HIPCHK(c, hipMemcpy(*dst, src.data(), src.size() * sizeof(Tp), hipMemcpyHostToDevice));
  return MS_OK;
}

// a setter's table (ms_table_blob.h) as one allocation; the sections' pointers are b.at(*dst, handle)
int upload_table(ms_ctx* c, TableBlob& b, void** dst) {
  HIPCHK(c, hipMalloc(dst, b.bytes()));
  HIPCHK(c, hipMemcpy(*dst, b.image(), b.bytes(), hipMemcpyHostToDevice));
  return MS_OK;
}

// ... and the end of one: no launch still reads it once the stream has drained
int drop_table(ms_ctx* c, void*& d_table) {
  if (!d_table) return MS_OK;
  HIPCHK(c, hipStreamSynchronize(S(c)));
  HIPCHK(c, hipFree(d_table));
  d_table = nullptr;
  return MS_OK;
}

int ext_to_patch(ms_ctx* c, const double* host, double* dst, int ncomp) {
  const size_t bytes = sizeof(double) * (size_t)c->til.nv * ncomp;
  HIPCHK(c, hipMemcpyAsync(c->d_stage, host, bytes, hipMemcpyHostToDevice, S(c)));
  HIPCHK(c, launch_permute_in(c->til.nv, c->d_perm, c->d_stage, dst, ncomp, c->stream));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

int patch_to_ext(ms_ctx* c, const double* src, double* host, int ncomp) {
  const size_t bytes = sizeof(double) * (size_t)c->til.nv * ncomp;
  HIPCHK(c, launch_permute_out(c->til.nv, c->d_perm, src, c->d_stage, ncomp, c->stream));
  HIPCHK(c, hipMemcpyAsync(host, c->d_stage, bytes, hipMemcpyDeviceToHost, S(c)));
  HIPCHK(c, hipStreamSynchronize(S(c)));
  return MS_OK;
}

}  // namespace

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  template <typename Tp>
  Tp* as() {
    return static_cast<Tp*>(p);
  }
};
#define SEAM_HIP(call)                                                         \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) return fail_hip(nullptr, e_, #call);                 \
  } while (0)
}  // namespace
