/*
 * membrane_hip.h -- C ABI of libmembrane_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of AvishaiBarnoy/membrane_solver: the
 * per-iteration energy + gradient assembly (surface tension, Helfrich /
 * Willmore bending, volume penalty + volume-constraint row) and the GD / CG
 * steppers with Armijo backtracking that consume it.  Reference citations are
 * relative to the reference checkout.
 *
 * Conventions
 *   - plain C types only; all host arrays are row-major, positions/gradients
 *     (nv,3) double, triangle rows (nf,3) int32 zero based -- the layouts of
 *     Mesh.positions_view (geometry/mesh.py:372-389) and
 *     Mesh.triangle_row_cache (geometry/mesh.py:597-624).  A row-major (n,3)
 *     array is byte-identical to the (3,n) Fortran-order arrays the
 *     reference's f2py kernels take, so the same pointers serve both seams.
 *   - every function returns MS_OK (0) or a negative MS_ERR_*; nothing
 *     throws; ms_last_error() gives the text.  No global mutable state but
 *     the last-error string of failed ms_create calls.
 *   - one context per device/process; a context is not thread-safe (the
 *     reference is single threaded).
 *   - all state lives in HBM between calls; host arrays cross PCIe only in
 *     the ms_set_* / ms_get_* calls and the *_host seam calls.
 */
#ifndef MEMBRANE_HIP_H
#define MEMBRANE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_OK 0
#define MS_ERR_INVALID (-1)       /* bad argument / shape                      */
#define MS_ERR_HIP (-2)           /* a HIP runtime call failed                 */
#define MS_ERR_TILE_CAPACITY (-3) /* a vertex patch does not fit LDS / uint16  */
#define MS_ERR_STATE (-4)         /* call order (e.g. gradient before energy)  */
#define MS_ERR_NOMEM (-5)
#define MS_ERR_UNSUPPORTED (-6)   /* a case the device path does not take       */

/* energy-module bits (modules/energy/{surface,bending,volume}.py) */
#define MS_MOD_SURFACE 1u
#define MS_MOD_BENDING 2u
#define MS_MOD_VOLUME_PENALTY 4u /* modules/energy/volume.py:94-128            */
/* constraint row: modules/constraints/volume.py:43-66 + the k==1 dense KKT
 * branch of runtime/constraint_manager.py:293-301 */
#define MS_CON_VOLUME 8u
/* also reduce the body volume in energy passes (the Lagrange volume-drift
 * check of runtime/minimizer.py:1478-1513 needs V even when no volume module
 * is loaded); no effect on energies or gradients */
#define MS_TRACK_VOLUME 16u
/* vertex-tilt magnitude energy 1/2 k_t sum |t_v|^2 A_v (modules/energy/tilt.py:99-172) */
#define MS_MOD_TILT 32u
#define MS_MOD_BENDING_TILT 64u /* modules/energy/bending_tilt.py (replaces MS_MOD_BENDING) */
#define MS_MOD_TILT_SMOOTH 128u /* modules/energy/tilt_smoothness.py (ambient_v1 transport) */
/* two-leaflet tilt fields (Mesh.tilts_in_view / tilts_out_view): tilt magnitude
 * (modules/energy/tilt_in.py, tilt_out.py -> tilt_leaflet.py:26-169) and tilt smoothness
 * (tilt_smoothness_in.py, tilt_smoothness_out.py -> tilt_smoothness_leaflet.py:17-79) */
#define MS_MOD_TILT_IN 256u
#define MS_MOD_TILT_OUT 512u
#define MS_MOD_TILT_SMOOTH_IN 1024u
#define MS_MOD_TILT_SMOOTH_OUT 2048u
/* leaflet bending + tilt-splay coupling (modules/energy/bending_tilt_in.py, bending_tilt_out.py ->
 * bending_tilt_leaflet.py:231-758, default options, analytic gradient mode) */
#define MS_MOD_BENDING_TILT_IN 4096u
#define MS_MOD_BENDING_TILT_OUT 8192u
/* soft disk tilt-profile target (modules/energy/tilt_disk_target_in.py:160-286, tilt_disk_target_out.py) */
#define MS_MOD_TILT_DISK_TARGET_IN 16384u
#define MS_MOD_TILT_DISK_TARGET_OUT 32768u
/* soft body-area penalty E = 1/2 k (A - A0)^2 over the body's facets (modules/energy/body_area_penalty.py:100-145);
 * k and A0 come from ms_set_area_penalty.  Its gradient k (A - A0) dA/dx is an effective surface tension on the
 * facets that carry the body flag (geometry/facet.py:168-249: the surface term's normal and 1e-12 clamp). */
#define MS_MOD_AREA_PENALTY 65536u
/* line tension E = sum gamma |e| over the tagged edges (modules/energy/line_tension.py:103-140); the edges and their
 * gamma come from ms_set_line_tension.  Its energy is added into the surface slot (MS_S_ESURF, energies[0]) behind the
 * energy pass, its gradient into G behind the gradient pass: two extra launches, no reduction slot of its own. */
#define MS_MOD_LINE_TENSION 131072u
/* edge length penalty E = sum 0.5 k (|e| - L0)^2 over the edges that carry a target length
 * (modules/energy/edge_length_penalty.py:35-69); the edges, their L0 and k come from ms_set_edge_length_penalty.  Like
 * line tension its energy is added into the surface slot (MS_S_ESURF, energies[0]) behind the energy pass, its gradient
 * into G behind the gradient pass, each behind line tension's launch when both are on: no reduction slot of its own. */
#define MS_MOD_EDGE_LENGTH_PENALTY 262144u
/* soft contact term on an inclusion rim E = -sum gamma L 1/2 (t_tail + t_head) . r_hat over the rim edges
 * (modules/energy/tilt_rim_source_in.py:371-451, tilt_rim_source_out.py); the edges, their gamma and the circle's
 * frame come from ms_set_leaflet_rim_source.  Tilt gradient only.  Its sums are added into the leaflet's tilt-magnitude
 * slot (MS_S_ETILT_IN / MS_S_ETILT_OUT, energies[3]) behind the pass that writes it: no reduction slot of its own. */
#define MS_MOD_TILT_RIM_SOURCE_IN 524288u
#define MS_MOD_TILT_RIM_SOURCE_OUT 1048576u
/* inter-leaflet coupling E = 1/2 k_c int |t_out + s t_in|^2 dA, s = -1 ("difference") or +1 ("sum")
 * (modules/energy/tilt_coupling.py:114-262): per facet with |n| >= 1e-12, coeff = 0.5 k_c ((q0 + q1 + q2) / 3) with
 * q_v = |t_out,v + s t_in,v|^2, E = sum coeff A_f; shape gradient coeff dA_f/dv_k; tilt gradients k_c d_v A_v (out) and
 * k_c s d_v A_v (in).  Modulus and sign come from ms_set_tilt_coupling.  Its sums are added into the outer leaflet's
 * tilt-magnitude slot (MS_S_ETILT_OUT, energies[3]) behind the passes that write it: no reduction slot of its own.
 * Reads both leaflet fields; single context only; not together with a single-field tilt module. */
#define MS_MOD_TILT_COUPLING 2097152u
/* split splay / twist tilt-gradient energy of the inner leaflet (modules/energy/tilt_splay_twist_in.py:113-252,
 * ambient_v1 transport, native divergence): per facet n = (v1 - v0) x (v2 - v0), g_k = (n x e_k) / max(n.n, 1e-20),
 * div = sum t_k . g_k, curl_n = (sum g_k x t_k) . n_hat, E = 1/2 sum A_f (k_splay div^2 + k_twist curl_n^2); tilt
 * gradient A_f k_splay div g_k + A_f k_twist curl_n (n_hat x g_k); no shape gradient.  The moduli come from
 * ms_set_tilt_splay_twist.  Its sums are added into the inner leaflet's smoothness slot (MS_S_ETS_IN, energies[3])
 * behind the pass that writes it: no reduction slot of its own.  Single context only; not together with a single-field
 * tilt module, nor with pins or the volume enforcer on the line search. */
#define MS_MOD_TILT_SPLAY_TWIST_IN 4194304u
/* soft contact term on an inclusion rim that drives the bilayer boundary mode theta_B = theta_in + theta_out
 * (modules/energy/tilt_rim_source_bilayer.py:416-515): E = -sum gamma L (1/2 (t_in,tail + t_in,head) +
 * 1/2 (t_out,tail + t_out,head)) . r_hat over the rim edges; the same vector -1/2 gamma L r_hat goes into BOTH tilt
 * gradients at both ends; no shape gradient.  The edges, their gamma and the circle's frame come from
 * ms_set_rim_source_bilayer: one table and one apply pass serve both fields.  Its sums are added into the outer leaflet's
 * tilt-magnitude slot (MS_S_ETILT_OUT, energies[3]) behind the passes that write it (tilt_out, tilt_rim_source_out) and
 * ahead of tilt_coupling: no reduction slot of its own.  Reads both leaflet fields; single context only; not together
 * with a single-field tilt module. */
#define MS_MOD_TILT_RIM_SOURCE_BILAYER 8388608u
/* contact work of the inner leaflet's boundary mode theta_B on an inclusion's ring of vertices
 * (modules/energy/tilt_thetaB_contact_in.py:200-268 geometry, :336-405 energy): the ring rows are ordered by angle in
 * the frame of the current positions AT EVERY EVALUATION, w_i = 1/2 (|p_next - p_i| + |p_i - p_prev|) around the closed
 * ring, r_hat_i the in-plane unit vector from the center, theta_i = t_in,i . r_hat_i, R_eff = sum w |r| / wsum.
 * E = -2 pi R_eff gamma theta_B ("scalar" work mode, no gradient) or -2 pi R_eff gamma (sum w theta / wsum)
 * ("field_linear", tilt gradient -(2 pi R_eff gamma / wsum) w_i r_hat_i), plus 1/2 k sum w (theta - theta_B)^2 with tilt
 * gradient k w_i (theta_i - theta_B) r_hat_i in the legacy penalty mode.  No shape gradient; the outer leaflet is not
 * touched.  Rows, frame and strengths come from ms_set_thetab_contact, theta_B from ms_set_thetab_value.  Its sums are
 * added into the inner leaflet's tilt-magnitude slot (MS_S_ETILT_IN, energies[3]) behind the passes that write it
 * (tilt_in, tilt_rim_source_in): no reduction slot of its own.  Single context only; not together with a single-field
 * tilt module. */
#define MS_MOD_TILT_THETAB_CONTACT_IN 16777216u
/* constraint row of the hard body-area constraint (modules/constraints/body_area.py:28-84): dA/dx over the body's
 * facets takes part in the KKT projection of the gradient -- alone (constraint_manager.py:293-301), or behind the
 * volume row in the 2 x 2 solve of runtime/constraint_projection.py:101-129.  Needs ms_set_area_constraint(MS_AREA_BODY);
 * without it the bit does nothing.  ms_set_params keeps the bit out of the word the kernels read. */
#define MS_CON_BODY_AREA 33554432u
/* rim matching of the outer leaflet (modules/energy/rim_slope_match_out.py:352-629, modes pointwise_radial_v1 and
 * ring_average_radial_v1): three tagged rings (rim, outer, optional disk) are ordered by angle from the positions of
 * EVERY evaluation and rim and outer entries paired by index (unequal counts: the outer positions interpolated at the
 * rim's arc-length parameters); phi = (h_out - h_rim) / (r_out - r_rim), E = 1/2 k sum w (t_out . r_hat - phi)^2 and,
 * with a disk ring, + 1/2 k sum w (t_in . r_hat - (theta_disk - phi))^2.  Tilt gradients on the rim rows of both
 * leaflets and on the disk rows of the inner one; a shape gradient along the normal on the rim and outer rows.  Rows,
 * frame and strength come from ms_set_rim_match.  The out term is added into the outer leaflet's tilt-magnitude slot
 * (MS_S_ETILT_OUT), the in term into the inner one's (MS_S_ETILT_IN), behind every pass that writes them: no reduction
 * slot of its own.  Single context only; not together with a single-field tilt module. */
#define MS_MOD_RIM_SLOPE_MATCH_OUT 67108864u
#define MS_LEAFLET_IN 0
#define MS_LEAFLET_OUT 1

/* bending_params.py:19-33 */
#define MS_BEND_HELFRICH 0
#define MS_BEND_WILLMORE 1
#define MS_GRAD_ANALYTIC 0
#define MS_GRAD_APPROX 1

#define MS_STEPPER_GD 0 /* runtime/steppers/gradient_descent.py:35-84        */
#define MS_STEPPER_CG 1 /* runtime/steppers/conjugate_gradient.py:52-119     */

typedef struct ms_ctx ms_ctx;

/* Names of the device-resident per-vertex buffers (internal patch order). */
enum ms_buffer {
  MS_BUF_X = 0,     /* positions                      (nvp,3) */
  MS_BUF_XT = 1,    /* trial positions                (nvp,3) */
  MS_BUF_G = 2,     /* gradient                       (nvp,3) */
  MS_BUF_GC = 3,    /* volume-constraint row dV/dx    (nvp,3) */
  MS_BUF_D = 4,     /* search direction               (nvp,3) */
  MS_BUF_PG = 5,    /* CG history: previous gradient  (nvp,3) */
  MS_BUF_PD = 6,    /* CG history: previous direction (nvp,3) */
  MS_BUF_FK = 7,    /* bending: factor_K_vec          (nvp,3) */
  MS_BUF_FA = 8,    /* bending: fA_eff, fA_vor        (nvp,2) */
  MS_BUF_SCAL = 9,  /* reduction scalars              (MS_NSCAL) */
  MS_BUF_COUNT = 10
};

/* Reduction scalars produced on the device (ms_fetch_scalars). */
enum ms_scalar {
  MS_S_ESURF = 0,   /* sum gamma_f A_f                                  */
  MS_S_VOL = 1,     /* body volume, geometry/body.py:104-123            */
  MS_S_EBEND = 2,   /* bending energy, modules/energy/bending.py:117-144 */
  MS_S_MINEDGE2 = 3, /* min squared edge length, runtime/topology.py:174  */
  MS_S_GUARD = 4,   /* >0: normal-rotation guard tripped, topology.py:13  */
  MS_S_GGC = 5,     /* <g, gC>                                          */
  MS_S_GCGC = 6,    /* <gC, gC>                                         */
  MS_S_GNORM2 = 7,  /* |g|^2 after projection and fixed-row zeroing     */
  MS_S_GDOTD = 8,   /* <g, d>                                           */
  MS_S_MAXD2 = 9,   /* max_i |d_i|^2 over movable rows                  */
  MS_S_ETILT = 10,  /* tilt magnitude energy, modules/energy/tilt.py    */
  MS_S_EBT = 11,    /* bending + tilt-splay energy, modules/energy/bending_tilt.py */
  MS_S_TGNORM2 = 12, /* |tilt gradient|^2 over free rows (tilt_relaxation.py:318) */
  MS_S_TRZ = 13,    /* <r, M^-1 r> of the tilt CG (tilt_relaxation.py:369,416) */
  MS_S_MAXG2 = 14,  /* max_i |g_i|^2 over movable rows (= max|d_i|^2 of a steepest-descent restart) */
  MS_S_ETS = 15,    /* tilt smoothness (Dirichlet) energy, modules/energy/tilt_smoothness.py */
  MS_S_ETILT_IN = 16,  /* leaflet energies: tilt_in / tilt_out / tilt_smoothness_in / _out */
  MS_S_ETILT_OUT = 17,
  MS_S_ETS_IN = 18,
  MS_S_ETS_OUT = 19,
  MS_S_TGNORM2_IN = 20, /* leaflet relaxation: |grad|^2 and <r, M^-1 r> per leaflet; the driver */
  MS_S_TGNORM2_OUT = 21, /* adds the two (tilt_relaxation.py:862-868, 1139-1141)               */
  MS_S_TRZ_IN = 22,
  MS_S_TRZ_OUT = 23,
  MS_S_EBT_IN = 24,  /* bending_tilt_in / bending_tilt_out energies */
  MS_S_EBT_OUT = 25,
  MS_S_EDT_IN = 26,  /* tilt_disk_target_in / _out energies */
  MS_S_EDT_OUT = 27,
  MS_S_DTR_IN = 28,  /* largest in-plane distance of a disk row (the default disk radius), max-reduced */
  MS_S_DTR_OUT = 29,
  MS_S_AREA = 30,   /* area of the body's facets (MS_MOD_AREA_PENALTY), modules/energy/body_area_penalty.py:125-132 */
  MS_NSCAL = 31     /* slot masks are uint32_t (1u << slot) and bit MS_NSCAL marks the partials' "ran" row: ONE slot is
                     * left before the masks have to widen */
};

typedef struct ms_params {
  uint32_t modules;        /* MS_MOD_* | MS_CON_VOLUME                          */
  int bending_model;       /* MS_BEND_*                                         */
  int bending_grad_mode;   /* MS_GRAD_*                                         */
  double volume_stiffness; /* penalty mode k                                    */
  double target_volume;    /* V0 (penalty energy and constraint target)         */
} ms_params;

typedef struct ms_stepper_params {
  int stepper;             /* MS_STEPPER_*                                      */
  int max_iter;            /* Armijo trials, default 10                         */
  double beta;             /* backtrack factor 0.7                              */
  double c;                /* Armijo slope 1e-4                                 */
  double gamma;            /* growth 1.5                                        */
  double alpha_max_factor; /* 10                                                */
  int restart_interval;    /* CG restart, 10                                    */
  double edge_fraction;    /* gp["shape_step_edge_fraction"], 0 = off           */
  int reuse_energy0;       /* 0: re-evaluate energy0 like line_search.py:294;
                              1: reuse the energy of the gradient evaluation;
                              2: 1 + an accepted trial pass (which also writes the
                                 bending factors) serves as the next step's energy
                                 pass.  Same kernel on the same doubles: all three
                                 modes give bitwise identical trajectories.       */
  int enforce_volume;      /* line_search.py:428-487 with constraint_enforcer =
                              Minimizer._enforce_constraints (minimizer.py:1379) and
                              volume_projection_during_minimization on: every trial
                              that passed the guard is projected onto the target
                              volume (volume.enforce_constraint: 3 linearised steps,
                              tol 1e-12) BEFORE its energy is taken; a rejected
                              trial restores the positions.  Unqueued trials.      */
  int precondition;        /* conjugate_gradient.py:74-76 (CG only): the direction is
                              built from the row-normalised gradient g_i/(|g_i|+1e-8);
                              the history and the Armijo slope keep the raw gradient.
                              Unfused direction pass, unqueued trials.              */
  int enforce_pins;        /* line_search.py:448-452 with pin_to_plane / pin_to_circle loaded
                              (minimizer.py:1379): every trial that passed the guard runs
                              the pin program (ms_enforce_pins) before the volume projection
                              (if enforce_volume) and its energy.  Needs ms_set_pins;
                              unqueued trials.
                              Next to a tilt family (single field or leaflets, rim sources
                              in the fixed frame and tilt_coupling included) a trial is:
                              x + alpha d and the guard alone (the un-enforced trial is
                              never evaluated), the pin program, the stored tilts projected
                              onto the pinned surface into the field's trial buffer, the
                              energy passes there.  An accepted trial keeps that projection;
                              a rejected trial and an exhausted search leave the tilts bit
                              for bit as they were after the projection at x
                              (line_search.py:475-481, :493-498).
                              Refused: pins next to tilt modules together with the volume
                              constraint (row or enforcer); a rim source in follow mode
                              with any enforcer; sharded contexts.                  */
  int enforce_fixed_plane; /* fixed_plane loaded: every trial that passed the guard runs
                              the plane projection FIRST, in front of the pin program
                              (the device's enforce order: fixed_plane -> pins ->
                              perimeter -> volume -> area).  Needs ms_set_fixed_plane
                              (else MS_ERR_STATE).  Next to a tilt family it takes the
                              lane of the pins next to tilt modules.  Unqueued trials,
                              every Armijo decision on the host, no resident steps.    */
  int enforce_perimeter;   /* perimeter loaded: every trial runs ms_project_perimeter
                              (tol 1e-10, 3 passes) behind the pin program, in front of
                              the volume projection.  Needs ms_set_perimeter (else
                              MS_ERR_STATE).  Refused next to tilt-family modules.      */
  int enforce_area;        /* body_area / global_area loaded (minimizer.py:1379): every
                              trial that passed the guard runs ms_project_area behind the
                              pin program and the volume projection before its energy is
                              taken.  Needs ms_set_area_constraint; unqueued trials, every
                              Armijo decision on the host.  Refused next to tilt-family
                              modules, pins, body_area_penalty; sharded contexts.     */
  int enforce_area_iters;  /* max_iter of that projection: body_area 20, global_area 3
                              (0: 20)                                               */
} ms_stepper_params;

typedef struct ms_step_result {
  int success;        /* line search accepted a step                            */
  int converged;      /* |g| < tol before stepping (minimizer.py:1324)          */
  int trials;         /* energy evaluations spent in the line search            */
  int guard_rejects;  /* trials rejected by the normal-rotation guard           */
  double next_step;   /* step size to use next (line_search.py:398-404,425)     */
  double energy;      /* accepted energy, or energy0 on failure                 */
  double alpha;       /* accepted alpha (0 on failure)                          */
  double energy_eval; /* energy of the gradient evaluation                      */
  double grad_norm;   /* |g|_2                                                  */
  double g_dot_d;
  double volume;      /* body volume at the (possibly new) positions            */
} ms_step_result;

const char *ms_version(void);
int ms_device_count(void);
const char *ms_last_error(const ms_ctx *ctx); /* ctx may be NULL */

/*
 * Build a context: vertices are put in patch order (recursive coordinate bisection down to single tiles), cut into tiles
 * of `tile_vertices` owned vertices (0 = 256; 64, 128, 129..256 or 512 -- 129..255 rows run on the 256-thread
 * instances), and the tile->facet /
 * tile->halo-vertex CSR is pushed to HBM once.  Replaces the per-step reads of
 * Mesh.triangle_row_cache / fixed_mask / boundary_vertex_ids
 * (geometry/mesh.py:597-624, :210-232, :304-319).  `fixed`, `boundary`,
 * `body_facets` (1 = facet belongs to the body, geometry/body.py:60-68) may be
 * NULL (none fixed / closed surface / all facets).  Facets with an index
 * outside [0,nv) are dropped, as fortran_kernels/surface_energy.f90:57-59 does.
 * shard_rank/shard_count: this context evaluates tiles of that shard only
 * (1 process per GPU; per-vertex buffers stay full size, see ms_shard_info).
 */
int ms_create(ms_ctx **out, int device, int nv, int nf, const double *positions,
              const int32_t *tri, const uint8_t *fixed, const uint8_t *boundary,
              const uint8_t *body_facets, int tile_vertices, int shard_rank,
              int shard_count);
void ms_destroy(ms_ctx *ctx);

/* Launch on the caller's HIP stream (hipStream_t as void*); NULL = own stream. */
int ms_set_stream(ms_ctx *ctx, void *hip_stream);

/* Mesh.get_facet_parameter_array("surface_tension") (geometry/mesh.py:234-265) */
int ms_set_surface_tension(ms_ctx *ctx, const double *gamma /* nf */);
/* bending_params._per_vertex_params (modules/energy/bending_params.py:41-115) */
int ms_set_bending_params(ms_ctx *ctx, const double *kappa /* nv */,
                          const double *c0 /* nv */);
int ms_set_params(ms_ctx *ctx, const ms_params *p);
/* body_area_penalty (modules/energy/body_area_penalty.py:113-123): stiffness k = param_resolver.get(body,
 * "area_stiffness") else the global "area_stiffness", target A0 = body.options["area_target"].  Used while
 * MS_MOD_AREA_PENALTY is in ms_params.modules; energies[2] of the evaluation calls is then volume penalty + area
 * penalty.  Single GPU, no tilt-family module next to it (both refused with MS_ERR_STATE). */
int ms_set_area_penalty(ms_ctx *ctx, double stiffness, double target_area);
/* the body's area as the last energy pass folded it (MS_S_AREA; synchronises): the module's own energy is
 * 1/2 k (area - A0)^2 */
int ms_get_body_area(ms_ctx *ctx, double *area);
/* The hard area constraints (modules/constraints/body_area.py, global_area.py).  kind MS_AREA_BODY: the facets of the
 * body (ms_create's body_facets), target = body.options["target_area"]; MS_AREA_GLOBAL: every facet, target = the
 * global target_surface_area; MS_AREA_NONE (or ms_clear_area_constraint) clears it.  The target must be finite and
 * positive (MS_ERR_INVALID).  Single GPU.  With MS_AREA_BODY and MS_CON_BODY_AREA in ms_params.modules the row dA/dx is
 * projected out of the gradient of ms_energy_and_gradient / ms_step on the device: one pass over G for the dot products,
 * lambda from the 1 x 1 (<gA,gA> > 1e-18) or the ridged 2 x 2 system (Cholesky, LU, else the gradient is left alone),
 * G -= lambda_V gV + lambda_A gA, then the fixed rows are zeroed.  global_area has no row. */
#define MS_AREA_NONE 0
#define MS_AREA_BODY 1
#define MS_AREA_GLOBAL 2
int ms_set_area_constraint(ms_ctx *ctx, int kind, double target_area);
int ms_clear_area_constraint(ms_ctx *ctx);
/* enforce_constraint of the module that is set (body_area.py:87-139, global_area.py:8-51) on the context's positions:
 * up to max_iter steps x -= (dA / (|gA|^2 + 1e-18)) gA on the movable rows, |gA|^2 over all rows, until |A - target| <
 * tol (absolute) or |gA|^2 < 1e-18.  *iters: steps taken; *area: the area of the last evaluation (synchronises). */
int ms_project_area(ms_ctx *ctx, double tol, int max_iter, int *iters, double *area);
/* The same with Body's cache (geometry/body.py:347-384): body_area's loop takes area and gradient from
 * compute_area_and_gradient, which answers from the body's cache when the cached version is the mesh's.  The volume
 * module's projection, when it ends on an evaluation (fewer steps than its max_iter), leaves that version current
 * without refreshing the cached area: the first pass of a body_area projection right behind it then works on the area
 * and the gradient of the last FRESH evaluation inside an earlier ms_project_area call.  first_step_cached != 0 asks
 * for that (ignored until a fresh evaluation has happened, and for MS_AREA_GLOBAL, which keeps no cache). */
int ms_project_area_cached(ms_ctx *ctx, double tol, int max_iter, int first_step_cached, int *iters, double *area);
/* the row dA/dx of the constraint that is set at the context's positions (row: nv x 3 in the caller's order, may be
 * NULL), its area and <gA,gA> (synchronises).  body_area.py:28-84 for MS_AREA_BODY. */
int ms_area_row(ms_ctx *ctx, double *row, double *area, double *norm2);
/* stats: launches of {k_area_row, k_area_dots, k_area_fold, k_area_apply} since ms_create.  No reference counterpart. */
int ms_area_stats(ms_ctx *ctx, double stats[4]);
/* The enforce-only shape constraints (modules/constraints/fixed_plane.py, perimeter.py): no KKT row, they only move
 * positions inside ConstraintModuleManager.enforce_all.  Single GPU (MS_ERR_STATE on a sharded context).  Every call
 * below that moves positions invalidates what ms_project_area_cached invalidates.
 *
 * fixed_plane (fixed_plane.py:25-53): every row that is not fixed becomes x - ((x - point) . n) n.  The library divides
 * the normal by its norm; a normal or point that is not finite, or |normal| < 1e-15 (where the module warns and skips),
 * is MS_ERR_INVALID.  normal == NULL clears the plane. */
int ms_set_fixed_plane(ms_ctx *ctx, const double normal[3], const double point[3]);
/* the projection on the context's positions, in place (synchronises); MS_ERR_STATE without a plane */
int ms_enforce_fixed_plane(ms_ctx *ctx);
/* perimeter (perimeter.py:27-74): n_loops edge lists, loop l owning the entries loop_off[l] .. loop_off[l + 1) of tail /
 * head (EXTERNAL rows, the order of ms_set_positions, in list order; duplicates stay, the sign of a reference edge index
 * is already resolved into tail / head), with its target length.  A row out of range or a target that is not finite is
 * MS_ERR_INVALID.  An empty loop is legal and does nothing.  n_loops == 0 clears. */
int ms_set_perimeter(ms_ctx *ctx, int n_loops, const int32_t *loop_off, const int32_t *tail, const int32_t *head,
                     const double *target);
/* Host only, no context: the tables ms_set_perimeter uploads, built by the same code from external rows and a row
 * permutation iperm (external row -> library row): counts = {entries, distinct vertices summed over the loops}; the
 * entries in library rows (e_tail, e_head: loop_off[n_loops]); per loop its distinct vertices in order of first
 * appearance, an entry's tail before its head (vert_off: n_loops + 1, vrow: 2 entries at most); and the vertex -> entry
 * CSR (csr_off: one more than vrow, csr_ent: 2 entries) whose items are -(entry + 1) where the vertex is the entry's tail
 * and +(entry + 1) where it is the head, in list order.  No reference counterpart. */
int ms_perimeter_tables_host(int nv, const int32_t *iperm, int n_loops, const int32_t *loop_off, const int32_t *tail,
                             const int32_t *head, int32_t counts[2], int32_t *e_tail, int32_t *e_head, int32_t *vert_off,
                             int32_t *vrow, int32_t *csr_off, int32_t *csr_ent);
/* perimeter.enforce_constraint on the context's positions, one kernel launch: the loops in list order, per loop up to
 * max_iter passes {P = sum of the listed lengths; stop when |P - target| < tol; g_v = the listed edges' -dir at the tail,
 * +dir at the head (edges shorter than 1e-12 add nothing); stop when sum |g_v|^2 < 1e-18 (all rows); x_v -= ((P - target)
 * / (sum |g_v|^2 + 1e-18)) g_v on the movable rows}.  passes[l]: passes of loop l that moved something; perimeter[l]: P of
 * its last evaluation (n_loops entries each).  Either may be NULL; with both NULL nothing is copied back and the call
 * does not synchronise.  The reference's call is tol 1e-10, max_iter 3 in every context. */
int ms_project_perimeter(ms_ctx *ctx, double tol, int max_iter, int32_t *passes, double *perimeter);
/* The padding rows nv .. nvp of the position buffer, which no kernel may move (*n_rows: how many; rows: n_rows x 3, or
 * NULL to ask for the count alone; synchronises).  For tests.  No reference counterpart. */
int ms_get_padded_rows(ms_ctx *ctx, int64_t *n_rows, double *rows);
/* stats: {k_fixed_plane launches, k_perimeter launches, line-search trials that ran either, loops set}.  No reference
 * counterpart. */
int ms_enforce_only_stats(ms_ctx *ctx, int64_t stats[4]);
/* line_tension (modules/energy/line_tension.py:24-34 selects the edges, :117-123 their gamma: the edge's own
 * "line_tension" option or else the global parameter; an edge whose gamma is 0 is skipped): n_edges tagged edges as
 * EXTERNAL rows (the order of ms_set_positions) in ascending edge order, gamma per edge.  Every row is validated
 * (MS_ERR_INVALID when one is out of range or a gamma is not finite).  tail == NULL clears the tables.  Used while
 * MS_MOD_LINE_TENSION is in ms_params.modules (with no tables the module contributes nothing); energies[0] of the
 * evaluation calls is then surface + line tension.  An edge shorter than 1e-15 contributes nothing (:133-134).  The
 * module takes the penalties' lane of ms_step: one trial per launch, every Armijo decision the host's, no rounds queued
 * ahead, no resident steps; under the one-workgroup interpreter its two kernels are not recorded (they flush it first).
 * Single GPU, no tilt-family module next to it (both refused with MS_ERR_STATE). */
int ms_set_line_tension(ms_ctx *ctx, int n_edges, const int32_t *tail, const int32_t *head, const double *gamma);
/* the module's own energy as the last energy pass summed it (line_tension.py:136; synchronises); 0 without tables */
int ms_get_line_energy(ms_ctx *ctx, double *energy);
/* stats: {k_line_energy launches, k_line_grad launches, and -- from HIP events around the launches made while
 * ms_profile_enable was on -- their summed microseconds, k_line_energy then k_line_grad}; reading resets the event
 * sums (synchronises).  No reference counterpart. */
int ms_line_stats(ms_ctx *ctx, double stats[4]);
/* Host only, no context: the tables ms_set_line_tension uploads, built by the same code from external rows and a row
 * permutation iperm (external row -> library row): counts = {edges kept, touched rows}; the edge table (e_tail,
 * e_head, e_gamma: n_edges entries at most) and the vertex -> edge CSR (vrow: 2 n_edges at most, off: one more,
 * other / csr_gamma: 2 n_edges).  No reference counterpart. */
int ms_line_tables_host(int nv, const int32_t *iperm, int n_edges, const int32_t *tail, const int32_t *head,
                        const double *gamma, int32_t counts[2], int32_t *e_tail, int32_t *e_head, double *e_gamma,
                        int32_t *vrow, int32_t *off, int32_t *other, double *csr_gamma);
/* edge_length_penalty (modules/energy/edge_length_penalty.py:16-22 selects the edges, :40-42 keeps those whose
 * "target_length" is not None, :35 reads k from the global "edge_stiffness" alone, default 100): n_edges charged edges as
 * EXTERNAL rows (the order of ms_set_positions) in ascending edge order, the target length per edge (0 is a target like
 * any other), one stiffness k.  Every row is validated (MS_ERR_INVALID when one is out of range, or a target or k is not
 * finite).  tail == NULL clears the tables; k == 0 leaves tables that hold no edge.  Used while
 * MS_MOD_EDGE_LENGTH_PENALTY is in ms_params.modules (with no tables the module contributes nothing); energies[0] of the
 * evaluation calls is then surface + line tension + edge length penalty.  An edge shorter than 1e-15 contributes nothing
 * (:54-55).  The module takes line_tension's lane of ms_step: one trial per launch, every Armijo decision the host's, no
 * rounds queued ahead, no resident steps; under the one-workgroup interpreter its two kernels are not recorded (they
 * flush it first).  Single GPU, no tilt-family module next to it (both refused with MS_ERR_STATE). */
int ms_set_edge_length_penalty(ms_ctx *ctx, int n_edges, const int32_t *tail, const int32_t *head,
                               const double *target_length, double k);
/* the module's own energy as the last energy pass summed it (edge_length_penalty.py:58; synchronises); 0 without tables */
int ms_get_edge_penalty_energy(ms_ctx *ctx, double *energy);
/* stats: {k_edgepen_energy launches, k_edgepen_grad launches, and -- from HIP events around the launches made while
 * ms_profile_enable was on -- their summed microseconds, k_edgepen_energy then k_edgepen_grad}; reading resets the event
 * sums (synchronises).  No reference counterpart. */
int ms_edge_penalty_stats(ms_ctx *ctx, double stats[4]);
/* Host only, no context: the tables ms_set_edge_length_penalty uploads, built by the code behind ms_line_tables_host
 * with the target length carried as a second column: counts = {edges kept, touched rows}; the edge table (e_tail, e_head,
 * e_l0: n_edges entries at most) and the vertex -> edge CSR (vrow: 2 n_edges at most, off: one more, other / csr_l0:
 * 2 n_edges).  No reference counterpart. */
int ms_edge_penalty_tables_host(int nv, const int32_t *iperm, int n_edges, const int32_t *tail, const int32_t *head,
                                const double *target_length, double k, int32_t counts[2], int32_t *e_tail,
                                int32_t *e_head, double *e_l0, int32_t *vrow, int32_t *off, int32_t *other,
                                double *csr_l0);
/* Per-vertex accumulation in the two big tile kernels (energy pass, gradient pass):
 * 0 (default) LDS atomic adds -- fastest, the floating-point summation order (hence the
 * last bits) may differ between runs; 1 staged CSR gather in a fixed order -- bitwise
 * reproducible run to run, ~20 % slower.  Environment MS_DETERMINISTIC=1 makes 1 the
 * default for new contexts. */
int ms_set_deterministic(ms_ctx *ctx, int on);
/* Mesh.tilts_view() (geometry/mesh.py:391-430) + gp["tilt_rigidity"]; tilts (nv,3) row-major */
int ms_set_tilts(ms_ctx *ctx, const double *tilts /* nv*3 */, double tilt_rigidity);
int ms_get_tilts(ms_ctx *ctx, double *tilts /* nv*3 */);
/* dE/dt = k_t t_v A_v of the last gradient evaluation (tilt.py:160-170) */
int ms_get_tilt_gradient(ms_ctx *ctx, double *tilt_grad /* nv*3 */);
/* ---- tilt field (single vertex-tilt field): relaxation at frozen positions ----
 * ms_set_tilt_fixed: vertex.tilt_fixed flags (runtime/minimizer_helpers.py:49-75),
 *   NULL clears them.
 * ms_tilt_energy_and_gradient: energy of the tilt-reading modules (tilt,
 *   bending_tilt) and the dense tilt gradient dE/dt at the stored tilts
 *   (runtime/evaluation_manager.py:386-462); tilt_grad (nv*3, host) may be NULL
 *   (then read it back with ms_get_tilt_gradient).
 * ms_relax_tilts: TiltRelaxationManager.relax_tilts
 *   (runtime/steppers/tilt_relaxation.py:237-424) on the device: tilts projected
 *   to the tangent planes, then gradient descent or (Jacobi-preconditioned)
 *   Fletcher-Reeves CG with halving back-tracking (<= 12 halvings, accept on
 *   E1 <= E0); tilt-fixed rows keep their projected value. */
typedef struct ms_tilt_relax_params {
  int solver;        /* 0 gradient descent, 1 conjugate gradient ("tilt_solver") */
  int max_iters;     /* tilt_inner_steps / tilt_coupled_steps / tilt_cg_max_iters */
  double step_size;  /* "tilt_step_size" */
  double tol;        /* "tilt_tol" on |dE/dt| over free rows, <= 0: off */
  int jacobi;        /* CG: "tilt_cg_preconditioner" == jacobi */
} ms_tilt_relax_params;
int ms_set_tilt_fixed(ms_ctx *ctx, const uint8_t *tilt_fixed /* nv or NULL */);
/* Rows on which a leaflet is absent (modules/energy/leaflet_presence.py:34-122: the rows whose vertex preset is in
 * leaflet_<l>_absent_presets), one byte per external row; NULL, or no byte set, clears the mask.  A facet with a corner
 * on such a row is no part of the outer field (leaflet_present_triangle_mask, :158-170): tilt_out and
 * tilt_smoothness_out skip it -- energy, shape-gradient and tilt-gradient rows -- and the outer leaflet's vertex areas
 * of a relaxation (tilt_relaxation.py:681-697) and the k_t A_v part of its Jacobi diagonal are summed over the kept
 * facets; the smoothness part of the diagonal and the normals keep every facet, as in the reference.  Every other
 * module reads the field as before.  The rows go through the vertex permutation as ms_set_tilt_fixed's do, and the call
 * invalidates what ms_set_leaflet_tilts invalidates.  While a mask is set the fused tilt lanes (the search / gradient
 * passes of a relaxation, the one-tile fused evaluator, the one-launch energy pass) are not selected: the per-module
 * kernels run, directly or replayed by the interpreter.  leaflet = MS_LEAFLET_IN, and a sharded context, return
 * MS_ERR_UNSUPPORTED.  MS_MOD_BENDING_TILT_OUT does not read the mask: callers refuse it next to one. */
int ms_set_leaflet_absent(ms_ctx *ctx, int leaflet, const uint8_t *absent /* nv or NULL */);
/* gp["tilt_smoothness_rigidity"] of the tilt_smoothness module */
int ms_set_tilt_smoothness(ms_ctx *ctx, double k_smooth);
int ms_tilt_energy_and_gradient(ms_ctx *ctx, double *energy, double *tilt_grad);
int ms_relax_tilts(ms_ctx *ctx, const ms_tilt_relax_params *params,
                   int *iters_out, int *evals_out);

/* ---- two-leaflet tilt fields (tilts_in / tilts_out) ----
 * ms_set_leaflet_tilts: Mesh.tilts_in_view()/tilts_out_view() (nv,3 row-major), the
 *   vertex.tilt_fixed_in / tilt_fixed_out flags (minimizer.py:460-486; NULL = none) and the
 *   leaflet's module parameters.  Modules are switched on by the MS_MOD_*_IN/_OUT bits of
 *   ms_params.modules; both leaflets must be set before the first evaluation.
 * Energies and the shape gradient (coeff_f dA/dx, tilt_leaflet.py:152-166) join the ordinary
 *   evaluation; every line-search trial projects both fields onto the trial surface's tangent
 *   planes like the single field (Mesh.project_tilts_to_tangent, geometry/mesh.py:788-814).
 * ms_leaflet_tilt_energy_and_gradient: EvaluationManager.compute_energy_and_leaflet_tilt_
 *   gradients_array with tilt_vertex_areas given (runtime/evaluation_manager.py:630-742): the
 *   magnitude modules take the lumped vertex-area form 1/2 k sum |t_v|^2 A_v there.
 * ms_relax_leaflet_tilts: TiltRelaxationManager.relax_leaflet_tilts
 *   (runtime/steppers/tilt_relaxation.py:426-1478), default options: GD or Jacobi/plain
 *   Fletcher-Reeves CG over the concatenated (in, out) field, <= 12 halvings, accept on
 *   E1 <= E0, fixed rows keep their projected start value. */
typedef struct ms_leaflet_params {
  double tilt_modulus;        /* "tilt_modulus_in|out" (tilt_params.py:6-12); 0 = no contribution */
  int tilt_mass_consistent;   /* "tilt_mass_mode_in|out" == consistent (tilt_params.py:15-23)  */
  double smoothness;          /* tilt_smoothness_in|out rigidity (tilt_smoothness_utils.py:95-100) */
  double precond_smoothness;  /* rigidity in the Jacobi diagonal (preconditioners.py:111-120)   */
} ms_leaflet_params;
int ms_set_leaflet_tilts(ms_ctx *ctx, int leaflet, const double *tilts /* nv*3 */,
                         const uint8_t *tilt_fixed /* nv or NULL */, const ms_leaflet_params *params);
int ms_get_leaflet_tilts(ms_ctx *ctx, int leaflet, double *tilts /* nv*3 */);
/* Diagnostic, changes nothing: the frozen geometry the last ms_relax_leaflet_tilts left for this leaflet -- its
 * barycentric vertex areas (under ms_set_leaflet_absent: over the kept facets) and the clamped inverse Jacobi diagonal
 * (1 everywhere unless the relaxation ran preconditioned CG).  Either output may be NULL.  MS_ERR_STATE before the
 * leaflet's first relaxation. */
int ms_get_leaflet_relax_geometry(ms_ctx *ctx, int leaflet, double *vertex_areas /* nv */, double *minv /* nv */);
/* tilt_disk_target_in / _out: E = 1/2 k int |t - theta(r) r_hat|^2 dA over the tagged disk rows, theta(r) =
 * theta_B I1(lambda r)/I1(lambda R) (30-term series, tilt_disk_target_in.py:148-157) or theta_B r/R when
 * |lambda| < 1e-12; r, r_hat in the plane through `center` with unit `normal`; R = radius, or the largest
 * in-plane distance of a disk row when radius <= 0 (:216-220).  disk_rows: nv flags (NULL switches it off). */
typedef struct ms_disk_target_params {
  double strength;   /* tilt_disk_target_strength_in|out */
  double theta_b;    /* tilt_disk_target_theta_B[_in|_out] */
  double lambda;     /* tilt_disk_target_lambda[_in|_out], else sqrt(tilt_modulus / bending_modulus) */
  double center[3];
  double normal[3];  /* required (the SVD plane fit of :80-93 is host work) */
  double radius;     /* <= 0: from the disk rows */
} ms_disk_target_params;
int ms_set_leaflet_disk_target(ms_ctx *ctx, int leaflet, const uint8_t *disk_rows /* nv or NULL */,
                               const ms_disk_target_params *params);
/* tilt_rim_source_in / _out: per rim edge mid = 1/2 (p0 + p1), r = (mid - c) - ((mid - c) . n) n, r_hat = r / |r| when
 * |r| > 1e-12 and 0 otherwise, L = |p1 - p0|; E = -sum gamma L 1/2 (t_tail + t_head) . r_hat, tilt gradient
 * -1/2 gamma L r_hat at both ends, no shape gradient.  follow == 0: c is `center`; follow != 0 (a rim row resolves
 * pin_to_circle_mode to fit): c is the mean of the rim rows of x -- taken when an evaluation at x runs and reused by
 * the line-search trials that follow it (tilt_rim_source_in.py:318 reads the mesh, not the trial positions); ms_step
 * with an enforcer on the line search then fails with MS_ERR_STATE.  tail / head are external rows; an edge with
 * gamma == 0 still makes its ends rim rows (they count in the mean).  Every row is validated, gamma / center / normal
 * must be finite and the normal non-zero (it is normalised here).  tail == NULL clears the tables.  Takes effect when
 * MS_MOD_TILT_RIM_SOURCE_IN / _OUT is in ms_params.modules.  Single context only. */
typedef struct ms_rim_source_params {
  double center[3];  /* tilt_rim_source_center (fixed frame) */
  double normal[3];  /* pin_to_circle_normal of the first rim row that carries one, else (0,0,1) */
  int follow;
} ms_rim_source_params;
int ms_set_leaflet_rim_source(ms_ctx *ctx, int leaflet, int n_edges, const int32_t *tail, const int32_t *head,
                              const double *gamma, const ms_rim_source_params *params);
/* the module's own energy at the last evaluation (its sums are also part of energies[3]) */
int ms_get_leaflet_rim_source_energy(ms_ctx *ctx, int leaflet, double *energy);
/* launches so far: {k_rim_frame, k_rim_coef, k_rim_apply} */
int ms_leaflet_rim_source_stats(ms_ctx *ctx, int leaflet, double stats[3]);
/* Host only, no context: the row -> rim edge CSR ms_set_leaflet_rim_source uploads, built by the same code from
 * external rows and a row permutation (iperm: external -> library row).  counts = {edges, rim rows}; vrow holds
 * counts[1] rows (ascending), off counts[1] + 1 offsets, other / csr_gamma 2 * counts[0] entries (room for
 * 2 * n_edges each, and n_edges * 2 + 1 for vrow / off + 1). */
int ms_rim_source_tables_host(int nv, const int32_t *iperm, int n_edges, const int32_t *tail, const int32_t *head,
                              const double *gamma, int32_t counts[2], int32_t *vrow, int32_t *off, int32_t *other,
                              double *csr_gamma);
/* tilt_rim_source_bilayer: ms_set_leaflet_rim_source's tables, checks and frame rules (ms_rim_source_params), kept once per
 * context and applied to both leaflet fields in one pass.  tail == NULL clears the tables.  Takes effect when
 * MS_MOD_TILT_RIM_SOURCE_BILAYER is in ms_params.modules; tilt_rim_source_in / _out next to it keep tables of their own.
 * Single context only. */
int ms_set_rim_source_bilayer(ms_ctx *ctx, int n_edges, const int32_t *tail, const int32_t *head, const double *gamma,
                              const ms_rim_source_params *params);
/* the module's own energy at the last evaluation (its sums are also part of energies[3]) */
int ms_get_rim_source_bilayer_energy(ms_ctx *ctx, double *energy);
/* launches so far: {k_rim_frame, k_rim_coef, k_rim_apply2} */
int ms_rim_source_bilayer_stats(ms_ctx *ctx, double stats[3]);
/* tilt_thetaB_contact_in: the ring rows (tilt_thetaB_contact_in.py:178-197, in vertex_ids order), the frame (:56-67 center,
 * :82-91 normal -- the fitted-plane branch stays host work: a normal is required) and the strengths (:133-142, :150-175).
 * rows are external rows, validated: in range and unique; at most MS_THETAB_MAX_ROWS of them (one workgroup orders the
 * ring in LDS), more is refused.  Every parameter must be finite and the normal non-zero (it is normalised here).
 * rows == NULL clears the tables; a refused call leaves the table in use as it was.  Takes effect when
 * MS_MOD_TILT_THETAB_CONTACT_IN is in ms_params.modules.  Single context only. */
#define MS_THETAB_MAX_ROWS 4096
#define MS_THETAB_WORK_SCALAR 0
#define MS_THETAB_WORK_FIELD_LINEAR 1
typedef struct ms_thetab_contact_params {
  double center[3];  /* tilt_thetaB_center */
  double normal[3];  /* tilt_thetaB_normal */
  double k;          /* tilt_thetaB_strength_in */
  double gamma;      /* tilt_thetaB_contact_strength_in */
  int work_mode;     /* tilt_thetaB_contact_work_mode: MS_THETAB_WORK_* */
  int penalty_mode;  /* tilt_thetaB_contact_penalty_mode: 1 = legacy */
} ms_thetab_contact_params;
int ms_set_thetab_contact(ms_ctx *ctx, int n_rows, const int32_t *rows, const ms_thetab_contact_params *params);
/* theta_B (tilt_thetaB_value, tilt_thetaB_contact_in.py:145-147): it changes between steps, so it is no part of the tables */
int ms_set_thetab_value(ms_ctx *ctx, double theta_b);
/* the module's own energy at the last evaluation (its sums are also part of energies[3]) */
int ms_get_thetab_contact_energy(ms_ctx *ctx, double *energy);
/* {sum w theta / wsum, R_eff, wsum} of the last evaluation (all 0 where the ring contributes nothing) */
int ms_get_thetab_contact_scalars(ms_ctx *ctx, double out[3]);
/* update_scalar_params (tilt_thetaB_contact_in.py:271-302) on the device's state: the ring of the current positions and
 * the stored inner tilts are evaluated (no energy cell is written), and in the legacy penalty mode with k > 0 and a ring
 * that contributes theta_B = sum w theta / wsum + 2 pi R_eff gamma / (k wsum) replaces the stored value.  theta_b gets
 * the value now stored, changed whether it was replaced.  ms_get_thetab_contact_scalars then returns this ring's. */
int ms_update_thetab_value(ms_ctx *ctx, double *theta_b, int *changed);
/* launches so far: {k_thetab_geom, k_thetab_apply} */
int ms_thetab_contact_stats(ms_ctx *ctx, double stats[2]);
/* rim_slope_match_out with a non-zero strength: the rim, outer and optional disk rows
 * (modules/energy/rim_slope_match_out.py:160-169, each in vertex_ids order; :86-102 a disk group equal to the rim group is
 * the caller's to drop), the frame (:110-114 center, :141-149 normal -- the fitted-plane branch :152-153, :422-425 stays
 * host work: a normal is required; geometry/plane_ops.py:8-41 the in-plane axes) and the strength (:105-107).  rows are
 * external rows, validated: in range, unique within a table and the three tables pairwise disjoint; at most
 * MS_RIM_MATCH_MAX_ROWS per ring (one workgroup orders a ring in LDS), more is refused; n_rim and n_outer at least 1
 * (:420-421 an empty ring is a host constant 0.0: no table), n_disk 0 for no disk term.  Every parameter must be finite
 * and the normal non-zero (it is normalised here).  A refused call leaves the tables in use as they were.  Takes effect
 * when MS_MOD_RIM_SLOPE_MATCH_OUT is in ms_params.modules.  Single context only. */
#define MS_RIM_MATCH_MAX_ROWS MS_THETAB_MAX_ROWS
typedef struct ms_rim_match_params {
  double center[3];  /* rim_slope_match_center */
  double normal[3];  /* rim_slope_match_normal */
  double strength;   /* rim_slope_match_strength */
} ms_rim_match_params;
int ms_set_rim_match(ms_ctx *ctx, int n_rim, const int32_t *rim, int n_outer, const int32_t *outer, int n_disk,
                     const int32_t *disk, const ms_rim_match_params *params);
/* drops the tables (the module bit is refused again until the next ms_set_rim_match) */
int ms_clear_rim_match(ms_ctx *ctx);
/* the module's own energy at the last evaluation and its two terms {E, E_out, E_in}: E_out is also part of the outer
 * leaflet's tilt-magnitude sum, E_in of the inner one's (both in energies[3]) */
int ms_get_rim_match_energy(ms_ctx *ctx, double energy[3]);
/* launches so far: {k_rsm_geom, k_rsm_apply}.  The reference evaluates the module once at x and once per trial put to
 * the Armijo test (runtime/minimizer.py line search -> compute_energy_array); every such evaluation orders the rings,
 * while the evaluations of a relaxation (positions frozen) share one geometry launch. */
int ms_rim_match_stats(ms_ctx *ctx, double stats[2]);
/* tilt_thetaB_boundary_in, the constraint t_in . d = theta_B on a ring of vertices
 * (modules/constraints/tilt_thetaB_boundary_in.py:162-236): the ring rows (:89-109, in vertex_ids order) and the frame
 * (:70-74 center, :77-86 normal -- the fitted-plane branch stays host work: a normal is required).  Per row
 * r = (p - c) - ((p - c) . n) n, d = r_hat - (r_hat . N_v) N_v normalised, N_v the unit vertex normal; a row with
 * |r| <= 1e-12 or |d| <= 1e-12 is dropped.  rows are external rows, validated: in range and unique, any number of them.
 * Center and normal must be finite and the normal non-zero (it is normalised here).  rows == NULL clears the table; a
 * refused call leaves the table in use as it was.  theta_B is the value of ms_set_thetab_value.  With a table set,
 * ms_relax_leaflet_tilts enforces the constraint at its start and end and after accepted steps (ms_set_tilt_projection)
 * and projects the inner tilt gradient of every evaluation (runtime/steppers/tilt_relaxation.py:612-616, :803-853,
 * :1048-1052, :1372-1378, :1416-1417, :1474-1478).  Single context only. */
typedef struct ms_thetab_boundary_params {
  double center[3];  /* tilt_thetaB_center */
  double normal[3];  /* tilt_thetaB_normal */
} ms_thetab_boundary_params;
int ms_set_thetab_boundary(ms_ctx *ctx, int n_rows, const int32_t *rows, const ms_thetab_boundary_params *params);
/* tilt_projection_cadence / tilt_projection_interval (tilt_relaxation.py:494-510): a relaxation re-enforces the tilt
 * constraint after every interval-th accepted step (per_step, the default with interval 1) or once behind its loop
 * (per_pass).  Any other cadence and an interval < 1 are refused. */
#define MS_TILT_PROJECTION_PER_STEP 0
#define MS_TILT_PROJECTION_PER_PASS 1
int ms_set_tilt_projection(ms_ctx *ctx, int cadence, int interval);
/* enforce_tilt_constraint (tilt_thetaB_boundary_in.py:339-378) on the context's positions and the stored inner tilts:
 * t <- t + (theta_B - t . d) d on the kept rows that are not tilt_fixed_in; nothing else is touched. */
int ms_thetab_boundary_enforce(ms_ctx *ctx);
/* _boundary_directions (:162-236) on the context's positions, per table row: d[3 n_rows] (0 where the row is dropped)
 * and keep[n_rows] */
int ms_thetab_boundary_directions(ms_ctx *ctx, double *d, uint8_t *keep);
/* what _leaflet_tilt_gradients of the relaxation sees (tilt_relaxation.py:818-853): the evaluation of
 * ms_leaflet_tilt_energy_and_gradient, then the inner gradient's rows g <- g - ((g . d) / (d . d)) d
 * (constraint_manager.py:651-841 with runtime/constraint_projection.py:157-345: the rows are disjoint, so the KKT matrix
 * is diagonal), then the fixed rows zeroed. */
int ms_thetab_boundary_projected_gradient(ms_ctx *ctx, double *energy, double *grad_in, double *grad_out);
/* launches so far: {k_tbb_geom, k_tbb_apply enforcing, k_tbb_apply projecting a gradient} */
int ms_thetab_boundary_stats(ms_ctx *ctx, double stats[3]);
/* Host only, no context: the ring row -> incident facet CSR ms_set_thetab_boundary uploads, built by the same code from
 * external rows, external facets (tri: 3 n_facets rows) and a row permutation (iperm: external -> library row).
 * off gets n_rows + 1 offsets; fv, where given, 3 * off[n_rows] library rows (the facets of a row in ascending facet
 * order, every facet's corners in its own order).  fv == NULL: the offsets only, to size fv. */
int ms_thetab_boundary_tables_host(int nv, const int32_t *iperm, int n_facets, const int32_t *tri, int n_rows,
                                   const int32_t *rows, int32_t *off, int32_t *fv);
/* tilt_coupling: modulus k_c (tilt_coupling_modulus, finite) and sign -1 ("difference"), +1 ("sum") or 0 (off; the
 * module bit is then refused by the passes).  Any other sign is refused.  Takes effect when MS_MOD_TILT_COUPLING is in
 * ms_params.modules.  Single context only. */
int ms_set_tilt_coupling(ms_ctx *ctx, double modulus, int sign);
/* the module's own energy as its LAST LAUNCH summed it, whatever that launch evaluated: an evaluation at x, a line-search
 * trial, or -- after ms_relax_leaflet_tilts -- possibly a rejected trial of the relaxation, not the stored fields.  Run
 * ms_energy first to read it for the stored state (its sums are also part of energies[3]). */
int ms_get_tilt_coupling_energy(ms_ctx *ctx, double *energy);
/* launches so far: {k_couple<0>, k_couple<1>, k_couple_vec} */
int ms_tilt_coupling_stats(ms_ctx *ctx, double stats[3]);
/* tilt_splay_twist_in: the moduli k_splay (tilt_splay_modulus_in, else bending_modulus_in, else bending_modulus) and
 * k_twist (tilt_twist_modulus_in, else tilt_twist_modulus, else 0), finite and non-negative.  Both 0: the bit
 * contributes exactly nothing.  Takes effect when MS_MOD_TILT_SPLAY_TWIST_IN is in ms_params.modules.  Single context
 * only. */
int ms_set_tilt_splay_twist(ms_ctx *ctx, double k_splay, double k_twist);
/* the module's own energy as its LAST LAUNCH summed it, whatever that launch evaluated (ms_get_tilt_coupling_energy's
 * caveat holds): run ms_energy first to read it for the stored state (its sums are also part of energies[3]). */
int ms_get_tilt_splay_twist_energy(ms_ctx *ctx, double *energy);
/* launches so far: {k_splay<0>, k_splay<1>} */
int ms_tilt_splay_twist_stats(ms_ctx *ctx, double stats[2]);
/* per-vertex (kappa, c0) of bending_tilt_in / bending_tilt_out (modules/energy/bt_params.py:225-318:
 * bending_modulus_in|out else bending_modulus; spontaneous_curvature_in|out else the global one) */
int ms_set_leaflet_bending(ms_ctx *ctx, int leaflet, const double *kappa /* nv */, const double *c0 /* nv */);
int ms_leaflet_tilt_energy_and_gradient(ms_ctx *ctx, double *energy, double *grad_in /* nv*3 or NULL */,
                                        double *grad_out /* nv*3 or NULL */);
/* The same evaluation with module_form != 0: the magnitude modules tilt_in / tilt_out in their OWN mass mode, as
 * the plugin API evaluates them when a caller hands it tilt_in_grad_arr / tilt_out_grad_arr -- lumped
 * k A_f/3 t_k, or consistent k A_f/12 (2 t_k + t_a + t_b) per corner
 * (modules/energy/tilt_leaflet.py:101-150).  module_form == 0 is the call above. */
int ms_leaflet_tilt_energy_and_gradient_ex(ms_ctx *ctx, int module_form, double *energy,
                                           double *grad_in /* nv*3 or NULL */, double *grad_out /* nv*3 or NULL */);
int ms_relax_leaflet_tilts(ms_ctx *ctx, const ms_tilt_relax_params *params,
                           int *iters_out, int *evals_out);

/* Mesh.project_tilts_to_tangent (geometry/mesh.py:788-814): t <- t - (t.n) n with the
 * unit vertex normals of the current positions (triangle_ops.py:55-73) */
int ms_project_tilts_to_tangent(ms_ctx *ctx);

/* compute_angle_defects (geometry/curvature.py:335-403): per-vertex angle defect 2 pi - sum of the incident
 * triangle angles (law of cosines, lengths clamped at 1e-15, cosines clipped), 0 on boundary vertices: the
 * integrated Gaussian curvature.  Their sum is 2 pi chi on a closed manifold mesh (Gauss-Bonnet). */
int ms_angle_defects(ms_ctx *ctx, double *defects /* nv */);
/* geometry/curvature.compute_curvature_fields (:404-448) at the context's positions, one tile-kernel pass: each output
 * is (nv,3) in caller row order and may be NULL --
 *   mean_curvature_normal : K_v / (2 max(A_v, 1e-12)), K_v and the mixed-Voronoi areas A_v as compute_curvature_data;
 *   h_area_anglesum       : (H = |mean-curvature normal|, mixed area A_v, sum of the incident triangle angles);
 *   defect_kg             : (angle defect 2 pi - angle sum, 0 on boundary rows; K_G = defect / max(A_v, 1e-12); 0);
 *   principal             : (k1, k2 = H +- sqrt(max(H^2 - K_G, 0)); 0).
 * The raw angle sums also serve the open-surface Gauss-Bonnet invariant of modules/energy/gaussian_curvature.py
 * (runtime/diagnostics/gauss_bonnet.py:260-340). */
int ms_curvature_fields(ms_ctx *ctx, double *mean_curvature_normal, double *h_area_anglesum,
                        double *defect_kg, double *principal);

int ms_set_positions(ms_ctx *ctx, const double *positions /* nv*3 */);
int ms_get_positions(ms_ctx *ctx, double *positions /* nv*3 */);
int ms_get_gradient(ms_ctx *ctx, double *grad /* nv*3 */);
int ms_get_vertex_buffer(ms_ctx *ctx, int buffer, double *out /* nv*ncomp */);

/*
 * Minimizer.compute_energy_and_gradient_array (runtime/minimizer.py:941-992):
 * module loop, volume-constraint projection, fixed rows zeroed.  energies[4] =
 * {surface + line tension + edge length penalty, bending, volume-penalty + area-penalty, tilt}.  grad may be NULL
 * (stays on device).
 */
int ms_energy_and_gradient(ms_ctx *ctx, double energies[4], double *grad);
/*
 * What ONE energy module's compute_energy_and_gradient_array accumulates (the plugin seam,
 * runtime/energy_manager.py:21, evaluation_manager.py:134-151): the module loop's raw sum -- fixed rows are NOT
 * zeroed and no constraint row is projected out (the minimizer does both afterwards, minimizer.py:979-990).
 */
int ms_energy_and_raw_gradient(ms_ctx *ctx, double energies[4], double *grad);
/* EvaluationManager.compute_energy_array_total (evaluation_manager.py:184-225) */
int ms_energy(ms_ctx *ctx, double energies[4]);

/* One stepper.step at the current positions (the body of minimizer.py:1314-1374
 * + line_search.py:267-426), fully device resident. */
int ms_step(ms_ctx *ctx, const ms_stepper_params *sp, double step_size,
            double tol, ms_step_result *out);
/* ConjugateGradient.reset (conjugate_gradient.py:44-50) */
int ms_reset_stepper(ms_ctx *ctx);

/* Minimizer.minimize loop body (runtime/minimizer.py:1230-1535) for n_steps
 * iterations without returning to the host language: [tilt relaxation] ->
 * ms_step -> step-size bookkeeping (fixed mode, zero-step counter, stepper
 * reset on failure, :1425-1476) -> Lagrange volume-drift check with device
 * projection (:1478-1513).  step_log (n_steps x 8, may be NULL) receives per
 * iteration {success, next_step, energy, energy_eval, grad_norm, g_dot_d,
 * alpha, trials}.  Identical to driving ms_step from the caller. */
typedef struct ms_minimize_params {
  ms_stepper_params stepper;
  double step_size;        /* in: first step size                              */
  double tol;              /* convergence |g| < tol                            */
  int fixed_step_mode;     /* gp["step_size_mode"] == "fixed"                  */
  double fixed_step;       /* gp["step_size"]                                  */
  int max_zero_steps;      /* gp["max_zero_steps"], 10                         */
  double step_size_floor;  /* gp["step_size_floor"], 1e-8                      */
  int drift_check;         /* Lagrange mode, no per-trial projection, target set */
  double target_volume;
  double volume_tolerance; /* gp["volume_tolerance"], 1e-3                     */
  int project_on_drift;    /* an enforceable volume constraint module exists   */
  int relax_tilts;         /* tilt_solve_mode nested/coupled                   */
  ms_tilt_relax_params relax;
} ms_minimize_params;

typedef struct ms_minimize_result {
  int iterations;          /* iterations executed                              */
  int converged;           /* stopped on |g| < tol                             */
  int zero_step_exit;      /* stopped after max_zero_steps failed tiny steps   */
  int step_success;        /* success flag of the last line search            */
  int accepted, trials, guard_rejects, moved;  /* totals; moved: x changed     */
  double step_size;        /* out: step size for the next call                 */
  double energy_eval;      /* energy of the last gradient evaluation           */
  double grad_norm;
  int volume_cache_current; /* the loop ended right after a drift check that did NOT project: Body's cached
                             * volume is current, so a finalize projection starts from the cached gradient
                             * (pass it as first_step_cached to ms_project_volume_cached)               */
  int energy_current_valid; /* the step logic already holds the module energies of the positions the loop ended at (the
                             * accepted trial's, or the unchanged x's after a failed step; evaluation reuse level 2): */
  double energy_current;    /* ... their sum -- Minimizer.minimize's final compute_energy() (minimizer.py:1524)
                             * without another energy pass                                                */
} ms_minimize_result;

int ms_minimize(ms_ctx *ctx, const ms_minimize_params *params, int n_steps,
                ms_minimize_result *out, double *step_log);
/* modules/constraints/volume.enforce_constraint projection loop (:117-149) */
int ms_project_volume(ms_ctx *ctx, double target, double tol, int max_iter,
                      int *iters_out, double *volume_out);
/* The same projection as the reference's minimizer reaches it.  Body caches the volume gradient of its last
 * compute_volume_and_gradient evaluation (geometry/body.py:386-407, :463); compute_volume (:70-120) refreshes only
 * the cached volume and mesh version.  An enforce that follows a compute_volume at the same mesh version -- the
 * Lagrange drift check, runtime/minimizer.py:1492 -- therefore takes its FIRST step with the current volume but the
 * gradient the previous enforce evaluated last.  first_step_cached != 0 reproduces that (no effect while nothing is
 * cached); every fresh evaluation refreshes the cache, also through ms_project_volume. */
int ms_project_volume_cached(ms_ctx *ctx, double target, double tol, int max_iter,
                             int first_step_cached, int *iters_out, double *volume_out);

/* ---- phase-level entry points (multi-GPU drivers interleave collectives) -- */
/* energy pass over this shard's tiles at x (+ alpha*d if use_direction);
 * writes trial positions to XT when write_trial; guard != 0 also evaluates the
 * normal-rotation guard.  Asynchronous; partial sums are reduced into SCAL. */
int ms_phase_energy(ms_ctx *ctx, int use_direction, double alpha, int write_trial,
                    int guard, int write_bending_factors);
int ms_phase_gradient(ms_ctx *ctx);   /* gradient pass (needs bending factors) */
int ms_phase_direction(ms_ctx *ctx, int stepper, int use_history);
int ms_phase_accept(ms_ctx *ctx, int keep_history); /* x <- xt, CG history     */
int ms_fetch_scalars(ms_ctx *ctx, double *out /* MS_NSCAL */); /* synchronises */
int ms_store_scalars(ms_ctx *ctx, const double *in /* MS_NSCAL */);

/* Sharded accept: every rank forms xt = x + alpha*d on ALL rows (x and d are
 * replicated after the direction all-gather, so no exchange is needed), then
 * x <-> xt and, if keep_history, the CG history swap of ms_phase_accept. */
int ms_phase_commit_trial(ms_ctx *ctx, double alpha, int keep_history);

/* Fused K_C + direction pass (no constraint row, no tilt module): the sharded
 * counterpart of what ms_step queues (runtime/minimizer.py:941-992 followed by
 * conjugate_gradient.py:60-100 / gradient_descent.py:35-84); reduces the
 * direction scalars of this rank's rows. */
int ms_phase_gradient_direction(ms_ctx *ctx, int stepper, int use_history);
/* After a boundary exchange of fK/fA written by an accepted trial pass: the
 * factor buffers describe the committed x. */
int ms_phase_set_factors_valid(ms_ctx *ctx, int valid);

/* ---- shard boundary exchange (multi-GPU; the reference is single-process) ----
 * A rank's boundary rows are the rows it owns that other ranks' tiles read as
 * halo.  One exchange = ms_pack_boundary -> all-gather of the fixed-size
 * messages (RCCL, done by the caller on the context's stream) ->
 * ms_unpack_boundary.  Message = [MS_NSCAL reduction scalars | boundary rows of
 * the listed per-vertex buffers]; unpack scatters every peer's rows into the
 * local buffers and returns all ranks' scalar headers (shard_count x MS_NSCAL)
 * for the rank-ordered host fold.
 * info = {max boundary rows over ranks, this rank's, this rank's halo rows, shard_count}. */
int ms_boundary_info(ms_ctx *ctx, int64_t info[4]);
size_t ms_exchange_bytes(ms_ctx *ctx, int n_buffers, const int *buffer_ids);
int ms_pack_boundary(ms_ctx *ctx, int n_buffers, const int *buffer_ids,
                     void *send_dev, size_t send_bytes);
int ms_unpack_boundary(ms_ctx *ctx, int n_buffers, const int *buffer_ids,
                       const void *recv_dev, size_t stride_bytes,
                       double *scal_all_host);

/* ---- library-side multi-GPU driver -------------------------------------------
 * The sharded step (the control flow of membrane_solver_amd/parallel.py's
 * ShardedStepper, i.e. ms_step with the exchanges of DESIGN.md section 6) run inside
 * the library: per exchange pack -> all-gather -> unpack -> mailbox poll, with no
 * interpreter in the loop.  The all-gather is RCCL's ncclAllGather on the
 * context's stream (ms_shard_comm_init; librccl is resolved from the process,
 * i.e. the copy torch.distributed already loaded) or a caller-supplied function
 * (tests use an in-process stand-in).  ms_shard_unique_id fills the 128-byte
 * ncclUniqueId on one rank; the caller broadcasts it to the others. */
typedef int (*ms_allgather_fn)(void *user, const void *send_dev, void *recv_dev,
                               size_t bytes_per_rank);
int ms_shard_unique_id(void *id128);
int ms_shard_comm_init(ms_ctx *ctx, const void *id128);
int ms_shard_set_allgather(ms_ctx *ctx, ms_allgather_fn fn, void *user);
/* Peer-to-peer exchange (no collective library in the step): every rank's pack kernel stores its scalar header and
 * boundary rows straight into EVERY peer's receive slab (xGMI stores through IPC-mapped device memory), a one-wave
 * kernel then raises this rank's flag word on every peer, and every block row of the unpack kernel waits -- bounded:
 * a peer that never arrives becomes an error after ~2 s, not a wave that never finishes -- for the flag word of the
 * rank whose message it unpacks.  Two slabs alternate (a peer can be at most one exchange ahead).
 *   ms_shard_peer_export: fills handles[0..127] with the hipIpcMemHandle_t of this rank's receive slab and of its flag
 *                          words (64 bytes each); the caller all-gathers the 128-byte records in rank order;
 *   ms_shard_peer_open:   opens every peer's two handles (world x 128 bytes, rank order; the own record is skipped);
 *   ms_shard_peer_set_pointers: the same for shard contexts of ONE process (thread shards): raw device pointers of
 *                          every rank's slab / flag words in rank order (ms_shard_peer_local gives a rank's own).
 * With peers set, ms_shard_step uses this exchange instead of ncclAllGather / the all-gather callback. */
int ms_shard_peer_export(ms_ctx *ctx, void *handles128);
int ms_shard_peer_open(ms_ctx *ctx, const void *handles_all);
int ms_shard_peer_local(ms_ctx *ctx, void **recv_slab, void **flag_words);
int ms_shard_peer_set_pointers(ms_ctx *ctx, void *const *recv_slabs, void *const *flag_words);
/* Shard contexts of ONE process share the device's few hardware queues: a rank's waiting wave can sit in front of the
 * very kernels of another rank it waits for.  Such contexts (tests) wait on the host instead: after raising its flags a
 * rank synchronises its stream and calls fn(user), which returns once every rank has done the same. */
typedef int (*ms_barrier_fn)(void *user);
int ms_shard_peer_set_barrier(ms_ctx *ctx, ms_barrier_fn fn, void *user);
int ms_shard_step(ms_ctx *ctx, const ms_stepper_params *params, double step_size,
                  double tol, ms_step_result *out);
/* number of exchanges done so far by ms_shard_step on this context */
int64_t ms_shard_exchange_count(const ms_ctx *ctx);
/* Peer-to-peer transport with in-kernel flag words: ms_shard_step also takes a trial's Armijo decision on the device
 * (from the scalar headers every rank has in its slab, added in rank order: the host's arithmetic), and queues what an
 * acceptance is followed by -- the commit x <- x + alpha d, the gradient + direction pass of the new point and that
 * pass's exchange -- behind it, gated on the decision word; the host replays the decision from the same headers
 * (a difference is an error) and the next ms_shard_step takes the pass's results instead of queueing it
 * (runtime/minimizer.py:1189-1535, line_search.py:386-392: no reference counterpart, same trajectory).
 * MS_SHARD_CHAIN=0 switches all of it off.  stats: {chains queued, chains that ran (main trial accepted), adopted by
 * the next step, dropped (the next step wanted another pass), 0, 0, 0, 0}: entries 4-7 are reserved and written as 0. */
int ms_shard_chain_stats(const ms_ctx *ctx, int64_t stats[8]);
/* ranks of the context's RCCL communicator as ncclCommCount reports them (0: no communicator) */
int ms_shard_comm_ranks(ms_ctx *ctx);
/* Kind of device memory the peer exchange's receive slabs and flag words live in: 0 uncached (MTYPE_UC, what the
 * collective library's own IPC signal buffers use), 1 fine-grained, 2 plain hipMalloc (coarse-grained: coherent across
 * GPUs at kernel boundaries only -- the fallback when the other kinds cannot be allocated or exported); -1 before
 * the slabs exist.  No reference counterpart (the reference is single-process). */
int ms_shard_peer_memory_kind(const ms_ctx *ctx);

/* Per-vertex state in caller-owned device memory (e.g. a torch tensor, so RCCL
 * collectives can run on it in place).  ms_state_bytes gives the size;
 * ms_rebind_state copies the current state there and uses it from then on.
 * The caller keeps the memory alive until ms_destroy. */
size_t ms_state_bytes(const ms_ctx *ctx);
int ms_rebind_state(ms_ctx *ctx, void *device_base, size_t bytes);

/* device pointer + geometry of a per-vertex buffer, for RCCL collectives on it */
int ms_device_buffer(ms_ctx *ctx, int buffer, void **dev_ptr, size_t *bytes);
/* rows = padded vertex rows (nvp); this shard owns rows [row0,row1) */
int ms_shard_info(ms_ctx *ctx, int64_t *nvp, int64_t *row0, int64_t *row1,
                  int64_t *rows_per_shard);
/* tiling statistics: n_tiles, facet instances (with halo duplicates), max halo */
int ms_tile_stats(ms_ctx *ctx, int64_t *n_tiles, int64_t *facet_instances,
                  int64_t *max_halo, int64_t *lds_bytes_energy,
                  int64_t *lds_bytes_gradient);

/* Per-kernel device timing with HIP events on the context's stream.  While
 * enabled every energy / gradient / direction / reduce launch is bracketed by
 * an event pair; ms_profile_read synchronises, returns the summed milliseconds
 * and launch counts per kind {0 energy, 1 gradient, 2 direction, 3 reduce,
 * 4 tilt, 5 bending_tilt facet pass, 6 tilt vector ops, 7 energy pair launch (two
 * trial evaluations of one line search in one launch), 8 energy triple launch
 * (three), 9 gradient, lean instantiation (k_gradient<1,false,256,0,true,true>: analytic
 * bending, uniform surface tension, no separate previous-direction rows)} and resets the
 * counters.  Used by bench.py for the roofline figure. */
#define MS_PROF_KINDS 13 /* 10: energy launch with four to eight trial evaluations (k_energy<...,8>);
                          * 11: tilt smoothness pass (k_tsmooth); 12: tilt search pass (k_tsearch: several step
                          * sizes of a relaxation's backtracking ladder, every tilt module, one launch) */
int ms_profile_enable(ms_ctx *ctx, int on);
int ms_profile_read(ms_ctx *ctx, double total_ms[MS_PROF_KINDS],
                    int64_t launches[MS_PROF_KINDS]);

/* Line-search queue statistics since ms_create (ms_step): stats[0] rounds queued, [1] multi-trial energy
 * launches among them, [2] trial evaluations of those launches that lay behind the accepted trial (wasted),
 * [3] searches whose accepted trial was an energy-only early trial of a multi-trial launch (re-evaluated alone),
 * [4] decisions on which host and device differed (each one also fails the call with MS_ERR_STATE: the device takes
 * every Armijo decision once, in the fold that closes the stage -- runtime/steppers/line_search.py:386-392 -- and the
 * host replays it from the same doubles), [5] rounds queued for a step that had not started yet (behind the running
 * gradient pass; ms_minimize only), [6] those the step adopted, [7] those dropped. */
int ms_queue_stats(ms_ctx *ctx, int64_t stats[8]);
/* Read-only trial log of the most recent ms_step call (a step of ms_minimize's kernel-per-phase path included): one
 * row per alpha of the backtracking ladder, in the order the loop of runtime/steppers/line_search.py:357-421 sees
 * them.  Row (MS_TRIAL_COLS doubles): {alpha, trial energy as the host replayed the decision from it, Armijo
 * right-hand side energy0 + c * alpha * <g,d>, trials of the energy launch that evaluated it (1: a gated stage or a
 * trial the host decided alone), slot of the trial inside that launch, flags}.  MS_TRIAL_BEHIND: the trial lay behind
 * the accepted slot of its launch -- evaluated, not part of the search (ms_queue_stats counts these as wasted);
 * MS_TRIAL_GUARD: the normal-rotation guard rejected the alpha and no energy was taken (the energy column is 0).
 * The log holds at most that call's max_iter rows; *n_rows is the number logged, of which min(*n_rows, max_rows) are
 * copied (rows may be NULL when max_rows is 0).  first_launch_hist (may be NULL): since ms_create, the number of
 * queued rounds whose first launch evaluated 1, 2, ... 8 trials.  Keeping the log changes no launch and no result.
 * No reference counterpart. */
#define MS_TRIAL_COLS 6
#define MS_TRIAL_BEHIND 1
#define MS_TRIAL_GUARD 2
int ms_search_trials(ms_ctx *ctx, double *rows, int max_rows, int *n_rows, int64_t first_launch_hist[8]);
/* The fused gradient + direction pass of ms_step (CG history, no constraint row, single context) does not store the
 * direction when the last direction with history was no descent direction: the step is expected to fail without a
 * trial (conjugate_gradient.py:78-96 then line_search.py:325-328) and the stepper to restart along -g, so nobody
 * reads it.  Only the store is left out: the scalars, the step log and every result stay bit for bit what they were.
 * When the direction is wanted after all -- <g,d> < 0, ms_get_vertex_buffer(MS_BUF_D), the phase API -- the direction
 * kernel writes it from the stored gradient and history first.  *skipped: steps whose gradient pass left the store out;
 * *materialized: directions written out afterwards.  Since ms_create.  (MS_BUF_D after ms_reset_stepper is unspecified until the next step.) */
int ms_direction_stats(ms_ctx *ctx, int64_t *skipped, int64_t *materialized);
/* The energy kernel has a lean instance for the headline case: surface + Helfrich bending with uniform surface tension,
 * bending modulus and spontaneous curvature on a closed surface of more than one tile, LDS-atomic vertex sums (not
 * ms_set_deterministic), no volume term and no bending_tilt records.  Every other case runs the general instance.
 * The lean instance performs the general instance's arithmetic operation for operation; what the general one decides
 * from its arguments at run time is compiled out.  MS_KA_LEAN=0 in the environment at ms_create forces the general
 * instance.
 * *lean / *general: energy launches (or k_exec records) of either kind since ms_create.  No reference counterpart. */
int ms_energy_stats(ms_ctx *ctx, int64_t *lean, int64_t *general);
/* One-tile meshes (every mesh the reference's own benchmarks and decks use: <= 256 vertices): the library records its
 * kernel launches and runs them pack by pack in ONE workgroup (k_exec) instead of launching each -- same device code,
 * same results bit for bit, a few launches per step instead of dozens.  MS_EXEC=0 in the environment switches it off.
 * Tilt relaxations (ms_relax_tilts / ms_relax_leaflet_tilts) then run as ONE launch: the command lists of the loop are
 * captured once and the reference's control flow (tilt_relaxation.py:303-421, 885-1230) runs in that workgroup
 * (MS_EXEC_RELAX=0: host-driven loop over packs).
 * stats: {active now, packs launched, launches recorded, bit 0 wanted (inactive while profiling) | relaxation
 * programs run << 8}.  No reference counterpart. */
int ms_exec_stats(ms_ctx *ctx, int64_t stats[4]);
/* Meshes whose tiles all fit on the chip at once (a few hundred tiles): ms_minimize runs the steps of the surface
 * (+ volume constraint row) / gradient-descent lane in ONE launch per call -- one workgroup per tile keeps its tile in
 * LDS across steps, grid barriers between the phases of a step, every workgroup folds the partials itself
 * (runtime/minimizer.py:1189-1535, runtime/steppers/line_search.py:267-426 for that lane).  A step the kernel cannot
 * take (guard range, exhausted search, drift projection, convergence) goes through the ordinary path.
 * MS_RESIDENT=0 switches it off.  stats: {co-residency (-1 not asked, 0 no, 1 yes), launches, steps taken, steps
 * declined}.  No reference counterpart. */
int ms_resident_stats(ms_ctx *ctx, int64_t stats[4]);

/* ---- pin_to_plane / pin_to_circle (modules/constraints/pin_to_plane.py, pin_to_circle.py) -------------------------
 * Tables built on the host by membrane_solver_amd.modules.constraints.pins.device_tables; rows are EXTERNAL rows
 * (the order of ms_set_positions).  params: n_params x 7 doubles (normal, point / centre / slide base, radius; a
 * slide circle's radius < 0 is the members' mean radial distance).  The enforcement program is n_stages stages in
 * order: MS_PIN_STAGE_FIXED (per-row plane / circle projections, item_arg = op << 24 | param row, a row at most once
 * per stage), MS_PIN_STAGE_PLANE_GROUP (slide plane through the members' centroid; item_arg 1 = a fixed member that
 * keeps its place), MS_PIN_STAGE_CIRCLE_GROUP (slide circle).  lane: MS_PIN_LANE_PROJECT removes the rows of
 * constraint_gradients_rows_array from every gradient (and the volume row) before the KKT multiplier is taken:
 * n_grad per-row directions (MS_PIN_GRAD_*) and n_avg slide-circle supports whose normal components are replaced by
 * their mean; MS_PIN_LANE_SKIP leaves the gradient untouched, volume row included -- the reference's KKT solve
 * (runtime/constraint_projection.py:101-129, _solve_kkt_system) fails on C C^T for such row sets and returns.
 * params == NULL clears the tables. */
#define MS_PIN_STAGE_FIXED 0
#define MS_PIN_STAGE_PLANE_GROUP 1
#define MS_PIN_STAGE_CIRCLE_GROUP 2
#define MS_PIN_OP_PLANE 0
#define MS_PIN_OP_CIRCLE 1
#define MS_PIN_GRAD_PLANE 0
#define MS_PIN_GRAD_CIRCLE 1
#define MS_PIN_GRAD_RADIAL 2
#define MS_PIN_LANE_SKIP 0
#define MS_PIN_LANE_PROJECT 1
int ms_set_pins(ms_ctx *ctx, int n_params, const double *params, int n_stages, const int32_t *stage_kind,
                const int32_t *stage_param, const int32_t *stage_off, const int32_t *item_row,
                const int32_t *item_arg, int lane, int n_grad, const int32_t *grad_row, const int32_t *grad_kind,
                const int32_t *grad_param, int n_avg, const int32_t *avg_param, const int32_t *avg_off,
                const int32_t *avg_row);
/* pin_to_plane.enforce_constraint then pin_to_circle.enforce_constraint (in the order the tables hold them) on
 * buffer X, in place: one k_pin_enforce launch. */
int ms_enforce_pins(ms_ctx *ctx);
/* stats: {lane (-1 no tables, 0 skip, 1 project), runs of the enforcement program, runs of the gradient pass, trials
 * projected}.  A run is a k_pin_enforce / k_pin_grad launch or, on a one-tile context, a record of the one-workgroup
 * interpreter's pack (MS_EXEC_PINS=0: always a launch). */
int ms_pin_stats(ms_ctx *ctx, int64_t stats[4]);
/* Tilt relaxations of multi-tile meshes: the backtracking search (runtime/steppers/tilt_relaxation.py:326-347,
 * 380-398, 918-973, 1150-1230: up to twelve halvings of the step on E(P(t + step*src)), positions frozen) runs as
 * search passes -- one launch evaluates several step sizes of the ladder for every tilt-reading module of both
 * leaflets (k_tsearch) -- with the iteration and evaluation counts of the sequential loop.  Module sets the pass
 * does not cover (disk targets, a lone tilt module on the single field, consistent mass there) and MS_TSEARCH=0 keep
 * one launch per module, field and trial.  stats: {search passes launched, step sizes evaluated by them}. */
int ms_tsearch_stats(ms_ctx *ctx, int64_t stats[2]);
/* Diagnostic, changes nothing: which lane the tilt family takes on this context.  The size of a tile's vertex patch,
 * cap = owned rows + largest halo, decides it: the fused tilt passes step aside above 150 KiB of LDS (the
 * launch-per-module kernels run instead, same results), a workgroup may ask for 160 KiB at the most.
 * stats[0..11] = {cap, max_ent (largest vertex -> corner list of a tile),
 *   one field:  8-step-size search pass fits, gradient pass fits, energy-only pass fits (each 0 / 1),
 *   two fields: the same three,
 *   LDS bytes of the leaflet bending_tilt instance of the shape-gradient kernel in the context's current summation
 *   mode and module mask, whether that instance fits (0: an evaluation that needs it -- a shape gradient with
 *   bending_tilt_in/out in the mask -- returns MS_ERR_TILE_CAPACITY before it launches anything; everything else on the
 *   context works), threads per workgroup, rows a tile owns}.
 * The values come from the functions and limits the library's own planners read. */
int ms_tilt_lane_stats(ms_ctx *ctx, int64_t stats[12]);
/* Host-only (no GPU needed): the same for a mesh as ms_create would tile it (fixed_order != 0: the fixed-order
 * summation mode of ms_set_deterministic; no constraint row) ... */
int ms_plan_tilt_lanes(int nv, int nf, const double *positions, const int32_t *tri, int tile_vertices,
                       int fixed_order, int64_t stats[12]);
/* ... and for a patch of `cap` rows outright (threads = rows a tile owns = tile size): where the thresholds lie. */
int ms_tilt_lane_plan(int threads, int cap, int max_ent, int fixed_order, int64_t stats[12]);
/* Diagnostic of the same interpreter: on != 0 arms a device buffer to which every record run appends its duration
 * (s_memrealtime); a call also returns what has accumulated since the last one, per (kind, mode) pair: rows of
 * {kind, mode | instance << 16, count, total microseconds} (max_rows rows of 4 doubles; NULL: just arm / disarm). */
int ms_exec_trace(ms_ctx *ctx, int on, double *rows, int max_rows, int *n_rows);

/* Host-only planning pass (no GPU needed): runs the same tiling ms_create
 * uses and reports stats[0..7] = {n_tiles, facet_instances, max_halo,
 * max_tile_facets, dropped_facets, owner_instances, owned_corner_slots,
 * lds_bytes_gradient}.  perm_out (nv, patch row -> caller row) may be NULL.
 * Invariants: owner_instances == nf - dropped, owned_corner_slots == 3*that. */
int ms_plan_tiling(int nv, int nf, const double *positions, const int32_t *tri,
                   int tile_vertices, int shard_count, int64_t stats[8],
                   int32_t *perm_out);
/* Host-only: LDS bank model of the lane order inside the tiles (no GPU needed).
 * model[0] = mean LDS cycles of one corner gather (8-byte reads: lane groups of 32
 * over 64 four-byte banks, identical addresses broadcast; 1.0 = conflict-free),
 * model[1] = the same for one per-corner accumulator update (ds_add_f64 on owned
 * corners: lane groups of 16 over 32 banks, identical addresses serialise),
 * model[2], model[3] = fraction of lane groups that are conflict-free for each. */
int ms_plan_tiling_conflicts(int nv, int nf, const double *positions,
                             const int32_t *tri, int tile_vertices, double model[4]);
/* Host-only: the lane order of the lean k_energy instances (no GPU needed).  They
 * read each tile's facet records in an order of their own (the records themselves
 * are the common ones), chosen by a greedy for the LDS instructions they issue per
 * aligned lane group and corner slot k:
 *   A16  ds_add_f64: groups of 16 lanes, OWNED targets only (a halo corner issues
 *        none), ways = most targets in one residue mod 16 (same slot twice = 2)
 *   R16  ds_read2_b64 halves: groups of 16, distinct slots by residue mod 16
 *   R32  ds_read_b64: groups of 32, distinct slots by residue mod 32
 * model[0..7] scores the common order, model[8..15] the lean one:
 *   {mean A16 ways per group with an owned target, mean R16, mean R32,
 *    sum over groups of 7.4 A16 + 2 R16 + R32 (the energy kernel's mix),
 *    sum of 5.55 A16 + 4 R16 + 3 R32 (the lean gradient kernel's mix, which reads
 *    the common order: reported for comparison),
 *    A16 groups, R16 groups, R32 groups}.
 * facet_off_out (n_tiles + 1), common_out and lean_out (facet_instances x 4:
 * l0, l1, l2, flags) may each be NULL; sizes as ms_plan_tiling reports them. */
int ms_plan_lane_order(int nv, int nf, const double *positions, const int32_t *tri,
                       int tile_vertices, double model[16], int32_t *facet_off_out,
                       int32_t *common_out, int32_t *lean_out);
/* stats[0]: 1 if the lean k_energy instances of this context read their own lane order
 * (0: MS_LANE_ORDER=0 at ms_create, or a tile of more than 1024 slots);
 * stats[1]: 1 if they stage from a halo list of their own (not built: always 0). */
int ms_lane_order_stats(ms_ctx *ctx, int64_t stats[2]);

/* ---- kernel-provider seam: the five procedures under fortran_kernels/ ----
 * Host arrays in, host arrays out (H2D/D2H per call: for parity, not speed).
 * Semantics follow the Fortran: see fortran_kernels/loader.py:15-20 KernelSpec.
 */
/* surface_energy.f90:27-99 -- grad (nv*3) is ACCUMULATED into */
int ms_surface_energy_and_gradient_host(int nv, int nf, const double *pos,
                                        const int32_t *tri, const double *gamma,
                                        double *grad, double *energy);
/* bending_kernels.f90:32-74 */
int ms_grad_cotan_batch_host(int n, const double *u, const double *v,
                             double *grad_u, double *grad_v);
/* bending_kernels.f90:87-131 -- out is overwritten (zeroed first) */
int ms_apply_beltrami_laplacian_host(int dim, int nv, int nf,
                                     const double *weights, const int32_t *tri,
                                     const double *field, double *out);
/* tilt_kernels.f90:26-86 */
int ms_p1_triangle_divergence_host(int nv, int nf, const double *pos,
                                   const double *tilts, const int32_t *tri,
                                   double *div_tri, double *area, double *g0,
                                   double *g1, double *g2);
/* tilt_kernels.f90:88-190 -- va0..va2 may be NULL */
int ms_compute_curvature_data_host(int nv, int nf, const double *pos,
                                   const int32_t *tri, double *k_vecs,
                                   double *vertex_areas, double *weights,
                                   double *va0, double *va1, double *va2);

#ifdef __cplusplus
}
#endif
#endif /* MEMBRANE_HIP_H */
