// Internal declarations shared by the host API, the tile builder and the
// gfx950 kernels of libmembrane_hip.so.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "membrane_hip.h"

namespace ms {

// Switches of finished experiments (MS_NO_FAST, MS_TILE_ORDER, MS_FACET_ORDER, MS_KA_LDS_MIN) exist only in variant
// builds (tools/build_variant.sh passes -DMS_VARIANT_ENV): the shipped library does not read them.
inline const char* variant_env(const char* name) {
#ifdef MS_VARIANT_ENV
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// One tile-facet instance: local vertex slots inside the tile's LDS patch
// ([0,n_owned) owned, then halo) + flags.
struct TileFacet {
  uint16_t l0, l1, l2;
  uint16_t flags;  // bit0: this tile owns the facet's scalar terms (energy, volume,
                   //       min-edge, guard) ; bit1: facet belongs to the body
};
static_assert(sizeof(TileFacet) == 8, "TileFacet must be 8 bytes");

constexpr uint16_t TF_OWNER = 1;
constexpr uint16_t TF_BODY = 2;

// ---- device-side line-search decisions (ms_step's queue) -----------------------------------------------------------
// A fold (k_reduce) that closes a line-search stage takes the Armijo decision itself -- ONE workgroup, from the energies
// it has just folded and the right-hand sides the host supplied -- and publishes it as one word with an agent-scope
// (write-through) store.  Every kernel queued behind the stage reads that word with an agent-scope load and runs iff it
// holds the code the host queued it for; no workgroup re-derives a decision from doubles, so the workgroups of one
// launch cannot disagree.  The host replays the decision from the same doubles (mailbox) and compares codes.
constexpr int MS_MAX_TRIALS = 8;        // trials one energy launch can evaluate (alphas of one Armijo ladder)
constexpr int MS_P_RAN = MS_NSCAL;      // partial row: 1.0 from every workgroup of a GATED launch that ran, 0.0 from one that did not
constexpr int MS_NPART = MS_NSCAL + 1;  // rows of a partials array
constexpr int MS_MB_DEC = MS_NSCAL;     // mailbox entry of the fold's decision code
constexpr int MS_MB_WORDS = MS_NSCAL + 1;  // {value, sequence} entries of a mailbox
constexpr int MS_DEC_STRIDE = 64;       // uint32 words between two decision records (256 bytes: a GO record carries 8 right-hand sides and 8 handed-over parameters)
enum : uint32_t {
  DEC_NONE = 0,         // never written
  DEC_CONTINUE = 1,     // every trial so far was rejected: the next stage of the ladder runs
  DEC_ACCEPT_MAIN = 2,  // accepted, and the accepted trial's outputs are the ordinary ones (xt, fK, fA): the gradient pass runs
  DEC_ACCEPT_SIDE = 3,  // an EARLY trial of a multi-trial launch was accepted (energy-only evaluation): nothing queued runs
  DEC_GO = 4,           // (host side only: the merged fold's test passed)
  DEC_STOP = 5,         // merged fold: the search it was queued for does not happen (converged, the other kind of
                        // direction, guard range): nothing behind it runs
  DEC_ERR_RAN = 0x100   // flag: a gated launch ran on some of its workgroups only
};

constexpr uint8_t VF_FIXED = 1;
constexpr uint8_t VF_BOUNDARY = 2;
constexpr uint8_t VF_TILT_FIXED = 4;  // vertex.tilt_fixed (runtime/minimizer_helpers.py:49-75)
constexpr uint8_t VF_TILT_FIXED_IN = 8;    // vertex.tilt_fixed_in  (minimizer.py:460-472)
constexpr uint8_t VF_TILT_FIXED_OUT = 16;  // vertex.tilt_fixed_out (minimizer.py:474-486)
constexpr uint8_t VF_ABSENT_OUT = 32;      // the outer leaflet is absent on this row (leaflet_presence.py:34-122)

// LDS bank model of one lane order (lane_order_model): per aligned lane group and corner slot k, the number of "ways"
// (serialised passes) of the instruction the group issues.
//   a16: ds_add_f64, groups of 16, OWNED targets only, by slot mod 16; the same slot twice is two ways
//   r16: ds_read2_b64 halves, groups of 16, distinct slots by slot mod 16 (24-byte rows: bank 6 l mod 32); same slot broadcasts
//   r32: ds_read_b64, groups of 32, distinct slots by slot mod 32
// *_sum: ways summed over the groups; *_groups: groups counted (a16: groups with an owned target only).
// ka, kc: the two headline kernels' instruction mixes per corner, summed over groups (cycles of the model)
struct LaneModel {
  double a16_sum = 0, r16_sum = 0, r32_sum = 0;
  double a16_groups = 0, r16_groups = 0, r32_groups = 0;
  double ka() const { return LANE_W_KA[0] * a16_sum + LANE_W_KA[1] * r16_sum + LANE_W_KA[2] * r32_sum; }
  double kc() const { return LANE_W_KC[0] * a16_sum + LANE_W_KC[1] * r16_sum + LANE_W_KC[2] * r32_sum; }
  // per group-way: an atomic 1.85 (7.4 cycles per extra way of a wave = four groups), a ds_read2_b64 2, a ds_read_b64 1.
  // K_A per corner: 4 atomics, 1 read2, 1 read; K_C: 3 atomics, 2 read2 (px, fk), 3 reads (px, fk, fa)
  static constexpr double LANE_W_KA[3] = {7.4, 2.0, 1.0};
  static constexpr double LANE_W_KC[3] = {5.55, 4.0, 3.0};
};

// Host-side result of the tiling pass.
struct Tiling {
  int nv = 0, nf = 0, T = 256;
  int own = 256;               // vertex rows a tile owns (<= T = threads per workgroup): tile t owns rows [t*own, (t+1)*own)
  int n_tiles = 0;             // tiles covering real vertices
  int n_tiles_padded = 0;      // multiple of shard_count
  int tiles_per_shard = 0;
  int64_t nvp = 0;             // padded vertex rows = n_tiles_padded * own
  std::vector<int32_t> perm;   // internal row -> external row   (nv)
  std::vector<int32_t> iperm;  // external row -> internal row   (nv)
  std::vector<int32_t> tile_facet_off;  // n_tiles+1
  std::vector<TileFacet> tile_facets;   // facet instances
  std::vector<int32_t> tile_facet_ext;  // external facet row of each instance
  // the lean k_energy instances' own lane order: per tile a permutation of tile_facets' records; tiles below the
  // ordering threshold are copies
  std::vector<TileFacet> tile_facets_lean;
  LaneModel model_common, model_lean;   // lane_order_model of the two arrays
  std::vector<int32_t> tile_halo_off;   // n_tiles+1
  std::vector<int32_t> halo_ids;        // internal vertex ids
  // per-tile vertex -> corner CSR (deterministic gather order): for owned vertex i of
  // tile t the entries vent[tile_ent_off[t] + voff[t*(T+1)+i] ... +voff[t*(T+1)+i+1])
  // are (facet_local << 2 | corner), ascending in facet_local.
  std::vector<int32_t> tile_ent_off;    // n_tiles+1
  std::vector<uint16_t> tile_voff;      // n_tiles*(T+1)
  std::vector<uint16_t> vent;
  int max_ent = 0;
  int max_halo = 0;
  int max_tile_facets = 0;
  int64_t dropped_facets = 0;
};

// Builds the patch ordering + tiles.  Returns MS_OK or MS_ERR_*; `err` gets text.
int build_tiling(int nv, int nf, const double* positions, const int32_t* tri,
                 const uint8_t* body_facets, int T, int shard_count, Tiling& out,
                 std::string& err);

// Scores `recs` (the tiling's tile_facet_off ranges) with the LDS bank model above.
LaneModel lane_order_model(const Tiling& t, const TileFacet* recs, int tile0, int tile1);

// ---- device-side view handed to kernels ---------------------------------
struct DeviceMesh {
  int nv, T, n_tiles;
  int own;                // vertex rows per tile (<= T = threads per workgroup)
  int has_boundary;       // any vertex carries VF_BOUNDARY (uniform fast-path switch)
  const int32_t* tile_facet_off;
  const TileFacet* tile_facets;
  // the same records in 4 bytes (10 bits per corner slot | 2 flag bits) for the T = 256 instances of the two tile
  // kernels; nullptr when some tile needs more than 1024 LDS slots (those instances are not used then)
  const uint32_t* tile_facets32;
  // what the lean k_energy instances (energy_body's LEANE) read instead: the same records per tile in a lane order
  // chosen for the LDS atomics and gathers they issue -- or tile_facets32 itself (MS_LANE_ORDER=0)
  const uint32_t* tile_facets_lean;
  int no_fast;            // MS_NO_FAST at ms_create: never pick the T = 256 instances (A/B switch)
  const double* tf_gamma;  // surface tension per facet instance
  // uniform-parameter shortcuts: when every facet carries the same surface tension (every vertex the same kappa and
  // c0) the kernels take the value from here and the per-facet / per-vertex arrays are not read at all
  int gamma_uniform, kc_uniform;
  double gamma_const, kappa_const, c0_const;
  const int32_t* tile_halo_off;
  const int32_t* halo_ids;
  const int32_t* tile_ent_off;
  const uint16_t* tile_voff;
  const uint16_t* vent;
  const uint8_t* vflags;  // nvp
  const double* kappa;    // nvp
  const double* c0;       // nvp
};

struct EnergyArgs {
  DeviceMesh m;
  int tile0, tile1;       // this shard's tile range
  const double* x;        // base positions
  const double* d;        // direction or nullptr
  double alpha;
  double* xt;             // trial positions out or nullptr
  double* fK;             // (nvp,3) out or nullptr
  double* fA;             // (nvp,2) out or nullptr
  double* partials;       // [n_tiles][MS_NSCAL]
  int bending_model;
  uint32_t modules;
  // bending_tilt: per-vertex record {base = 2H - c0 (0 on boundary), A_eff, kappa*ratio*H, 0}
  // written instead of the final factors; fK then holds K_dir * kappa * ratio (k_bt finishes)
  double* bt_vert;
  // queued stage (nullptr: unconditional): run only if the decision word holds `gate_want` (see DEC_*)
  const uint32_t* gate;
  uint32_t gate_want;
  // nonzero: never the lean instance (MS_KA_LEAN=0 at ms_create, a one-tile mesh; launch_energy sets it under a
  // k_exec recorder)
  uint32_t lean_off = 0;
  const double* bt_normals;  // leaflet bending_tilt: unit vertex normals of the evaluated positions (signed H, K_dir = n)
  // energy-only evaluation of BOTH leaflets' bending_tilt in one launch: the second leaflet's record from the same
  // curvature sums with its own (kappa, c0) (no factor outputs: fK / fA serve one leaflet at a time)
  double* bt_vert2 = nullptr;
  const double* kappa2 = nullptr;
  const double* c02 = nullptr;
  int atomic;             // accumulate per-vertex sums with LDS atomics (not bitwise reproducible)
  // multi-trial launch (pair = n >= 2): trials 0 .. n-2 of the ladder are evaluated in the same launch at alpha_side[j]
  // into partials_side[j] (energy only unless xt/fK/fA_side[j] are given: j < 2), trial n-1 at `alpha` with the
  // ordinary outputs
  int pair;
  double alpha_side[MS_MAX_TRIALS - 1];
  double* partials_side[MS_MAX_TRIALS - 1];
  double* xt_side[2];
  double* fK_side[2];
  double* fA_side[2];
};

struct GradientArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* fK;
  const double* fA;
  double* g;
  double* gC;             // or nullptr
  double* partials;
  const double* scal;     // device scalars (volume for the penalty factor)
  uint32_t modules;
  int bending_grad_mode;
  double volume_stiffness, target_volume;
  double area_stiffness, target_area;  // body_area_penalty: k and A0 (K_C's effective tension k (A - A0))
  int accumulate;         // add into existing g instead of overwriting
  // fused direction pass (only when no constraint row has to be projected out first)
  int dir_mode;           // 0 off, 1 d = -g (GD / CG restart), 2 per-row Polak-Ribiere with history
  double* d;
  const double* pg;
  const double* pd;
  // queued behind a line search (nullptr: unconditional): run only if the decision word holds `gate_want`
  const uint32_t* gate;
  uint32_t gate_want;
  int pd_neg_pg;           // the previous direction is -pg (an implicit steepest-descent step): derive, do not load
  int atomic;
  // leaflet bending_tilt (BENDMODE 3): per-corner fA_eff = 1/2 kappa_k (base_k + s div_f t)^2
  const double* bt_vert;   // (nvp,4): [0] = base
  const double* tilts;     // (nvp,3) the leaflet's tangent tilts
  double div_sign;
};

struct TiltArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* d;        // direction or nullptr (energy at x + alpha d)
  double alpha;
  const double* tilts;    // (nvp,3) tilts read by every mode
  double* tilts_out;      // mode 2: projected tilts are written here (may alias `tilts`)
  double k_tilt;
  double* g;              // mode 1: shape gradient is ADDED into g
  double* tilt_grad;      // mode 1: k_t t_v A_v (written)
  double* minv;           // mode 3: Jacobi preconditioner 1/(k_t A_v) (normals go to tilts_out)
  double* partials;
  int e_slot;             // reduction slot of the energy partial (MS_S_ETILT / _IN / _OUT)
  int consistent;         // tilt_leaflet.py:101-114: consistent P1 mass coeff (energy / shape gradient)
  int tg_accumulate;      // mode 1: ADD the tilt gradient instead of writing it
  int cons_tilt_grad;     // mode 1 with `consistent`: the tilt gradient takes the consistent P1 mass too,
                          // k A_f/12 (2 t_k + t_a + t_b) per corner (tilt_leaflet.py:124-150), instead of k t_v A_v
  double* va_out;         // mode 3: barycentric vertex areas (nvp) or nullptr
  double* fields;         // mode 5: curvature fields, four planes of (fields_rows, 3) -- see k_tilt
  int64_t fields_rows;
  // mode 3, the set-up of a relaxation in the same launch: proj_out receives P(tilts) of the owned rows (k_tvec mode 2
  // with step 0, on the normals just formed); finish_minv: `minv` receives the clamped INVERSE of the diagonal (k_tvec
  // mode 3: 1 where the diagonal is <= 1e-12 and on rows clamped by fixed_bit) -- when no smoothness term is to be
  // added to the diagonal first
  double* proj_out = nullptr;
  int finish_minv = 0;
  int fixed_bit = 0;
  // mode 3 also as the projection pass of up to two more fields (mode 2's arithmetic on the same normals):
  // fld_out[k] <- fld_in[k] - (fld_in[k].n) n on the owned rows -- the leaflet trial projections of an energy evaluation
  // that needs the normals anyway (bending_tilt_in/out)
  const double* fld_in[2] = {nullptr, nullptr};
  double* fld_out[2] = {nullptr, nullptr};
  // mode 3 as the set-up of a TWO-field relaxation in one launch (the normals and the vertex areas are the same): the
  // second field's projection, diagonal and area outputs
  const double* tilts_b = nullptr;
  double* proj_out_b = nullptr;
  double* minv_b = nullptr;
  double* va_out_b = nullptr;
  double k_tilt_b = 0.0;
  int finish_minv_b = 0;
  int fixed_bit_b = 0;
  // leaflet absence (leaflet_presence.py:158-170): a facet with a corner that carries this flag bit is no part of the
  // field.  Modes 0 / 1: it adds no energy, no shape-gradient and no tilt-gradient rows (tilt_leaflet.py:77-167).  Mode
  // 3: the field's vertex areas -- va_out and the diagonal -- skip it (tilt_relaxation.py:681-697); the normals do
  // not.  0 = no mask: the flag bytes are not staged and nothing else changes.
  int absent_bit = 0;
  int absent_bit_b = 0;
};

struct DiskTargetArgs {   // tilt_disk_target_in.py:160-286
  int tile0, tile1, nv, T, n_tiles;
  const uint8_t* vflags;
  const uint8_t* disk;    // (nvp) 1 on the tagged rows
  const double* x;
  const double* d;        // direction or nullptr (positions x + alpha d)
  double alpha;
  const double* tilts;
  double* diff;           // mode 1 / 3 out: t - theta(r) r_hat on the disk rows, 0 elsewhere
  double* target;         // mode 2 out / mode 3 in: theta(r) r_hat of the tagged rows at FROZEN positions (tilt
                          // relaxations evaluate the profile dozens of times on the same surface), NaN = profile off
  double theta_b, lambda, radius;  // radius <= 0: read scal[r_slot]
  double center[3], normal[3];
  const double* scal;
  double* partials;
  int r_slot;
};
hipError_t launch_disk_target(const DiskTargetArgs& a, int mode, hipStream_t s);

struct BtArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* d;         // direction or nullptr (energy at x + alpha d)
  double alpha;
  const double* tilts;     // (nvp,3) tangent tilts
  const double* bt_vert;   // (nvp,4) from the energy pass at the same positions
  double* fK;              // mode 1: in K_dir*kappa*ratio, out the back-prop factor
  double* fA;              // mode 1: out {fA_eff, fA_vor}
  double* tilt_grad;       // mode 2: dE/dt ADDED here
  double* partials;
  double* g;               // mode 3: shape gradient of the divergence term ADDED here
  double div_sign;         // -1 inner leaflet, +1 outer leaflet / single field
  int e_slot;              // reduction slot of the energy partial (MS_S_EBT / _IN / _OUT)
  // mode 0 only: also the tilt-magnitude energy of the same field (modules/energy/tilt.py:99-172, per-facet form) from
  // the rows this kernel has staged anyway -- k_tilt's energy-only launch is not needed then.  0 = off.
  double k_tilt_fused;
  int e_tilt_slot;
};

struct TsArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* d;         // direction or nullptr (cotans at x + alpha d)
  double alpha;
  const double* tilts;     // (nvp,3)
  double k_smooth;
  double* tilt_grad;       // mode 1: dE/dt ADDED here
  double* diag;            // mode 2: Jacobi diagonal 1/2 k_s sum (c_a + c_b) ADDED here
  double* partials;
  int e_slot;              // reduction slot of the energy partial (MS_S_ETS / _IN / _OUT)
  int absent_bit = 0;      // modes 0 / 1: facets with a corner that carries this flag bit drop out with their weights
                           // (tilt_smoothness_utils.py:57-68); 0 = no mask
};

// stream kernels (one workgroup of BLOCK threads per tile): their arguments as structs, so that the same device body
// serves the ordinary launch and the one-workgroup interpreter (k_exec)
struct TvecArgs {
  int mode, tile0, nv, T;
  const uint8_t* vflags;
  double* tg;
  const double* minv;
  double* dir;
  const double* tilts;
  const double* src;
  const double* normals;
  double* out;
  double coef;
  const double* coef_dev;  // device programs (k_exec): the coefficient is read from here instead (nullptr: `coef`)
  int flag;
  double* partials;
  int n_tiles;
  uint8_t fixed_bit;
  int s_gn2, s_rz;
};
struct DirectionArgs {
  int tile0, nv, T;
  const uint8_t* vflags;
  double* g;
  const double* gC;
  double* d;
  const double* pg;
  const double* pd;
  const double* scal;
  int use_constraint, cg_history;
  double* partials;
  int n_tiles, write_g;
  const uint32_t* gate;
  uint32_t gate_want;
  int pd_neg_pg, precond;
};
// pin_to_plane / pin_to_circle (ms_pins.hip): the staged enforcement program and the project lane's gradient pass
struct PinEnforceArgs {
  double* x;
  const double* params;  // 7 per row: normal, point / centre / base, radius (< 0: the mean radial distance)
  int n_stages;
  const int32_t* stage_kind;
  const int32_t* stage_param;
  const int32_t* stage_off;
  const int32_t* item_row;
  const int32_t* item_arg;
};
struct PinGradArgs {
  const double* x;
  double* g;
  double* gc;  // the volume row, or nullptr
  const double* params;
  int n_grad;
  const int32_t* grad_row;
  const int32_t* grad_kind;
  const int32_t* grad_param;
  int n_avg;
  const int32_t* avg_param;
  const int32_t* avg_off;
  const int32_t* avg_row;
  int n_touch;
  const int32_t* touch_row;
  double* partials;
  int n_tiles, tile;
};
// record: on a stream with a recorder the program becomes a record of the pack (CK_PIN_ENFORCE / CK_PIN_GRAD) instead of
// a launch behind a flush
hipError_t launch_pin_enforce(const PinEnforceArgs& a, hipStream_t s, bool record);
hipError_t launch_pin_grad(const PinGradArgs& a, hipStream_t s, bool record);
// The edge lane (ms_edge.hip): line_tension, E = sum gamma |x_h - x_t| over the tagged edges, and edge_length_penalty,
// E = sum (0.5 k) (|x_h - x_t| - L0)^2 over the edges that carry a target length.  A term's energy is added into the
// MS_S_ESURF partials behind the energy pass and its gradient into G behind the gradient pass, line_tension's launch
// before edge_length_penalty's.  Both terms use one table layout: `col` is gamma or L0.  Rows are the library's
// (til.iperm applied).
enum : int { EDGE_LINE = 0, EDGE_PEN = 1 };
struct EdgeEnergyArgs {
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what EnergyArgs hands k_energy
  double alpha;
  const uint8_t* vflags;  // (a fixed row does not move in a trial)
  double k;               // EDGE_PEN: edge_stiffness (global only)
  int n_edges;
  const int32_t* tail;    // edge table, ascending edge order (EDGE_LINE: gamma != 0 only)
  const int32_t* head;
  const double* col;      // gamma / target length per edge
  double* partials;       // the energy pass's: workgroup w adds into [MS_S_ESURF * n_tiles + tile0 + w]
  int n_tiles, tile0;
  int grid;               // workgroups of the launch: min(tiles, ceil(n_edges / 256))
  double* wg_sums;        // [grid] per-workgroup sums ...
  uint32_t* done;         // ... counted here; the workgroup that arrives last adds them up in index order ...
  double* energy;         // ... into the module's own energy (ms_get_line_energy, ms_get_edge_penalty_energy)
};
struct EdgeGradArgs {
  const double* x;
  double* g;
  const double* gc;       // the volume row K_C wrote, or nullptr
  double k;               // EDGE_PEN: edge_stiffness
  int n_touch;
  const int32_t* vrow;    // touched rows, ascending
  const int32_t* off;     // n_touch + 1: CSR over the rows' edges of the term, ascending edge order
  const int32_t* other;   // the other end's row
  const double* col;      // gamma / target length of the edge, per CSR entry
  double* partials;       // the gradient pass's: workgroup w adds sum dg_v . gC_v into [MS_S_GGC * n_tiles + tile0 + w]
  int n_tiles, tile0;
  int grid;
};
hipError_t launch_edge_energy(int term, const EdgeEnergyArgs& a, hipStream_t s);
hipError_t launch_edge_grad(int term, const EdgeGradArgs& a, hipStream_t s);
// tilt_rim_source_in/out (ms_rim.hip): E = sum over the rim rows of c_row . t_row, c_row = sum over the row's rim edges
// of -1/2 gamma L r_hat; the workgroup sums go into the field's tilt-magnitude partials (MS_S_ETILT_IN / _OUT) behind
// the pass that writes them -- or define them when tilt_<leaflet> itself is off -- and c into the tilt gradient.  Rows
// are the library's (til.iperm applied).
struct RimArgs {
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what EnergyArgs hands k_energy
  double alpha;
  const uint8_t* vflags;  // (a fixed row does not move in a trial)
  int n_touch;
  const int32_t* vrow;    // rim rows, ascending
  const int32_t* off;     // n_touch + 1: CSR over the rows' rim edges, ascending edge order
  const int32_t* other;   // the other end's row
  const double* gamma;    // the edge's strength, per CSR entry
  double center[3];       // fixed frame: tilt_rim_source_center
  double normal[3];       // unit normal of the circle's plane
  const double* center_dev;  // follow mode: the center k_rim_frame wrote (else nullptr)
  double* coef;           // [3 n_touch] c_row: k_rim_coef writes it, k_rim_apply reads it when use_coef ...
  int use_coef;           // ... and forms the rows itself when not
  const double* tilts;
  double* tilt_grad;      // c_row added into the row, or nullptr
  double* partials;       // workgroup w -> [slot * n_tiles + tile0 + w]
  int n_tiles, tile0, n_cells;  // n_cells: tiles of the context (define: the cells past `grid` are zeroed)
  int slot, define;       // define: store (no pass before this one wrote the slot) instead of add
  int grid;               // workgroups of the launch: min(tiles, ceil(n_touch / 256))
  double* wg_sums;        // [grid] per-workgroup sums ...
  uint32_t* done;         // ... counted here; the workgroup that arrives last adds them up in index order ...
  double* energy;         // ... into the module's own energy (ms_get_leaflet_rim_source_energy)
};
hipError_t launch_rim_frame(const RimArgs& a, double* center_out, hipStream_t s);
hipError_t launch_rim_coef(const RimArgs& a, hipStream_t s);
hipError_t launch_rim_apply(const RimArgs& a, hipStream_t s);
// tilt_rim_source_bilayer: k_rim_apply on both leaflet fields at once (a.tilts / a.tilt_grad the inner leaflet's, t_out /
// tg_out the outer one's; tg_out is read only where a.tilt_grad is set); the sums go into a.slot = MS_S_ETILT_OUT
hipError_t launch_rim_apply2(const RimArgs& a, const double* t_out, double* tg_out, hipStream_t s);
// tilt_thetaB_contact_in (ms_thetab.hip): the ring rows ordered by angle on x (+ alpha d) by ONE workgroup
// (k_thetab_geom: the per-row table w / r_hat / keep and the record {wsum, R_eff, n_kept, contributes}), then
// k_thetab_apply on that table: theta_i = t_in,i . r_hat_i, the energy of the active modes into the inner leaflet's
// tilt-magnitude partials (cell 0 of MS_S_ETILT_IN, added or defined), the rows of the tilt gradient on request and
// {sum w theta / wsum, R_eff, wsum} for the scalar update.  Rows are the library's (til.iperm applied), in the
// setter's order (ties of the angular order are broken by that order).
struct ThetabArgs {
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what EnergyArgs hands k_energy
  double alpha;
  const uint8_t* vflags;  // (a fixed row does not move in a trial)
  int n;                  // ring rows, 1 .. MS_THETAB_MAX_ROWS
  const int32_t* rows;
  double center[3];       // tilt_thetaB_center
  double normal[3];       // unit normal of the ring's plane
  double u[3], v[3];      // in-plane axes (tilt_thetaB_contact_in.py:97-111)
  double* w;              // [n] arc-length weight of the row, formed on the full ring
  double* rhat;           // [3 n] in-plane unit vector from the center
  int32_t* keep;          // [n] |r| > 1e-12
  double* rec;            // {wsum over the kept rows, R_eff, n_kept, 1 when the ring contributes / 0 for the 1e-12 returns}
  const double* tilts;    // inner leaflet
  double* tilt_grad;      // the rows' gradient added here, or nullptr
  double k, gamma, theta_b;
  int field_linear, penalty;
  double* partials;       // the energy -> [slot * n_tiles + tile0]; nullptr: scalars only (no cell, no energy written)
  int n_tiles, tile0, n_cells;  // n_cells: tiles of the context (define: the cells past the first are zeroed)
  int slot, define;       // define: store (no pass before this one wrote the slot) instead of add
  double* wg_sums;        // [1] the workgroup's sum ...
  uint32_t* done;         // ... counted here (publish_wg_sum, one workgroup) ...
  double* energy;         // ... into the module's own energy (ms_get_thetab_contact_energy)
  double* scalars;        // {sum w theta / wsum, R_eff, wsum}; all 0 when the ring contributes nothing
};
hipError_t launch_thetab_geom(const ThetabArgs& a, hipStream_t s);
hipError_t launch_thetab_apply(const ThetabArgs& a, hipStream_t s);
// rim_slope_match_out (ms_rimmatch.hip): the rim, outer and optional disk rings ordered by angle on x (+ alpha d) by ONE
// workgroup (k_rsm_geom: the ordered rows, the rim table r_hat / w / phi / 1/dr / valid, the pairing idx0 / w0 / w1 with
// the outer ring -- identity or arc-length interpolation --, the first rim entry of every outer row, the disk table
// r_hat_d / w_d and the record {n_valid, contributes, local_disk, sum w_d}), then k_rsm_apply on those tables: both
// energies into cell 0 of the leaflets' tilt-magnitude partials (added or defined), the rows of the two tilt gradients
// and of the shape gradient on request.  Rows are the library's (til.iperm applied), in the setter's order (ties of the
// angular order are broken by that order); the three tables are pairwise disjoint.
struct RsmArgs {
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what EnergyArgs hands k_energy
  double alpha;
  const uint8_t* vflags;  // (a fixed row does not move in a trial)
  int n_rim, n_out, n_disk;  // ring rows, each 0 .. MS_RIM_MATCH_MAX_ROWS (n_rim, n_out >= 1; n_disk == 0: no disk term)
  const int32_t* rows_rim;
  const int32_t* rows_out;
  const int32_t* rows_disk;
  double center[3];       // rim_slope_match_center
  double normal[3];       // unit normal of the rings' plane
  double u[3], v[3];      // in-plane axes (geometry/plane_ops.py:21-41)
  double k;               // rim_slope_match_strength
  // k_rsm_geom writes, k_rsm_apply reads; indexed by the position in the ring's angular order
  int32_t* orow_rim;      // [n_rim] the rim's rows in angular order
  int32_t* orow_out;      // [n_out]
  int32_t* orow_disk;     // [n_disk]
  double* rhat;           // [3 n_rim] in-plane unit vector from the center, 0 where |r| <= 1e-12
  double* w;              // [n_rim] arc-length weight on the ordered rim, 0 where the entry is not valid
  double* phi;            // [n_rim] (h_out - h_rim) / (r_out - r_rim), 0 where not valid
  double* inv_dr;         // [n_rim] 1 / dr, 0 where not valid
  int32_t* valid;         // [n_rim]
  int32_t* idx0;          // [n_rim] the outer entry below the rim entry's arc-length parameter (idx1 = idx0 + 1 mod n_out) ...
  double* w0;             // [n_rim] ... and the two interpolation weights; identity pairing: idx0 = i, w0 = 1, w1 = 0
  double* w1;
  int32_t* first0;        // [n_out + 1] first rim entry with idx0 >= j: idx0 is monotone, so the entries of an outer row are a range
  double* s_out;          // [n_out] arc-length knots of the ordered outer ring (interpolation only)
  double* rhat_d;         // [3 n_disk] the disk rows' r_hat, 0 where |r| <= 1e-12
  double* w_d;            // [n_disk] arc-length weight on the ordered disk ring, 0 where |r| <= 1e-12
  double* dif;            // [n_rim] k_rsm_apply's scratch: diff, ...
  double* dif_in;         // [n_rim] ... diff_in of the launch
  double* rec;            // {n_valid, 1 when the rings contribute / 0 for the early returns, local_disk, sum w_d} and
                          // k_rsm_apply's {E_out, E_in}
  const double* t_in;     // inner leaflet (read only when n_disk > 0)
  const double* t_out;    // outer leaflet
  double* tg_in;          // the rows' gradients added here, or nullptr
  double* tg_out;
  double* g;              // the shape gradient's rows added here, or nullptr (grad_arr=None of the reference)
  double* partials;       // E_out -> [slot_out * n_tiles + tile0], E_in -> [slot_in * n_tiles + tile0]
  int n_tiles, tile0, n_cells;  // n_cells: tiles of the context (define: the cells past the first are zeroed)
  int slot_out, slot_in;
  int define_out, define_in;  // store (no pass before this one wrote the slot) instead of add; -1: leave the slot alone
  double* wg_sums;        // [1] the workgroup's sum ...
  uint32_t* done;         // ... counted here (publish_wg_sum, one workgroup) ...
  double* energy;         // ... into the module's own energy (ms_get_rim_match_energy)
};
hipError_t launch_rsm_geom(const RsmArgs& a, hipStream_t s);
hipError_t launch_rsm_apply(const RsmArgs& a, hipStream_t s);
// tilt_thetaB_boundary_in (ms_thetab_bnd.hip): the constraint t_in . d = theta_B on a ring of rows.  k_tbb_geom writes
// the per-row table (d, the unit vertex normal N_v, keep) from x (+ alpha d), or from a trial buffer handed in as x;
// k_tbb_apply<0/1/2> enforces in place, writes P(enforce(t)) into another buffer, or projects a gradient.  Rows are
// the library's (til.iperm applied), in the setter's order.
struct TbbArgs {
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what EnergyArgs hands k_energy
  double alpha;
  const uint8_t* vflags;  // (a fixed row does not move in a trial; the field's fixed bit skips a row of an apply)
  int n;                  // ring rows, any number
  const int32_t* rows;
  const int32_t* off;     // n + 1: CSR over the rows' incident facets, ascending facet order
  const int32_t* fv;      // three rows per CSR entry: the facet's corners in its own order
  double center[3];       // tilt_thetaB_center
  double normal[3];       // unit normal of the ring's plane
  double* dir;            // [3 n] d, 0 where the row is dropped
  double* nrm;            // [3 n] N_v
  uint8_t* keep;          // [n]
  double* field;          // apply: the inner tilts (modes 0 / 1) or the inner tilt gradient (mode 2)
  double* out;            // mode 1: where P(enforce(t)) of the ring rows goes
  double theta_b;
  int project;            // mode 0: t <- t - (t . N_v) N_v behind the enforcement
  uint8_t fixed_bit;      // the inner field's
};
hipError_t launch_tbb_geom(const TbbArgs& a, hipStream_t s);
hipError_t launch_tbb_apply(int mode, const TbbArgs& a, hipStream_t s);
// tilt_coupling (ms_couple.hip): E = 1/2 k_c int |t_out + s t_in|^2 dA, k_tilt's lumped arithmetic on the field
// d = t_out + s t_in.  k_couple<0/1> per tile on x (+ alpha d); k_couple_vec per vertex on the frozen surface's areas.
struct CoupleArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what TiltArgs hands k_tilt
  double alpha;
  const double* t_in;     // (nvp,3) both leaflets' tilts
  const double* t_out;
  double k_c, sign;       // tilt_coupling_modulus; -1.0 "difference" / +1.0 "sum"
  double* g;              // k_couple<1>: shape gradient ADDED, or nullptr
  double* tg_in;          // k_c s d_v A_v ADDED, or nullptr
  double* tg_out;         // k_c d_v A_v ADDED, or nullptr
  const double* va;       // k_couple_vec: barycentric vertex areas of the frozen positions (nvp)
  double* partials;       // the tile's cell [slot * n_tiles + tile] ...
  int slot, cell_mode;    // ... 0 left alone, 1 added to (a pass before this one defined it), 2 defined
  double* wg_sums;        // [tile1 - tile0] per-workgroup sums: the module's own energy is their sum in index order,
                          // taken on the host when asked for (ms_get_tilt_coupling_energy)
};
size_t couple_lds_bytes(int T, int cap, int max_ent, int mode);
hipError_t launch_couple(const CoupleArgs& a, int mode, int cap, int max_ent, hipStream_t s);
hipError_t launch_couple_vec(const CoupleArgs& a, int with_grad, hipStream_t s);
// tilt_splay_twist_in (ms_splay.hip): E = 1/2 sum_f A_f (k_splay div^2 + k_twist curl_n^2) of the inner leaflet's tilts,
// k_tsmooth's data flow.  k_splay<0/1> per tile on x (+ alpha d).
struct SplayArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* d;        // trial direction or nullptr, alpha: exactly what TsArgs hands k_tsmooth
  double alpha;
  const double* tilts;    // (nvp,3) the inner leaflet's tilts
  double k_splay, k_twist;
  double* tilt_grad;      // k_splay<1>: dE/dt ADDED here
  double* partials;       // the tile's cell [slot * n_tiles + tile] ...
  int slot, cell_mode;    // ... 0 left alone, 1 added to (a pass before this one defined it), 2 defined
  double* wg_sums;        // [tile1 - tile0] per-workgroup sums: the module's own energy is their sum in index order,
                          // taken on the host when asked for (ms_get_tilt_splay_twist_energy)
};
size_t splay_lds_bytes(int T, int cap, int max_ent, int mode);
hipError_t launch_splay(const SplayArgs& a, int mode, int cap, int max_ent, hipStream_t s);
// The hard area constraints (ms_area.hip): body_area's KKT row and the enforcers of body_area / global_area.  The lane's
// sums live in partial rows and result cells of its own (the mailbox has one slot left): part[AP_ROWS][n_tiles], written
// by k_area_row (AP_A, AP_GAGA) and k_area_dots (the rest), folded in tile order by k_area_fold into res[0 .. AP_ROWS),
// which also leaves the multipliers of the projection in res[AP_LAMV], res[AP_LAMA].
enum : int { AP_A = 0, AP_GAGA, AP_GGV, AP_GGA, AP_GVGV, AP_GVGA, AP_ROWS, AP_LAMV = AP_ROWS, AP_LAMA, AP_RES };
struct AreaRowArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  double* ga;             // (nvp,3) out: dA/dx of the owned rows
  double* part;
  int all_facets;         // global_area: every facet; else the facets that carry TF_BODY
  int cap;
};
struct AreaProjArgs {
  int tile0, tile1, nv, own, n_tiles;
  double* g;
  const double* gv;       // the volume row K_C wrote, or nullptr
  const double* ga;
  double* part;
  const double* res;
};
size_t area_row_lds_bytes(int T, int cap, bool atomic);
hipError_t launch_area_row(const AreaRowArgs& a, bool atomic, hipStream_t s);
hipError_t launch_area_dots(const AreaProjArgs& a, hipStream_t s);
hipError_t launch_area_fold(const double* part, double* res, int n_tiles, int tile0, int tile1, int rows, hipStream_t s);
hipError_t launch_area_apply(const AreaProjArgs& a, hipStream_t s);
// The enforce-only constraints (ms_enforce.hip): fixed_plane's projection of a position buffer and perimeter's loops.
struct FixedPlaneArgs {
  int64_t nv;             // the real rows: nv .. nvp are never touched
  const uint8_t* vflags;
  double* x;
  double n[3], q[3];      // unit normal, point of the plane
};
// perimeter's tables (ms_api_enforce.inc builds them): loop l owns the entries loop_off[l] .. loop_off[l + 1) (tail / head
// in library rows, list order, duplicates kept) and the distinct vertices vert_off[l] .. vert_off[l + 1) (vrow, in order of
// first appearance); vertex j's incident entries are csr_ent[csr_off[j] .. csr_off[j + 1)) in list order, -(entry + 1) where
// it is the tail and +(entry + 1) where it is the head.  ent / gv: scratch of 4 x the longest loop's entries / vertices.
struct PerimeterArgs {
  int n_loops;
  const int32_t *loop_off, *tail, *head, *vert_off, *vrow, *csr_off, *csr_ent;
  const double* target;
  const uint8_t* vflags;
  double* x;
  double *ent, *gv;
  int max_ent, max_verts;
  double* res;            // [2 n_loops]: passes that moved something, P of the last evaluation
  double tol;
  int max_iter;
};
hipError_t launch_fixed_plane(const FixedPlaneArgs& a, hipStream_t s);
hipError_t launch_perimeter(const PerimeterArgs& a, hipStream_t s);
struct RowDotArgs {
  int tile0, nv, T;
  const double* g;
  const double* gC;
  double* partials;
  int n_tiles;
};
struct AxpyMaskedArgs {
  int64_t n_rows;
  const uint8_t* vflags;
  double* x;
  const double* y;
  double coef;
};

// ---- the one-workgroup interpreter (k_exec) ------------------------------------------------------------------------
// When a context's mesh is ONE tile, every kernel of the library is one workgroup (folds: a handful), a step is dozens of
// launches of a few microseconds of work each, and what the step costs is launches and host round trips.  Such a
// context attaches an ExecRecorder to its stream: the launchers then append {kind, instance, arguments} records to a
// pack instead of launching, and the pack is launched as ONE kernel -- k_exec, one workgroup, which runs the recorded
// device bodies (the same code as the ordinary kernels) in order, a workgroup barrier between them -- when the host
// needs the device to make progress (it is about to wait for a mailbox, or touches the stream directly).  The pack
// travels as the kernel's argument block.  Results are bit for bit those of the launch-per-kernel path.
enum : uint16_t {
  CK_ENERGY = 1, CK_GRADIENT, CK_TILT, CK_BT, CK_TS, CK_TVEC, CK_DISK, CK_REDUCE, CK_DIRECTION, CK_ROWDOT,
  CK_AXPY_MASKED, CK_MEMSET, CK_RELAX, CK_RELAX_FUSED, CK_TSEARCH,  // (CK_TSEARCH: the single-step-size form of k_tsearch, mode = fields)
  CK_PIN_ENFORCE, CK_PIN_GRAD  // the pin program and the project lane's pass (ms_pins_dev.h), one workgroup each
};
struct ExecCmdHead {
  uint16_t kind;
  uint16_t bytes;     // of the whole record (head + arguments), a multiple of 8
  int32_t mode;       // template MODE of the tilt-family kernels, launch mode of the stream kernels
  int32_t cap, max_ent;
  int32_t grid;       // blocks of the ordinary launch: the body runs for block 0 .. grid-1 in turn
  uint32_t inst;      // template instance (energy / gradient: EnergyInst::code() / GradientInst::code())
  int32_t mesh;       // which DeviceMesh of the pack head the tile kernels' arguments go with
  int32_t pad;
};
static_assert(sizeof(ExecCmdHead) == 32, "ExecCmdHead is 32 bytes");

// Which template instance of the energy / gradient kernels runs.  energy_instance() / gradient_instance() choose one
// from the arguments, visit_instance() (ms_kernels.hip) turns it into template parameters for the launchers and for
// k_exec alike, valid() is the list of instances that are compiled, in_exec() the part of it k_exec has, and code() is
// ExecCmdHead::inst (what ms_exec_trace reports).
struct EnergyInst {
  bool bend, guard, atomic, area, fast;  // fast: the T = 256 instances
  int multi;                             // trial positions per launch: 0 (one), 2, 3 or 8
  bool lean = false;                     // the headline instances (energy_body's LEANE), every multi
  constexpr bool valid() const {
    return (bend || !atomic) && (multi == 0 || ((multi == 2 || multi == 3 || multi == 8) && bend && !guard && !area)) &&
           (!lean || (bend && !guard && atomic && fast && !area));
  }
  // (k_exec keeps the general instances: a lean one has no code())
  constexpr bool in_exec() const { return valid() && fast && multi == 0 && !lean; }
  // bit 0 bending, bit 1 guard, bit 2 LDS-atomic vertex sums, bit 3 body area (body_area_penalty)
  constexpr uint32_t code() const { return (bend ? 1u : 0u) | (guard ? 2u : 0u) | (atomic ? 4u : 0u) | (area ? 8u : 0u); }
  static constexpr EnergyInst from_code(uint32_t c) {
    return {(c & 1u) != 0, (c & 2u) != 0, (c & 4u) != 0, (c & 8u) != 0, true, c < 16u ? 0 : -1};
  }
  constexpr bool operator==(const EnergyInst& o) const {
    return bend == o.bend && guard == o.guard && atomic == o.atomic && area == o.area && fast == o.fast && multi == o.multi &&
           lean == o.lean;
  }
};
static_assert(EnergyInst{true, false, true, false, true, 3, true}.valid() && !EnergyInst{true, false, true, false, true, 0, true}.in_exec() &&
                  !EnergyInst{true, false, false, false, true, 0, true}.valid() && !EnergyInst{true, true, true, false, true, 0, true}.valid(),
              "EnergyInst: lean goes with the T = 256 LDS-atomic bending instances only and is never one of k_exec's");
struct GradientInst {
  int mode;  // bending: 0 none, 1 analytic, 2 approx, 3 leaflet bending_tilt (generic-size instances only)
  bool volrow, atomic, lean, area, fast;
  constexpr bool valid() const {
    return mode >= 0 && mode <= 3 && (!lean || (mode == 1 && fast && !area)) && (mode != 3 || (!area && !fast));
  }
  constexpr bool in_exec() const { return valid() && (fast || mode == 3); }
  // bit 0 lean, bit 1 constraint row, bit 2 LDS-atomic vertex sums, bit 3 body-area penalty term, bits 4-5 bending mode
  constexpr uint32_t code() const {
    return (lean ? 1u : 0u) | (volrow ? 2u : 0u) | (atomic ? 4u : 0u) | (area ? 8u : 0u) | ((uint32_t)mode << 4);
  }
  static constexpr GradientInst from_code(uint32_t c) {
    return {c < 64u ? (int)(c >> 4) : -1, (c & 2u) != 0, (c & 4u) != 0, (c & 1u) != 0, (c & 8u) != 0, (c >> 4) != 3u};
  }
  constexpr bool operator==(const GradientInst& o) const {
    return mode == o.mode && volrow == o.volrow && atomic == o.atomic && lean == o.lean && area == o.area && fast == o.fast;
  }
};
// every instance k_exec has is its own code's instance, and every code is either refused or the code of its instance
constexpr bool inst_codes_round_trip() {
  for (uint32_t c = 0; c < 64u; ++c) {
    const EnergyInst e = EnergyInst::from_code(c);
    const GradientInst g = GradientInst::from_code(c);
    if (e.in_exec() != e.valid() || (e.in_exec() && e.code() != c)) return false;
    if (g.in_exec() != g.valid() || (g.in_exec() && g.code() != c)) return false;
  }
  for (uint32_t b = 0; b < 32u; ++b)
    for (int m = 0; m < 4; ++m) {
      const EnergyInst e = {(b & 1u) != 0, (b & 2u) != 0, (b & 4u) != 0, (b & 8u) != 0, (b & 16u) != 0, m == 0 ? 0 : (m == 3 ? 8 : m + 1)};
      const GradientInst g = {m, (b & 1u) != 0, (b & 2u) != 0, (b & 4u) != 0, (b & 8u) != 0, (b & 16u) != 0};
      if (e.in_exec() && !(EnergyInst::from_code(e.code()) == e)) return false;
      if (g.in_exec() && !(GradientInst::from_code(g.code()) == g)) return false;
    }
  return true;
}
static_assert(inst_codes_round_trip(), "EnergyInst / GradientInst: code() and from_code() are inverses on k_exec's instances");
static_assert(EnergyInst{true, true, true, true, true, 0}.code() == 15u && EnergyInst{true, false, true, false, true, 0}.code() == 5u &&
                  EnergyInst{false, true, false, false, true, 0}.code() == 2u && EnergyInst{true, false, false, true, true, 0}.code() == 9u,
              "ExecCmdHead::inst of an energy record: bend 1, guard 2, atomic 4, area 8");
static_assert(GradientInst{1, true, true, true, false, true}.code() == 0x17u && GradientInst{3, false, false, false, false, false}.code() == 0x30u &&
                  GradientInst{1, true, false, false, true, true}.code() == 0x1au && GradientInst{2, false, false, false, false, true}.code() == 0x20u,
              "ExecCmdHead::inst of a gradient record: lean 1, volrow 2, atomic 4, area 8, mode << 4");
constexpr int EXEC_MESHES = 3;       // distinct DeviceMesh values per pack (plain, inner leaflet, outer leaflet)
constexpr int EXEC_PACK_BYTES = 3968;  // kernel-argument block of one k_exec launch (HIP allows 4096)
struct ExecPackHead {
  int32_t n_cmds, bytes;
  int32_t T, pad;
  // diagnostic (ms_exec_trace): when set, thread 0 appends {kind << 32 | mode, duration in 10 ns ticks} per record run;
  // word 0 of the buffer counts the entries
  unsigned long long* stamps;
  DeviceMesh m[EXEC_MESHES];
};
constexpr int EXEC_STAMP_CAP = 1 << 16;
struct ExecMemsetArgs {
  double* p;
  int64_t n;  // doubles
};
// CK_RELAX: the tilt relaxation (TiltRelaxationManager.relax_tilts / relax_leaflet_tilts,
// runtime/steppers/tilt_relaxation.py:237-424, 426-1478) as a PROGRAM: the record is followed by command lists the
// host captured once -- "gradient at the current tilts", "trial field + its energy", "first direction", "next
// direction", each for both parities of the tilts <-> trial pointer swap an acceptance is -- and the workgroup walks
// the reference's control flow itself (Fletcher-Reeves CG or gradient descent, up to 12 halvings, accept on E1 <= E0),
// reading the folded scalars where the host would read its mailbox.  No launch and no host round trip inside a
// relaxation; the host gets {iterations, evaluations, final parity} in one mailbox post.
struct ExecRelaxHead {
  int32_t solver, max_iters, nf, n_e;
  double step_size, tol;
  int32_t e_slot[16];               // energy slots in the host's order of addition (tilt_energy_from_mailbox)
  int32_t s_gn2[2], s_rz[2];
  const double* scal;               // device scalars the lists' folds write
  double* cells;                    // [0] the trial coefficient (sign * step), [1] the Fletcher-Reeves beta
  unsigned long long* host_box;     // pinned result mailbox: entries 0..3 = iterations, evaluations, parity, status
  unsigned long long ticket;
  int32_t off_grad[2], n_grad[2];   // list offsets (bytes from the pack base) and lengths (records)
  int32_t off_trial[2], n_trial[2];
  int32_t off_dir0, n_dir0, off_dir1, n_dir1;
  int32_t total_bytes, pad;         // record + lists (the interpreter's main loop skips them)
};
// CK_RELAX_FUSED: a leaflet relaxation with the frozen geometry held on the CU (ms_relax_fused.inc)
struct ExecRelaxFusedField {
  double* tilts;              // in: the projected start field; out: the relaxed field
  const double* minv;         // Jacobi M^-1 (1 on clamped rows)
  const double* va;           // barycentric vertex areas (tilt_in / tilt_out in the vertex-area form)
  const double* bt_vert;      // (nvp,4): [0] = base_k = 2H - c0 of this leaflet
  const double* kappa;
  const double* dt_target;    // theta(r) r_hat of the tagged rows (NaN: profile off)
  const uint8_t* disk;
  double k_tilt, k_smooth, dt_strength, div_sign;
  int32_t has_tilt, has_bt, has_ts, has_dt;
  uint32_t fixed_bit, pad;
};
struct ExecRelaxFusedArgs {
  DeviceMesh m;
  const double* x;
  const double* normals;      // unit vertex normals of the frozen surface
  ExecRelaxFusedField f[2];
  int32_t nf, solver, max_iters, cap, max_ent, pad;
  double step_size, tol;
  unsigned long long* host_box;  // {iterations, evaluations, parity (0), done}
  unsigned long long ticket;
};
size_t relax_fused_lds_bytes(int cap, int max_ent, int max_tile_facets);

struct ExecRecorder {
  hipStream_t stream = nullptr;
  int T = 0;
  std::vector<unsigned char> buf;  // ExecPackHead + records
  int n_mesh = 0;
  size_t lds = 0;                  // dynamic LDS the recorded bodies need (max)
  long launches = 0, cmds = 0;     // statistics
  bool capture = false;            // records are collected for a program (CK_RELAX): no size limit, never launched
  unsigned long long* d_stamps = nullptr;  // ms_exec_trace: per-record durations go here
  // args/bytes: the kernel's argument struct; tile kernels (mesh != nullptr) are stored without their leading DeviceMesh
  hipError_t push(uint16_t kind, int mode, int cap, int max_ent, int grid, uint32_t inst, size_t lds_bytes,
                  const void* args, size_t bytes, const DeviceMesh* mesh = nullptr);
  hipError_t flush();
  // launch `pack` (ExecPackHead + records, any size up to the largest k_exec variant) as it is
  hipError_t launch_pack(const std::vector<unsigned char>& pack, size_t lds_bytes);
};
constexpr int EXEC_PACK_MID = 12160, EXEC_PACK_BIG = 28544;  // larger argument blocks for programs (CK_RELAX)
ExecRecorder* exec_find(hipStream_t s);   // the recorder attached to a stream, or nullptr
void exec_attach(ExecRecorder* r);
void exec_detach(ExecRecorder* r);
// launchers that are not recorded flush first (stream order)
inline hipError_t exec_sync(hipStream_t s) {
  ExecRecorder* r = exec_find(s);
  return r ? r->flush() : hipSuccess;
}

// the resident step kernel (ms_resident.inc): many minimizer steps of the surface (+ volume row) / gradient-descent lane
// in one launch, one workgroup per tile, grid barriers between the phases
struct ResidentArgs {
  DeviceMesh m;
  double* x;               // (nvp,3) positions: read at entry, owned rows written back at exit
  double* d;               // (unused)
  double* g;               // (nvp,3) raw gradient rows of the last evaluation (tile-boundary rows are read by the
  double* gC;              //         neighbours); (nvp,3) constraint-row rows, or nullptr
  double* partials;        // [2][2][MS_NPART][n_tiles]: consecutive phases alternate; two trials per search phase
  unsigned int* bar;       // barrier words (zeroed by the host before the launch)
  double* log;             // [n_steps][8] step log rows (ms_minimize's layout), written by workgroup 0
  double* result;          // [16]: steps done, reason, step size, energy, volume, min_edge^2, trials, barriers,
                           //       [8..13] where workgroup 0 spent its time (us, see k_resident)
  int n_steps, volrow, want_vol, atomic, max_iter;
  double step_size, tol, c1, beta, gamma, alpha_max_factor;
  int drift_check;
  double target_volume, volume_tolerance;
  int cap, max_ent;
};
enum : int {
  RES_DONE = 0,        // all requested steps taken
  RES_CONVERGED = 1,   // |g| < tol at the top of step `steps done` (no step taken there)
  RES_BAIL = 2,        // step `steps done` needs the ordinary path (guard range, non-descent, exhausted search)
  RES_DRIFT = 3,       // step `steps done - 1` was accepted and the volume drifted past the tolerance
  RES_TIMEOUT = 4      // a grid barrier timed out (never expected: the host re-runs from the last consistent x)
};
constexpr int RESIDENT_BAR_WORDS = 11 * 32;
size_t resident_lds_bytes(int cap, int max_ent, int max_tile_facets, bool atomic);
hipError_t resident_fits(int n_tiles, size_t lds, int device, int* resident);
hipError_t launch_resident(const ResidentArgs& a, size_t lds, hipStream_t s);

// kernel launchers (ms_kernels.hip).  cap = T + max halo (LDS patch slots),
// max_ent = largest per-tile vertex->corner entry count.
size_t energy_lds_bytes(int T, int cap, int max_ent, bool bend, bool guard, bool flags, bool atomic = false);
size_t gradient_lds_bytes(int T, int cap, int max_ent, bool bend, bool volrow, bool atomic = false, bool leaf = false);
// (*ran, when given: the instance that was launched or recorded)
hipError_t launch_energy(const EnergyArgs& a, bool guard, int cap, int max_ent, hipStream_t s, EnergyInst* ran = nullptr);
hipError_t launch_gradient(const GradientArgs& a, int cap, int max_ent, hipStream_t s);
// which instantiation the launchers pick; !valid() for arguments they refuse (hipErrorInvalidValue)
EnergyInst energy_instance(const EnergyArgs& a, bool guard);
GradientInst gradient_instance(const GradientArgs& a);
bool gradient_lean_instance(const GradientArgs& a);  // gradient_instance(a).lean
// mode 0: energy partial (MS_S_ETILT); 1: energy + gradients; 2: project tilts to tangent
size_t tilt_lds_bytes(int T, int cap, int max_ent, bool consistent = false, int mode = 1);
// (a launch with an absence mask stages one flag byte per patch row behind the kernel's own LDS)
inline size_t absent_lds_bytes(int cap) { return ((size_t)cap + 7) & ~(size_t)7; }
hipError_t launch_tilt(const TiltArgs& a, int mode, int cap, int max_ent, hipStream_t s);
// bending_tilt facet pass.  mode 0: energy (MS_S_EBT); 1: energy + back-prop factors;
// 2: energy + tilt gradient
size_t bt_lds_bytes(int T, int cap, int max_ent, int mode = 1);
hipError_t launch_bt(const BtArgs& a, int mode, int cap, int max_ent, hipStream_t s);
// tilt smoothness (Dirichlet) pass.  mode 0: energy (MS_S_ETS); 1: energy + tilt gradient; 2: Jacobi diagonal
size_t ts_lds_bytes(int T, int cap, int max_ent);
hipError_t launch_ts(const TsArgs& a, int mode, int cap, int max_ent, hipStream_t s);
hipError_t launch_tvec(int mode, int tile0, int tile1, int nv, int T, const uint8_t* vflags, double* tg,
                       const double* minv, double* dir, const double* tilts, const double* src,
                       const double* normals, double* out, double coef, int flag, double* partials,
                       int n_tiles, hipStream_t s, uint8_t fixed_bit = VF_TILT_FIXED,
                       int s_gn2 = MS_S_TGNORM2, int s_rz = MS_S_TRZ);
// Tilt search pass (ms_tsearch.inc): with the positions frozen, the energies of the tilt-reading modules of up to two
// fields at up to MS_MAX_TRIALS step sizes of ONE backtracking ladder in ONE facet pass -- the trial rows
// P(t + coef_j src) (k_tvec mode 2) are formed where they are staged, never written; trial j's per-tile partials go to
// partials[j] in the slots the single-trial kernels use (k_bt<0>, k_tsmooth<0>, k_tvec mode 4), by the same sums.
struct TsearchField {
  const double* tilts;     // (nvp,3) current tangent tilts
  const double* src;       // (nvp,3) search direction rows (the gradient or the CG direction)
  const double* bt_vert;   // (nvp,4) record of the energy pass at these positions (bending_tilt on)
  const double* kappa;     // (nvp) bending rigidity of this field
  const double* va;        // (nvp) barycentric vertex areas (tilt_form 2)
  double div_sign;         // -1 inner leaflet, +1 otherwise
  double k_tilt;           // tilt modulus
  double k_smooth;         // smoothness rigidity
  int tilt_form;           // 0: module off; 1: per-facet form (k_bt<0>'s fused term / k_tilt<0>); 2: vertex-area form
  int s_ebt, s_etilt, s_ets;  // reduction slots; s_ebt / s_ets < 0: module off
  int fixed_bit;           // vertex flag bit that clamps a row of this field
  double* trial_out;       // single-trial pass: the trial rows of the owned vertices are written here (or nullptr)
};
struct TsearchArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  const double* normals;   // (nvp,3) frozen unit vertex normals
  int n_fields, n_trials;
  // the same pass as the tilt-module energy evaluation of a SHAPE trial (one step size, plain): positions x + alpha d
  // (d != nullptr), the fields' rows taken as they are (already projected onto that surface), tilt_form 1
  const double* d;
  double alpha;
  int plain;
  TsearchField f[2];
  double coef[MS_MAX_TRIALS];       // sign * step_j
  double* partials[MS_MAX_TRIALS];  // partial set of trial j
};
size_t tsearch_lds_bytes(int cap, int n_fields, int n_trials);
hipError_t launch_tsearch(const TsearchArgs& a, int cap, hipStream_t s);

// Tilt gradient pass (ms_tsearch.inc): energies and tilt gradients of every tilt-reading module of up to two fields at the
// current tilts, positions frozen, then k_tvec mode 0 on the finished rows -- one launch per evaluation of a relaxation.
struct TgradField {
  const double* tilts;
  const double* bt_vert;
  const double* kappa;
  const double* va;        // tilt_form 2
  const double* minv;      // Jacobi M^-1 (the <r, M^-1 r> partial)
  double* grad;            // (nvp,3) out: dE/dt, clamped rows zero
  double div_sign, k_tilt, k_smooth;
  int tilt_form;           // 0 off; 1 per-facet energy, gradient k t_v A_v with the gathered barycentric area (k_tilt<1>); 2 vertex-area form (k_tvec mode 4)
  int s_ebt, s_etilt, s_ets, s_gn2, s_rz;
  int fixed_bit;
};
struct TgradArgs {
  DeviceMesh m;
  int tile0, tile1;
  const double* x;
  int n_fields;
  TgradField f[2];
  double* partials;
};
size_t tgrad_lds_bytes(int T, int cap, int max_ent, int n_fields, bool atomic, bool need_a3);
// combine: a corner's module terms are added and accumulated per vertex by LDS atomics (default mode); false: staged and gathered module by module, the per-module launches' sums
hipError_t launch_tgrad(const TgradArgs& a, int cap, int max_ent, bool combine, hipStream_t s);

// The LDS limits the host's size checks read (ms_create, the planners of the tilt passes, ms_tilt_lane_stats), in one
// place.  MS_LDS_CU: what one workgroup may ask for, the 160 KiB of a CU -- a launch above it is refused by the runtime.
// MS_LDS_TILT_PASS: the fused tilt passes (k_tsearch, k_tgrad, the fused relaxation) step aside above 150 KiB and the
// launch-per-module kernels, whose patches are smaller, run instead.
constexpr size_t MS_LDS_CU = (size_t)160 * 1024;
constexpr size_t MS_LDS_TILT_PASS = (size_t)150 * 1024;
// (what tsearch_plan, tilt_energy_pass and tgrad_plan decide by)
inline bool tsearch_fits(int cap, int n_fields, int n_trials) {
  return tsearch_lds_bytes(cap, n_fields, n_trials) <= MS_LDS_TILT_PASS;
}
inline bool tgrad_fits(int T, int cap, int max_ent, int n_fields) {
  return tgrad_lds_bytes(T, cap, max_ent, n_fields, false, true) <= MS_LDS_TILT_PASS;
}
// the leaflet bending_tilt instance of k_gradient (12 doubles per patch row, not 8): nothing at ms_create admits it
inline size_t leaflet_gradient_lds_bytes(int T, int cap, int max_ent, bool volrow, bool atomic) {
  return gradient_lds_bytes(T, cap, max_ent, true, volrow, atomic, true);
}

hipError_t launch_tvec2(const TvecArgs& a, const TvecArgs& b, int n_blocks, hipStream_t s);
// One fold launch.  set[]: the trials of a multi-trial launch in TRIAL order (the last one = the ordinary outputs); a
// plain fold has one set.
struct FoldSet {
  const double* partials;
  double* scal;
  unsigned long long* host_box;  // pinned mailbox {value, sequence} entries or nullptr
};
struct FoldArgs {
  int n_tiles, tile0, tile1;
  uint32_t slot_mask;
  unsigned long long ticket;
  int n_sets;
  FoldSet set[MS_MAX_TRIALS];
  const uint32_t* gate;   // fold only if *gate == gate_want (nullptr: always)
  uint32_t gate_want;
  int check_ran;          // the tile kernel feeding this fold was gated by the same word: its MS_P_RAN partials must add
                          // up to every tile (gate open) or to none (closed)
  uint32_t* dec_out;      // Armijo decision of this stage (nullptr: none)
  uint32_t* counter;      // arrival counter of the stage's energy workgroups (zero between launches)
  uint32_t e_mask;        // slots whose sum is a trial's energy (ESURF | EBEND as the module set has them)
  double rhs[MS_MAX_TRIALS];  // energy0 + c alpha_j <g,d>, trial order
  // Armijo right-hand sides formed on the device (nullptr: the host's rhs[] above): rhs_dev[j], written by the direction
  // fold that opened this round (go_out below)
  const double* rhs_dev;
  // MERGED fold (go_kind != 0): this launch also folds the direction scalars of the gradient pass that ran in front of
  // the energy launch (which did not wait for them), and the workgroup that arrives last first tests whether the search
  // the host queued the launch for happens at all -- go_kind 1: the direction with history is no descent direction
  // (<g,d> >= 0), the stepper restarts with d = -g; 2: the direction just written is a descent direction -- is not
  // converged (|g|^2 > go_tol2) and stays in the unguarded range (max|d_i|^2 < go_lim).  If not: DEC_STOP.  If so the
  // Armijo right-hand sides are formed here, rhs_j = go_e0 + (go_c alpha_j) <g,d>, alpha_j = alpha_{j-1} go_beta -- the
  // host's expressions with the host's roundings -- the trials are decided, and the right-hand sides of the ladder's
  // later alphas are left in go_out[2..] (doubles) for the gated stages behind this launch.
  int go_kind;
  double go_tol2, go_lim, go_e0, go_c, go_alpha0, go_beta;
  uint32_t* go_out;
  unsigned long long* host_err;  // pinned word: set non-zero when check_ran fails
  int side_full;          // fold every slot of the early trials' sets too (they have outputs of their own and can be
                          // accepted as they are); otherwise only their energy slots, by the head workgroup
};
hipError_t launch_reduce(const FoldArgs& a, hipStream_t s);

// the Armijo decision of a sharded trial from the scalar headers in this rank's slab (shard_decide, in the unpack kernel)
struct ShardDecideArgs {
  const double* recv;      // slab of this exchange: world x stride doubles, rank r's header at recv + r * stride
  size_t stride;
  int world;
  int has_alt, alt_off;    // pair launch: trial 0's slots sit alt_off further in the header
  int slot_a, slot_b;      // energy slots whose rank-ordered sums add up to the trial energy (-1: module off)
  double rhs_alt, rhs_main;
  uint32_t* dec_out;
  unsigned long long* post;  // pinned {value, value XOR ticket} pair for the host's replay (or nullptr)
  unsigned long long ticket;
};
hipError_t launch_pack_boundary(const int32_t* rows, int n_rows, const double* const* bufs,
                                const int* ncomp, int n_bufs, const double* scal, double* send,
                                hipStream_t s);
hipError_t launch_unpack_boundary(const int32_t* rows_all, const int32_t* row_off, int me, int world,
                                  int max_rows, double* const* bufs, const int* ncomp, int n_bufs,
                                  const double* recv, size_t stride, double* scal_all, hipStream_t s,
                                  unsigned long long* host_seq = nullptr, unsigned long long ticket = 0,
                                  bool remote_written = false, const unsigned long long* wait_flags = nullptr,
                                  unsigned long long wait_ticket = 0, unsigned long long* host_err = nullptr,
                                  const uint32_t* gate = nullptr, uint32_t gate_want = 0,
                                  // the trial decision this exchange feeds, taken by the header block that arrives last
                                  // (dec_arrived: a zeroed counter); nullptr: none
                                  const ShardDecideArgs* decide = nullptr, unsigned int* dec_arrived = nullptr);
hipError_t launch_post_seq(unsigned long long* host_seq, unsigned long long ticket, hipStream_t s);
// profiling only: *out = (*gate == want), one lane, queued right behind a gated launch (ms_profile_*)
hipError_t launch_gate_probe(const uint32_t* gate, uint32_t want, uint32_t* out, hipStream_t s);
// peer-to-peer exchange: pack straight into every peer's slab (dst[r] = that peer's slot for this rank), raise this
// rank's flag on every peer; the unpack kernel waits (bounded) for every peer's flag here
struct PeerFlags {
  unsigned long long* p[16];  // this exchange parity's flag rows of the peers (device table: ms_ctx::d_peer_flagtab)
};
// d_flags != nullptr: the last block to finish for a peer raises this rank's word there (no flag kernel); d_arrived: 16
// zeroed counters
hipError_t launch_pack_peers(const int32_t* rows, int n_rows, const double* const* bufs, const int* ncomp, int n_bufs,
                             const double* scal, double* const* dst, int world, hipStream_t s,
                             const PeerFlags* d_flags = nullptr, unsigned int* d_arrived = nullptr, int me = 0,
                             unsigned long long ticket = 0, const uint32_t* gate = nullptr, uint32_t gate_want = 0);
hipError_t launch_flag_peers(unsigned long long* const* peer_flags, int me, int world, unsigned long long ticket,
                             hipStream_t s);

hipError_t launch_axpy_rows(int64_t row0, int64_t row1, const int32_t* extra, int n_extra,
                            const uint8_t* vflags, double* x, const double* y, double coef,
                            hipStream_t s, const uint32_t* gate = nullptr, uint32_t gate_want = 0);
hipError_t launch_row_dot(int tile0, int tile1, int nv, int T, const double* g, const double* gC, double* partials,
                          int n_tiles, hipStream_t s);
hipError_t launch_direction(int tile0, int tile1, int nv, int T, const uint8_t* vflags, double* g,
                            const double* gC, double* d, const double* pg, const double* pd,
                            const double* scal, int use_constraint, int cg_history,
                            double* partials, int n_tiles, int write_g, hipStream_t s,
                            const uint32_t* gate = nullptr, uint32_t gate_want = 0, int pd_neg_pg = 0,
                            int precond = 0);
hipError_t launch_axpy_masked(int64_t n_rows, const uint8_t* vflags, double* x, const double* y,
                              double coef, hipStream_t s);
hipError_t launch_permute_in(int nv, const int32_t* perm, const double* src_ext, double* dst_int,
                             int ncomp, hipStream_t s);
hipError_t launch_permute_out(int nv, const int32_t* perm, const double* src_int, double* dst_ext,
                              int ncomp, hipStream_t s);
hipError_t launch_grad_cotan(int n, const double* u, const double* v, double* gu, double* gv,
                             hipStream_t s);
hipError_t launch_p1_divergence(int nv, int nf, const double* pos, const double* tilts,
                                const int32_t* tri, double* div, double* area, double* g0,
                                double* g1, double* g2, hipStream_t s);
hipError_t launch_laplacian_scatter(int dim, int nv, int nf, const double* weights,
                                    const int32_t* tri, const double* field, double* out,
                                    hipStream_t s);
hipError_t launch_curvature_raw(int nv, int nf, const double* pos, const int32_t* tri,
                                double* k_vecs, double* areas, double* weights, double* va0,
                                double* va1, double* va2, hipStream_t s);

}  // namespace ms
