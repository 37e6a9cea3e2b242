// The rules of csrc/ms_slot_writers.h, checked on the host: built with -fsanitize=address,undefined and run by
// tests/test_slot_writer_rules_host.py.  For every subset of the ten module bits of the table (three base modules,
// seven add-ons), both values of rsm_inner and all three phases, the table's answer for every writer is compared with
// the expressions the passes carried before the table existed, written out long-hand below.  Each carries the file
// and line it stood at in the commit before the table ("One module table behind the Minimizer's configuration and
// breakdown").  The derived masks and the run order are compared with that commit's literals.
#include <cstdint>
#include <cstdio>

#include "ms_slot_writers.h"

using namespace ms;

namespace {

constexpr uint32_t TILT_IN = MS_MOD_TILT_IN, TILT_OUT = MS_MOD_TILT_OUT, SMOOTH_IN = MS_MOD_TILT_SMOOTH_IN,
                   ST = MS_MOD_TILT_SPLAY_TWIST_IN, RS_IN = MS_MOD_TILT_RIM_SOURCE_IN, TB = MS_MOD_TILT_THETAB_CONTACT_IN,
                   RS_OUT = MS_MOD_TILT_RIM_SOURCE_OUT, RB = MS_MOD_TILT_RIM_SOURCE_BILAYER, CPL = MS_MOD_TILT_COUPLING,
                   RSM = MS_MOD_RIM_SLOPE_MATCH_OUT;
// the ten bits, and the add-ons in the one run order (ms_api_tilt.inc:74-112 is the order no buffer's writers leave)
constexpr uint32_t kBits[10] = {TILT_IN, TILT_OUT, SMOOTH_IN, ST, RS_IN, TB, RS_OUT, RB, CPL, RSM};
constexpr uint32_t kRunOrder[7] = {ST, RS_IN, TB, RS_OUT, RB, CPL, RSM};

const char* name(CellMode m) { return m == CellMode::DEFINE ? "DEFINE" : (m == CellMode::ADD ? "ADD" : "LEAVE"); }
const char* name(Phase p) { return p == Phase::ENERGY ? "ENERGY" : (p == Phase::TILT_EVAL ? "TILT_EVAL" : "GRADIENT"); }
int row_of(uint32_t bit) {
  for (int w = 0; w < kNumSlotWriters; ++w)
    if (kSlotWriters[w].bit == bit) return w;
  return -1;
}
// the kernels' fields as the passes set them: `define` 0 / 1, `cell_mode` 1 / 2, `define_in/out` -1 / 0 / 1
CellMode from_define(bool define) { return define ? CellMode::DEFINE : CellMode::ADD; }
CellMode from_cell_mode(int v) { return v == 2 ? CellMode::DEFINE : (v == 1 ? CellMode::ADD : CellMode::LEAVE); }
CellMode from_define3(int v) { return v == 1 ? CellMode::DEFINE : (v == 0 ? CellMode::ADD : CellMode::LEAVE); }

struct Want {
  CellMode mode = CellMode::LEAVE;       // of the writer's slot
  CellMode mode_disk = CellMode::LEAVE;  // of rim_slope_match_out's inner slot
  bool launch = false;
};

// what the parent did with writer `bit` in an evaluation of module set m
Want parent(uint32_t bit, uint32_t m, bool inner, Phase ph) {
  Want r;
  if (!(m & bit)) return r;
  if (ph != Phase::GRADIENT) {
    // phase_energy (ms_api_phases.inc:849-873) and tilt_eval (ms_api_tilt.inc:74-112) launch every module that is on
    r.launch = true;
    switch (bit) {
      case TILT_IN: case TILT_OUT: case SMOOTH_IN: r.mode = CellMode::DEFINE; break;  // k_tilt / k_tsmooth store their cells
      case RS_IN: r.mode = from_define(!(m & TILT_IN)); break;                     // ms_api_rim.inc:86 (f = tf[1])
      case RS_OUT: r.mode = from_define(!(m & TILT_OUT)); break;                   // ms_api_rim.inc:86 (f = tf[2])
      case TB: r.mode = from_define(!(m & (TILT_IN | RS_IN))); break;              // ms_api_thetab.inc:31
      case RB: r.mode = from_define(!(m & (TILT_OUT | RS_OUT))); break;            // ms_api_rim.inc:109-110
      case CPL: r.mode = from_cell_mode((m & (TILT_OUT | RS_OUT | RB)) ? 1 : 2); break;  // ms_api_couple.inc:37
      case RSM:
        r.mode = from_define3((m & (TILT_OUT | RS_OUT | RB | CPL)) ? 0 : 1);              // ms_api_rimmatch.inc:38
        r.mode_disk = from_define3(!inner ? -1 : ((m & (TILT_IN | RS_IN | TB)) ? 0 : 1));  // ms_api_rimmatch.inc:39
        break;
      case ST: r.mode = from_cell_mode((m & SMOOTH_IN) ? 1 : 2); break;  // ms_api_splay.inc:28
    }
    return r;
  }
  // behind a gradient pass (ms_api_phases.inc:1012-1055; every line below under `g_out`)
  switch (bit) {
    case TILT_IN: case TILT_OUT: r.launch = true; r.mode = CellMode::DEFINE; break;  // :1014-1015 k_tilt<1> rewrites the cells
    case SMOOTH_IN: break;  // :1056-1057 k_tsmooth has no shape gradient: not run
    case RS_IN: r.launch = (m & TILT_IN) != 0; if (r.launch) r.mode = from_define(false); break;   // :1014, :1020-1021; ms_api_rim.inc:86
    case RS_OUT: r.launch = (m & TILT_OUT) != 0; if (r.launch) r.mode = from_define(false); break;  // :1014, :1020-1021; ms_api_rim.inc:86
    case TB: r.launch = (m & TILT_IN) != 0; if (r.launch) r.mode = CellMode::ADD; break;    // :1014, :1025-1026 TB_CELL_ADD
    case RB: r.launch = (m & TILT_OUT) != 0; if (r.launch) r.mode = CellMode::ADD; break;   // :1014, :1030-1031 RB_CELL_ADD
    case CPL: r.launch = true; r.mode = (m & TILT_OUT) ? CellMode::ADD : CellMode::LEAVE; break;  // :1043-1045 CPL_CELL_ADD / _LEAVE
    case RSM:  // :1051-1052 RSM_CELL_ADD
      r.launch = true;
      r.mode = from_define3((m & TILT_OUT) ? 0 : -1);                // ms_api_rimmatch.inc:43
      r.mode_disk = from_define3((inner && (m & TILT_IN)) ? 0 : -1);  // ms_api_rimmatch.inc:44
      break;
    case ST: break;  // :1056-1057 never re-run: the cells are left
  }
  return r;
}

int fail(const char* what, uint32_t m, bool inner, Phase ph, uint32_t bit, const char* got, const char* want) {
  std::printf("FAIL %s: modules 0x%08x rsm_inner %d phase %s writer 0x%08x: table %s, parent %s\n", what, m, (int)inner,
              name(ph), bit, got, want);
  return 1;
}

}  // namespace

int main() {
  // the table itself: the ten bits once each, the add-ons in the run order
  if (kNumSlotWriters != 10) return std::printf("FAIL %d rows\n", kNumSlotWriters), 1;
  for (uint32_t b : kBits)
    if (row_of(b) < 0) return std::printf("FAIL no row for 0x%08x\n", b), 1;
  int n_addon = 0;
  for (const SlotWriter& w : kSlotWriters)
    if (!w.base && (n_addon >= 7 || w.bit != kRunOrder[n_addon++])) return std::printf("FAIL run order at 0x%08x\n", w.bit), 1;
  if (n_addon != 7) return std::printf("FAIL %d add-ons\n", n_addon), 1;
  // the add-on mask: ms_api_tilt.inc:818 (MS_LEAFLET_RS is ms_api_phases.inc:204)
  if (addon_mask() != (RS_IN | RS_OUT | RB | CPL | ST | TB | RSM)) return std::printf("FAIL addon_mask 0x%08x\n", addon_mask()), 1;
  for (int inner = 0; inner < 2; ++inner) {
    const uint32_t rsm_in = inner ? RSM : 0u;  // ms_api_rimmatch.inc:152 tf[1].mod_rsm
    // the union masks: etilt_all() of either field and ets_mods() of the inner one (ms_api_ctx.inc:153-159 over the bits
    // ms_api_context.inc:183-202 gives the fields)
    if (slot_writers(MS_S_ETILT_IN, inner) != (TILT_IN | RS_IN | TB | rsm_in)) return std::printf("FAIL writers of ETILT_IN\n"), 1;
    if (slot_writers(MS_S_ETILT_OUT, inner) != (TILT_OUT | RS_OUT | CPL | RB | RSM)) return std::printf("FAIL writers of ETILT_OUT\n"), 1;
    if (slot_writers(MS_S_ETS_IN, inner) != (SMOOTH_IN | ST)) return std::printf("FAIL writers of ETS_IN\n"), 1;
    // the add-ons among a field's mods() (ms_api_ctx.inc:153, ms_api_context.inc:189-202)
    if (addon_readers(1, inner) != (RS_IN | CPL | RB | ST | TB | rsm_in)) return std::printf("FAIL readers of the inner field\n"), 1;
    if (addon_readers(2, inner) != (RS_OUT | CPL | RB | RSM)) return std::printf("FAIL readers of the outer field\n"), 1;
  }
  long n = 0;
  const Phase phases[3] = {Phase::ENERGY, Phase::TILT_EVAL, Phase::GRADIENT};
  for (int inner = 0; inner < 2; ++inner)
    for (uint32_t sub = 0; sub < 1024u; ++sub)
      for (Phase ph : phases) {
        uint32_t m = 0;
        for (int k = 0; k < 10; ++k)
          if (sub & (1u << k)) m |= kBits[k];
        for (uint32_t bit : kBits) {
          const int w = row_of(bit);
          const SlotWriter& r = kSlotWriters[w];
          const Want want = parent(bit, m, inner != 0, ph);
          const CellMode got = cell_mode(w, r.slot, m, inner != 0, ph);
          if (got != want.mode) return fail("cell mode", m, inner != 0, ph, bit, name(got), name(want.mode));
          if (r.slot_disk >= 0) {
            const CellMode got2 = cell_mode(w, r.slot_disk, m, inner != 0, ph);
            if (got2 != want.mode_disk) return fail("cell mode (disk slot)", m, inner != 0, ph, bit, name(got2), name(want.mode_disk));
          }
          if (!r.base && launched(w, m, inner != 0, ph) != want.launch)
            return fail("launch", m, inner != 0, ph, bit, want.launch ? "no launch" : "launch", want.launch ? "launch" : "no launch");
        }
        ++n;
      }
  std::printf("%ld combinations ok\n", n);
  return n == 2L * 1024L * 3L ? 0 : 1;
}
