// The leaflet modules that share a reduction slot, in one table.  Seven add-on modules have no slot of their own
// (MS_NSCAL is full): each adds its energy into the per-tile partial cells of a slot whose base module is another one.
// The rows are in run order: the base modules, then the add-ons in the ONE order every evaluation runs them.  From that
// order follows what a writer does to its slot's cells (cell_mode), whether it is launched behind a gradient pass
// (launched), and every mask the host code asks for.  Adding a module to a slot = one row here and its case in
// addon_passes (ms_api_phases.inc).  Host only, no HIP: a plain C++ compiler builds it.
#pragma once
#include <cstdint>

#include "membrane_hip.h"

namespace ms {

enum class CellMode { LEAVE, ADD, DEFINE };       // what a pass does to its slot's cells: nothing, += its sums, = its sums
enum class Phase { ENERGY, TILT_EVAL, GRADIENT };  // phase_energy, tilt_eval, the passes behind phase_gradient's

enum : uint8_t { RD_IN = 1, RD_OUT = 2 };  // SlotWriter::reads: the inner / the outer leaflet's field
struct SlotWriter {
  uint32_t bit;     // MS_MOD_*
  int slot;         // MS_S_*: the cells it writes
  int slot_disk;    // ... and these (and the inner field read) only while a disk ring is loaded (rsm_inner); -1: none
  uint8_t reads;    // RD_*: the leaflet fields it reads whatever is loaded
  bool base;        // the slot's own module; the others are add-ons
  bool shape_grad;  // has a shape gradient: a base module's k_tilt<1> rewrites the cells behind a gradient pass, an
                    // add-on is launched there for its rows of G even where it leaves the cells
};
constexpr SlotWriter kSlotWriters[] = {
    {MS_MOD_TILT_IN, MS_S_ETILT_IN, -1, RD_IN, true, true},
    {MS_MOD_TILT_OUT, MS_S_ETILT_OUT, -1, RD_OUT, true, true},
    {MS_MOD_TILT_SMOOTH_IN, MS_S_ETS_IN, -1, RD_IN, true, false},
    {MS_MOD_TILT_SPLAY_TWIST_IN, MS_S_ETS_IN, -1, RD_IN, false, false},
    {MS_MOD_TILT_RIM_SOURCE_IN, MS_S_ETILT_IN, -1, RD_IN, false, false},
    {MS_MOD_TILT_THETAB_CONTACT_IN, MS_S_ETILT_IN, -1, RD_IN, false, false},
    {MS_MOD_TILT_RIM_SOURCE_OUT, MS_S_ETILT_OUT, -1, RD_OUT, false, false},
    {MS_MOD_TILT_RIM_SOURCE_BILAYER, MS_S_ETILT_OUT, -1, RD_IN | RD_OUT, false, false},
    {MS_MOD_TILT_COUPLING, MS_S_ETILT_OUT, -1, RD_IN | RD_OUT, false, true},
    {MS_MOD_RIM_SLOPE_MATCH_OUT, MS_S_ETILT_OUT, MS_S_ETILT_IN, RD_OUT, false, true},
};
constexpr int kNumSlotWriters = (int)(sizeof(kSlotWriters) / sizeof(kSlotWriters[0]));

constexpr bool writes_slot(const SlotWriter& w, int slot, bool rsm_inner) {
  return w.slot == slot || (w.slot_disk == slot && rsm_inner);
}
constexpr uint32_t addon_mask() {  // every add-on bit
  uint32_t m = 0;
  for (const SlotWriter& w : kSlotWriters) m |= w.base ? 0u : w.bit;
  return m;
}
constexpr uint32_t slot_writers(int slot, bool rsm_inner) {  // the writers of a slot, its base module included
  uint32_t m = 0;
  for (const SlotWriter& w : kSlotWriters) m |= writes_slot(w, slot, rsm_inner) ? w.bit : 0u;
  return m;
}
constexpr uint32_t addon_readers(int leaflet, bool rsm_inner) {  // the add-ons that read a leaflet's field (1 inner, 2 outer)
  uint32_t m = 0;
  for (const SlotWriter& w : kSlotWriters)
    if (!w.base && ((w.reads & (leaflet == 1 ? RD_IN : RD_OUT)) || (leaflet == 1 && w.slot_disk >= 0 && rsm_inner))) m |= w.bit;
  return m;
}

// What writer w does to the cells of `slot` in an evaluation of `modules`.
//   In an evaluation the first writer of the slot that is on DEFINES the cells, every later one ADDS.
//   Behind a gradient pass the cells hold the evaluation's sums unless the base module's k_tilt<1> has rewritten them:
//   then every add-on ADDS once more, otherwise the cells are LEFT.
constexpr CellMode cell_mode(int w, int slot, uint32_t modules, bool rsm_inner, Phase phase) {
  const SlotWriter& me = kSlotWriters[w];
  if (!(modules & me.bit) || !writes_slot(me, slot, rsm_inner)) return CellMode::LEAVE;
  if (phase == Phase::GRADIENT) {
    for (const SlotWriter& b : kSlotWriters)
      if (b.base && b.slot == slot && b.shape_grad && (modules & b.bit)) return me.base ? CellMode::DEFINE : CellMode::ADD;
    return CellMode::LEAVE;
  }
  for (int k = 0; k < w; ++k)
    if ((modules & kSlotWriters[k].bit) && writes_slot(kSlotWriters[k], slot, rsm_inner)) return CellMode::ADD;
  return CellMode::DEFINE;
}

// Is add-on w launched?  In an evaluation whenever it is on; behind a gradient pass only for its shape gradient or to
// add into cells that were rewritten (a writer that would leave every cell and has no rows of G is not launched).
constexpr bool launched(int w, uint32_t modules, bool rsm_inner, Phase phase) {
  const SlotWriter& me = kSlotWriters[w];
  if (!(modules & me.bit)) return false;
  if (phase != Phase::GRADIENT || me.shape_grad) return true;
  return cell_mode(w, me.slot, modules, rsm_inner, phase) == CellMode::ADD ||
         (me.slot_disk >= 0 && cell_mode(w, me.slot_disk, modules, rsm_inner, phase) == CellMode::ADD);
}

}  // namespace ms
