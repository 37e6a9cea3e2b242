"""What the per-module host tests read of the slot-writer table (csrc/ms_slot_writers.h) and of the host code that
derives its lists from it.  The table's rules themselves are checked by tests/slot_writer_rules.cpp against the
expressions the passes carried before the table; here a module's test asks for its row, its place in the run order,
and that the lanes which cannot carry an add-on decline the table's whole add-on mask."""

import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "membrane_solver_amd", "csrc")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def rows():
    """The table's rows in order: dicts of bit, slot, slot_disk (None: none), reads (set of RD_*), base, shape_grad."""
    src = _read("ms_slot_writers.h")
    body = src[src.index("constexpr SlotWriter kSlotWriters[] = {"):]
    body = body[:body.index("};")]
    out = []
    for m in re.finditer(r"\{(MS_MOD_\w+), (MS_S_\w+), (-1|MS_S_\w+), ([A-Z_| ]+), (true|false), (true|false)\}", body):
        out.append({"bit": m.group(1), "slot": m.group(2), "slot_disk": None if m.group(3) == "-1" else m.group(3),
                    "reads": {r.strip() for r in m.group(4).split("|")}, "base": m.group(5) == "true",
                    "shape_grad": m.group(6) == "true"})
    assert len(out) == body.count("{MS_MOD_") == 10
    return out


def row(bit):
    hits = [r for r in rows() if r["bit"] == bit]
    assert len(hits) == 1, bit
    return hits[0]


def writers_in_front(bit, slot):
    """The writers of `slot` the table runs ahead of `bit` (the slot's base module first)."""
    names = [r["bit"] for r in rows() if slot in (r["slot"], r["slot_disk"])]
    return names[:names.index(bit)]


def assert_lanes_decline_every_addon(bit):
    """The search / gradient pass of a relaxation, the one-tile relaxation program (and with it the fused evaluator,
    which only that program starts) and the slot readers take `bit` from the table's add-on mask."""
    assert not row(bit)["base"]
    tilt, phases, ctx = _read("ms_api_tilt.inc"), _read("ms_api_phases.inc"), _read("ms_api_ctx.inc")
    assert re.search(r"constexpr uint32_t MS_LEAFLET_ADDONS = addon_mask\(\);", phases)
    plan = tilt[tilt.index("bool tsearch_plan("):tilt.index("bool tgrad_plan(")]
    assert re.search(r"if \(mods & MS_LEAFLET_ADDONS\) return false;", plan)  # tsearch_plan (and tgrad_plan through it)
    # the relaxation program: one call site, under the gate; the fused evaluator is reached through it alone
    assert len(re.findall(r"\brelax_program\(", tilt)) == 2
    gate = re.search(r"exec_relax && !\(mods & MS_LEAFLET_ADDONS\)\) \{", tilt)
    assert gate and 0 < tilt.index("rc = relax_program(", gate.end()) - gate.end() < 200
    assert tilt.count("CK_RELAX_FUSED") == 1
    assert tilt.index("\nint relax_program(") < tilt.index("CK_RELAX_FUSED") < tilt.index("\nint relax_fields(")
    m = re.search(r"constexpr uint32_t MS_LEAFLET_MODS = ([^;]*);", phases)
    assert m and "MS_LEAFLET_ADDONS" in m.group(1)  # (the resident step declines every tilt module)
    # every field that reads the module counts it: TiltField::mods() through the table's readers
    assert re.search(r"uint32_t mods\(\) const \{[^}]*mod_addons[^}]*\}", ctx)
    assert len(re.findall(r"mod_addons = addon_readers\(", _read("ms_api_context.inc"))) == 2
