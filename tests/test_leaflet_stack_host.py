"""The leaflet-stack fixtures (tools/gen_golden_leaflet_stack.py) on the host: every file small enough to commit, every
active add-on of every case visible in the case's energy or tilt gradients, the breakdown consistent with the total, every
trajectory holding what it is named for, and the reference's own noise far enough below what the device tests have to
resolve.  No GPU, and nothing of the reference is read: only the committed fixtures."""

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

CASES_FILE, RELAX_FILE = "leaflet_stack_cases.npz", "leaflet_stack_relax.npz"
TRAJ = {"traj_disk6_gd_stack_nested.npz": "gd", "traj_disk6_cg_stack_coupled_backtrack.npz": "cg",
        "traj_disk6_cg_stack_pins.npz": "cg"}
CASES = load_golden(CASES_FILE)
NAMES = [str(n) for n in CASES["names"]]
ADDONS = [str(n) for n in CASES["addons"]]
CONSTRAINT = "tilt_thetaB_boundary_in"
CHAINS = {"I": ["tilt_in", "tilt_rim_source_in", "tilt_thetaB_contact_in"],
          "O": ["tilt_out", "tilt_rim_source_out", "tilt_rim_source_bilayer", "tilt_coupling"],
          "S": ["tilt_smoothness_in", "tilt_splay_twist_in"]}
REST = ["surface", "bending_tilt_in", "bending_tilt_out", "tilt_smoothness_out"]


def case(name):
    g = CASES
    mods = [str(m) for m in g[name + "__modules"]]
    return {"modules": mods, "empty": [str(m) for m in g[name + "__empty"]], "gp": json.loads(str(g[name + "__gp"])),
            "E": float(g[name + "__E"]), "E_scale": float(g[name + "__E_scale"]),
            "breakdown": dict(zip(mods, g[name + "__breakdown"].tolist())), "E_tilt": float(g[name + "__E_tilt"]),
            "grad": g[name + "__grad"], "gi": g[name + "__tilt_grad_in"], "go": g[name + "__tilt_grad_out"],
            "sens_names": [str(m) for m in g[name + "__sens_names"]], "sens_E": g[name + "__sens_E"],
            "sens_G": g[name + "__sens_G"]}


def bar(g, key):
    """what a device test may allow: ten times what a 1e-13 perturbation of the start does to the reference's own run"""
    return max(1e-12, 10.0 * float(g[key]))


@pytest.mark.parametrize("fname", [CASES_FILE, RELAX_FILE] + sorted(TRAJ))
def test_fixture_is_small_enough_to_commit(fname):
    assert os.path.getsize(os.path.join(GOLDEN, fname)) < 1 << 20


def test_the_case_list_is_the_one_the_chains_give():
    """Every non-empty subset of one chain next to the two others in full (the full stack stored once), the add-ons
    alone and the three empty tables."""
    import itertools

    want = set()
    for tag, chain in CHAINS.items():
        others = [m for t, c in CHAINS.items() if t != tag for m in c]
        for k in range(1, len(chain) + 1):
            for sub in itertools.combinations(chain, k):
                want.add(frozenset(REST + others + list(sub)))
    assert len(want) == 7 + 15 + 3 - 2
    got = {frozenset(case(n)["modules"]) for n in NAMES if not case(n)["empty"] and n != "addons_only"}
    assert got == want
    assert set(case("addons_only")["modules"]) == set(ADDONS) and len(ADDONS) == 6
    assert len(NAMES) == len(want) + 1 + 3
    c = case("empty_rsi_then_tbc")
    assert c["empty"] == ["tilt_rim_source_in"] and "tilt_thetaB_contact_in" in c["modules"] and "tilt_in" not in c["modules"]
    c = case("empty_rso_then_rb_cpl")
    assert c["empty"] == ["tilt_rim_source_out"] and "tilt_out" not in c["modules"]
    assert {"tilt_rim_source_bilayer", "tilt_coupling"} <= set(c["modules"])
    c = case("empty_rb_then_cpl")
    assert c["empty"] == ["tilt_rim_source_bilayer"] and "tilt_coupling" in c["modules"]
    assert not {"tilt_out", "tilt_rim_source_out"} & set(c["modules"])


@pytest.mark.parametrize("name", NAMES)
def test_every_active_addon_shows(name):
    """Dropping any active add-on moves E by >= 1e-4 E_scale or a tilt-gradient entry by >= 1e-4 of the largest: seven
    orders above the bars of the device tests.  An add-on with an empty table is listed, exempt, and exactly zero."""
    c = case(name)
    active = [m for m in c["modules"] if m in ADDONS and m not in c["empty"]]
    assert c["sens_names"] == active and len(c["sens_E"]) == len(c["sens_G"]) == len(active)
    for m, dE, dG in zip(active, c["sens_E"], c["sens_G"]):
        assert max(dE, dG) >= 1e-4, (name, m, dE, dG)
    for m in c["empty"]:
        assert c["breakdown"][m] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_breakdown_sums_to_the_total(name):
    c = case(name)
    g = CASES
    assert c["E_scale"] > 0.0
    assert abs(sum(c["breakdown"].values()) - c["E"]) <= 1e-13 * c["E_scale"]
    tilt_sum = sum(v for m, v in c["breakdown"].items() if m != "surface")
    assert abs(c["E_tilt"] - tilt_sum) <= 1e-13 * c["E_scale"]
    scale = 0.0
    for m in c["modules"]:
        if m in c["empty"]:
            continue
        assert abs(c["breakdown"][m] - float(g["alone__" + m + "__E"])) <= 1e-13 * c["E_scale"]
        assert abs(float(g["alone__" + m + "__E"])) <= float(g["alone__" + m + "__scale"]) * (1.0 + 1e-13)
        scale += float(g["alone__" + m + "__scale"])
    assert abs(scale - c["E_scale"]) <= 1e-15 * scale
    for key in ("grad", "gi", "go"):
        assert c[key].shape == g["positions"].shape and np.all(np.isfinite(c[key]))
    assert not c["grad"][g["fixed"]].any()  # (the boundary rows are fixed)


def test_relaxation_fixture():
    g = load_golden(RELAX_FILE)
    mods = [str(m) for m in g["modules"]]
    assert len(g["positions"]) == 84 and [str(c) for c in g["constraint_modules"]] == [CONSTRAINT]
    assert "surface" not in mods and set(ADDONS) <= set(mods) and len(mods) == 12
    gp = json.loads(str(g["gp_json"]))
    assert gp["tilt_solve_mode"] == "nested" and gp["tilt_solver"] == "cg" and gp["tilt_cg_preconditioner"] == "jacobi"
    assert int(g["n_gradient_evaluations"]) > 0 and int(g["n_energy_evaluations"]) > 0 and int(g["accepted_steps"]) > 0
    assert abs(float(np.sum(g["breakdown"])) - float(g["E_total"])) <= 1e-12 * float(np.sum(np.abs(g["breakdown"])))
    assert np.all(g["breakdown"][[mods.index(m) for m in ADDONS]] != 0.0)
    assert np.max(np.abs(g["tilts_in_final"] - g["tilts_in0"])) > 1e-4
    assert bar(g, "noise_tilts") < 1e-8 and bar(g, "noise_energy") < 1e-8


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_trajectory_has_the_property_it_is_named_for(fname):
    g = load_golden(fname)
    L = g["step_log"]
    mods, cons = [str(m) for m in g["modules"]], [str(c) for c in g["constraint_modules"]]
    gp = json.loads(str(g["gp_json"]))
    assert (L[:, 0] > 0).sum() >= 3 and g["stepper"] == {"gd": "GradientDescent", "cg": "ConjugateGradient"}[TRAJ[fname]]
    full = set(REST) | {m for c in CHAINS.values() for m in c}
    if "nested" in fname:
        assert set(mods) == full and cons == [CONSTRAINT]
        assert gp["tilt_solve_mode"] == "nested" and gp["tilt_solver"] == "cg"
    if "backtrack" in fname:
        # a search that took the energy at x and at two trials or more and accepted: a trial before it was rejected
        assert set(mods) == full and gp["tilt_solve_mode"] == "coupled" and gp["tilt_solver"] == "gd"
        assert np.any((L[:, 0] > 0) & (g["line_search_evals"] >= 3))
    if "pins" in fname:
        assert set(mods) == full - {"tilt_splay_twist_in"} and cons == ["pin_to_circle", CONSTRAINT]
        vo = json.loads(str(g["vopts"]))
        pinned = [k for k, v in vo.items() if "pin_to_circle" in v.get("constraints", [])]
        assert len(pinned) == 18 and all(vo[k]["pin_to_circle_mode"] == "slide" for k in pinned)
        assert float(g["E_own_final"]) != 0.0
    for key in ("noise_energy", "noise_positions", "noise_tilts"):
        assert bar(g, key) < 1e-8, (fname, key, float(g[key]))
