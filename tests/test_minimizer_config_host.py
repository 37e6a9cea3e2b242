"""The Minimizer's device configuration and energy breakdown against the record of the commit before the module table
(tests/golden/minimizer_config_log.json, written by tools/gen_golden_minimizer_config.py on that commit): the ordered
calls _device() makes on the device and the mirror for every trajectory fixture and for hand-built decks, on the first
call, on an unchanged second call and after a change inside and outside every table's key; the type and text of every
refusal; compute_energy_breakdown() over a device with distinct energies.  No GPU and no library."""

import json
import os

import pytest

import minimizer_config_cases as cases

with open(os.path.join(cases.GOLD, "minimizer_config_log.json")) as _fh:
    REC = json.load(_fh)
TRAJ = sorted(n for n in REC["config"] if n.startswith("traj_"))


def _json(v):
    return json.loads(json.dumps(v))


def test_the_record_covers_every_trajectory_fixture_and_every_case():
    assert len(TRAJ) == 38 and TRAJ == cases.traj_files()
    assert sorted(REC["config"]) == sorted(TRAJ + list(cases.HAND))
    assert sorted(REC["errors"]) == sorted(cases.ERRORS)
    assert set(REC["breakdown"]) >= set(TRAJ) | set(cases.BREAKDOWN_EXTRA)
    listed = {m for c in REC["config"].values() for m in c["modules"] + c["constraints"]}
    assert listed >= set(cases.mzmod._ENERGY_BITS) | {"volume", "body_area", "global_area", "pin_to_plane", "pin_to_circle",
                                                      "tilt_thetaB_boundary_in", "fixed_plane", "perimeter"}


@pytest.mark.parametrize("name", TRAJ)
def test_trajectory_fixture_configures_as_recorded(name):
    got = _json(cases.record_config(lambda: cases.traj_minimizer(name), cases.traj_changes))
    for g, w in zip(got["calls"], REC["config"][name]["calls"]):
        assert g == w, (name, w["after"])
    assert got == REC["config"][name]


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_built_deck_configures_as_recorded(name):
    got = _json(cases.record_config(*cases.HAND[name]))
    for g, w in zip(got["calls"], REC["config"][name]["calls"]):
        assert g == w, (name, w["after"])
    assert got == REC["config"][name]


@pytest.mark.parametrize("name", sorted(cases.ERRORS))
def test_refusal_keeps_its_type_and_text(name):
    build, device_free = cases.ERRORS[name]
    want, got = REC["errors"][name], cases.record_error(build)
    assert want["type"] is not None
    assert (got["type"], got["message"]) == (want["type"], want["message"])
    if device_free:  # (holds since the checks run before the mirror is synchronised)
        assert got["log"] == [], "refused after the device was touched"


@pytest.mark.parametrize("name", sorted(REC["breakdown"]))
def test_breakdown_is_the_recorded_one(name):
    if name in cases.BREAKDOWN_EXTRA:
        build = cases.BREAKDOWN_EXTRA[name]
    elif name in cases.HAND:
        build = cases.HAND[name][0]
    else:
        build = lambda: cases.traj_minimizer(name)  # noqa: E731
    assert cases.record_breakdown(build) == REC["breakdown"][name]
