"""leaflet_out_absent_presets on the host: the mask, the kept-facet set and the topology validation of
leaflet_common against the reference's (tools/gen_golden_leaflet_absent.py -> tests/golden/leaflet_absent_cases.npz), the
masked NumPy forms of tilt_out and tilt_smoothness_out, the masked vertex areas of a relaxation, and what stays refused.
No GPU."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

G = load_golden("leaflet_absent_cases.npz")
NAMES = [str(n) for n in G["names"]]


def _case(name):
    from membrane_solver_amd.geometry.mesh import ArrayMesh

    mname = str(G[name + "__mesh"])
    P, T = G["mesh__" + mname + "__positions"], G["mesh__" + mname + "__tri"]
    gp = json.loads(str(G[name + "__gp"]))
    vo = {int(k): v for k, v in json.loads(str(G[name + "__vopts"])).items()}
    mesh = ArrayMesh(P, T, global_parameters=gp, tilts_in=G[name + "__tilts_in"], tilts_out=G[name + "__tilts_out"],
                     vertex_options=vo, tilt_fixed_out=G[name + "__tilt_fixed_out"])
    return mesh, P, T, gp, vo


class _RefVertex:
    def __init__(self, options):
        self.options = options


class _RefMesh:
    """The few attributes of a reference Mesh the option readers look at: ``vertices`` {id: .options}, ids that are not
    the rows."""

    def __init__(self, P, T, vo):
        self.vertex_ids = np.arange(len(P)) + 100
        self.vertices = {int(v): _RefVertex(vo.get(i) or {}) for i, v in enumerate(self.vertex_ids)}
        self.vertex_index_to_row = {int(v): i for i, v in enumerate(self.vertex_ids)}
        self._tri = np.asarray(T)

    def triangle_row_cache(self):
        return self._tri, np.arange(len(self._tri))


@pytest.mark.parametrize("name", NAMES)
def test_mask_and_kept_facets_match_reference(name):
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    mesh, P, T, gp, vo = _case(name)
    absent = lc.absent_mask(mesh, mesh.global_parameters, "out")
    assert absent.dtype == bool and absent.shape == (len(P),)
    assert np.array_equal(absent, G[name + "__absent"])
    assert np.array_equal(lc.kept_facets(T, absent), G[name + "__kept"])
    assert not lc.absent_mask(mesh, mesh.global_parameters, "in").any()
    assert not lc.absent_mask(mesh, mesh.global_parameters, "sideways").any()
    # the same rows from a reference-style Mesh (options on the vertices, ids that are not rows)
    ref = _RefMesh(P, T, vo)
    assert np.array_equal(lc.absent_mask(ref, mesh.global_parameters, "out"), G[name + "__absent"])


def test_preset_list_is_normalised_as_the_reference_does():
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    assert lc.normalize_preset_list(None) == []
    assert lc.normalize_preset_list(" disk ") == ["disk"]
    assert lc.normalize_preset_list("  ") == []
    assert lc.normalize_preset_list(["disk", None, " rim ", "", 3]) == ["disk", "rim", "3"]
    assert lc.normalize_preset_list(("a",)) == ["a"]
    assert sorted(lc.normalize_preset_list({"a", "b"})) == ["a", "b"]
    assert lc.normalize_preset_list(7) == [] and lc.normalize_preset_list({"disk": 1}) == []
    mesh, P, _T, _gp, _vo = _case("disk4_ring1_lumped")
    for raw in ("disk", ["disk"], (" disk ",), {"disk"}, ["other", "disk"]):
        assert np.array_equal(lc.absent_mask(mesh, {"leaflet_out_absent_presets": raw}, "out"), G["disk4_ring1_lumped__absent"])
    for raw in (None, "", [], ["rim"], 5):
        assert not lc.absent_mask(mesh, {"leaflet_out_absent_presets": raw}, "out").any()


@pytest.mark.parametrize("name", NAMES)
def test_validation_strict_raises_and_triangles_passes(name):
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    mesh, _P, _T, gp, _vo = _case(name)
    straddles = bool(G[name + "__straddles"])
    for mode in ("triangles", "facet", "Facets ", "triangle"):
        lc.validate_absence_topology(mesh, dict(gp, leaflet_out_absence_mode=mode))
    for strict in (dict(gp, leaflet_out_absence_mode="strict"), {k: v for k, v in gp.items() if k != "leaflet_out_absence_mode"}):
        if straddles:
            with pytest.raises(ValueError, match="Leaflet absence topology invalid.*straddle absent/present"):
                lc.validate_absence_topology(mesh, strict)
        else:
            lc.validate_absence_topology(mesh, strict)
    assert straddles == (str(G[name + "__what"]) not in ("all", "none"))


@pytest.mark.parametrize("name", NAMES)
def test_masked_numpy_forms_match_reference(name):
    """tilt_out and tilt_smoothness_out over the kept facets: energy to 1e-12 relative, gradients to 1e-11 of their
    largest entry; the inner modules with the same functions and no mask."""
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    mesh, P, T, gp, _vo = _case(name)
    absent = lc.absent_mask(mesh, mesh.global_parameters, "out")
    tin, tout = G[name + "__tilts_in"], G[name + "__tilts_out"]
    out = lc.tilt_leaflet_numpy(P, T, tout, k_tilt=gp["tilt_modulus_out"], mass_mode=gp["tilt_mass_mode_out"], absent=absent)
    sm = lc.tilt_smoothness_numpy(P, T, tout, k_smooth=gp["bending_modulus_out"], absent=absent)
    inn = lc.tilt_leaflet_numpy(P, T, tin, k_tilt=gp["tilt_modulus_in"], mass_mode=gp["tilt_mass_mode_in"])
    smi = lc.tilt_smoothness_numpy(P, T, tin, k_smooth=gp["bending_modulus_in"])
    for got, key in ((out["E"], "E_tilt_out"), (sm["E"], "E_smooth_out"), (inn["E"], "E_tilt_in"), (smi["E"], "E_smooth_in")):
        want = float(G[f"{name}__{key}"])
        print(name, key, got, want)
        assert abs(got - want) <= 1e-12 * abs(want)
    for got, key in ((out["grad"], "grad_tilt_out"), (out["tilt_grad"], "tilt_grad_tilt_out"),
                     (sm["tilt_grad"], "tilt_grad_smooth_out"), (inn["grad"], "grad_tilt_in"),
                     (inn["tilt_grad"], "tilt_grad_tilt_in"), (smi["tilt_grad"], "tilt_grad_smooth_in")):
        want = G[f"{name}__{key}"]
        if not want.any():
            assert not got.any(), key
        else:
            print(name, key, relerr(got, want))
            assert relerr(got, want) <= 1e-11, key
    if str(G[name + "__what"]) == "all":
        assert out["E"] == 0.0 and sm["E"] == 0.0
    # the relaxation's outer vertex areas (the kept facets' thirds) and the inner ones
    va = lc.masked_vertex_areas(P, T, absent)
    assert np.max(np.abs(va - G[name + "__va_out"])) <= 1e-13 * max(np.max(G[name + "__va_in"]), 1e-300)
    assert np.max(np.abs(lc.masked_vertex_areas(P, T) - G[name + "__va_in"])) <= 1e-13 * np.max(G[name + "__va_in"])
    assert not va[absent].any()


def test_refusals():
    """What stays outside the device path, each with "outside the HIP hot path" in its message; none of them reaches
    the device (no GPU here)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    mesh, P, T, gp, vo = _case("disk4_ring1_lumped")
    # accepted: a selecting list (returns the rows), no list, an empty list
    assert np.array_equal(lc.absent_out_rows(mesh, gp), G["disk4_ring1_lumped__absent"])
    lc.check_supported(gp, mesh)
    assert lc.absent_out_rows(mesh, {}) is None and lc.absent_out_rows(mesh, {"leaflet_out_absent_presets": []}) is None
    # a preset list that selects no row: an option-less mesh, a preset no vertex carries, no mesh at all
    bare = ArrayMesh(P, T, global_parameters=dict(gp))
    for m, g in ((bare, gp), (mesh, dict(gp, leaflet_out_absent_presets=["rim"])), (None, gp)):
        with pytest.raises(L.MembraneHipError, match="selects no row.*outside the HIP hot path"):
            lc.check_supported(g, m)
    # leaflet_in_absent_presets, whether or not it selects a row
    for raw in (["disk"], "nothing"):
        with pytest.raises(L.MembraneHipError, match="leaflet_in_absent_presets.*outside the HIP hot path"):
            lc.check_supported(dict(gp, leaflet_in_absent_presets=raw), mesh)
    # the physical-edge staggered rim mode next to a mask (its restored trace rows are not built)
    with pytest.raises(L.MembraneHipError, match="physical_edge_staggered_v1.*outside the HIP hot path"):
        lc.check_supported(dict(gp, rim_slope_match_mode="physical_edge_staggered_v1"), mesh)
    lc.check_supported(dict(gp, rim_slope_match_mode="physical_edge_staggered_v1", leaflet_out_absent_presets=[]), mesh)
    # every other key of the list is refused as before, with and without a mask
    for key in lc._UNSUPPORTED_KEYS:
        if key in lc._ABSENT_KEYS:
            continue
        for base in (gp, {}):
            with pytest.raises(L.MembraneHipError, match=key + ".*outside the HIP hot path"):
                lc.check_supported(dict(base, **{key: "on"}), mesh)
    # the module's own entry point refuses the same way
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    em = EnergyModuleManager(["bending_tilt_out", "tilt_out"])
    kw = dict(positions=P, grad_arr=None, tilts_in=None, tilts_out=None)
    with pytest.raises(L.MembraneHipError, match="selects no row.*outside the HIP hot path"):
        em.get_module("tilt_out").compute_energy_and_gradient_array(
            bare, bare.global_parameters, ParameterResolver(bare.global_parameters), index_map=bare.vertex_index_to_row, **kw)
    # bending_tilt_out next to a mask: refused, and the message names the follow-up
    with pytest.raises(L.MembraneHipError, match="bending_tilt_out next to a non-empty.*outside the HIP hot path.*follow-up"):
        em.get_module("bending_tilt_out").compute_energy_and_gradient_array(
            mesh, mesh.global_parameters, ParameterResolver(mesh.global_parameters), index_map=mesh.vertex_index_to_row, **kw)


def test_flag_update_goes_through_the_permutation_and_keeps_the_other_bits():
    """ms_leaflet_absent_flags_host: the loop ms_set_leaflet_absent runs (library row i reads absent[perm[i]])."""
    import ctypes

    from membrane_solver_amd import _lib as L

    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    rng = np.random.default_rng(4)
    nv = 37
    perm = rng.permutation(nv).astype(np.int32)
    absent = (rng.random(nv) < 0.3).astype(np.uint8)
    before = rng.integers(0, 32, nv).astype(np.uint8)  # (the five flag bits below the absence bit)
    flags = before.copy()
    state = ctypes.c_int(-1)
    fn = L.lib().ms_leaflet_absent_flags_host  # (csrc/ms_test_hooks.h: exported for tests, no part of the public header)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, L._I32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                   ctypes.POINTER(ctypes.c_int)]
    L.check(fn(nv, perm.ctypes.data_as(L._I32), u8(absent), u8(flags), ctypes.byref(state)), None, "flags")
    assert state.value == 3
    assert np.array_equal(flags & 31, before) and np.array_equal((flags & 32) != 0, absent[perm] != 0)
    L.check(fn(nv, perm.ctypes.data_as(L._I32), None, u8(flags), ctypes.byref(state)), None, "flags")
    assert state.value == 1 and np.array_equal(flags, before)
    L.check(fn(nv, perm.ctypes.data_as(L._I32), None, u8(flags), ctypes.byref(state)), None, "flags")
    assert state.value == 0 and np.array_equal(flags, before)
    perm[5] = nv
    with pytest.raises(L.MembraneHipError, match="permutation out of range"):
        L.check(fn(nv, perm.ctypes.data_as(L._I32), u8(absent), u8(flags), ctypes.byref(state)), None, "flags")
