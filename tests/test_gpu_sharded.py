"""Sharded HIP backend on ONE GPU: 2-3 shard contexts (tile ranges) driven by threads whose
collectives are an in-process stand-in for RCCL.  This runs the real tile-range kernels,
ms_rebind_state, the phase API, the boundary pack/unpack kernels and the in-place shard commit;
only the RCCL transport itself is replaced.  Before every exchange each rank NaN-poisons all the
rows it does not own, so a halo row missing from the boundary lists cannot go unnoticed.  The
sharded run must match the single-context ms_step run."""

import os
import threading

import numpy as np
import pytest

from conftest import relerr
from shard_cases import (BY_ID, NEW_CASES, OPEN_IDS, TILT_BITS, clamped_steps, configure_kwargs, lane_report,
                         legacy_case, materialize, run_port)

pytestmark = pytest.mark.gpu


class ThreadGroup:
    """all_gather_into_tensor for `world` threads of one process (device tensors), ordered the way RCCL orders it:
    against each rank's CURRENT stream only (events), never by a device-wide synchronize -- so a pack or unpack
    kernel running on some other stream than the one the collective is ordered against shows up as a wrong row."""

    def __init__(self, world):
        import torch

        self.torch, self.world = torch, world
        self.slots = [None] * world
        self.done = [None] * world
        self.bar = threading.Barrier(world)
        self.local = threading.local()
        self.sizes = [[] for _ in range(world)]  # doubles per message of every all-gather, per rank

    def bind(self, rank):
        self.local.rank = rank

    def all_gather_into_tensor(self, out, inp):
        torch = self.torch
        r = self.local.rank
        cur = torch.cuda.current_stream()
        self.sizes[r].append(int(inp.numel()))
        ready = torch.cuda.Event()
        ready.record(cur)  # `inp` is complete once this rank's stream reaches here
        self.slots[r] = (inp, ready)
        self.bar.wait()
        n = inp.shape[0]
        for k in range(self.world):
            src, ev = self.slots[k]
            cur.wait_event(ev)
            out[k * n:(k + 1) * n].copy_(src)
        done = torch.cuda.Event()
        done.record(cur)
        self.done[r] = done
        self.bar.wait()
        for k in range(self.world):
            # nobody reuses its send buffer before every peer has copied it: a HOST wait, because the library driver's
            # callback refills the buffer with a null-stream hipMemcpy that no torch stream orders
            self.done[k].synchronize()
        self.bar.wait()

    def share(self, rank, item):
        """Every rank contributes one Python object; all get the rank-ordered list (one address space)."""
        if not hasattr(self, "shared"):
            self.shared = [None] * self.world
        self.shared[rank] = item
        self.bar.wait()
        out = list(self.shared)
        self.bar.wait()
        return out

    def all_reduce(self, t):
        """SUM over the ranks in rank order (the dense exchange mode): every rank reads every peer's tensor, and
        overwrites its own only after all of them have finished reading."""
        torch = self.torch
        r = self.local.rank
        cur = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(cur)
        self.slots[r] = (t, ready)
        self.bar.wait()
        acc = torch.zeros_like(t)
        for k in range(self.world):
            src, ev = self.slots[k]
            cur.wait_event(ev)
            acc += src
        done = torch.cuda.Event()
        done.record(cur)
        self.done[r] = done
        self.bar.wait()
        for k in range(self.world):
            self.done[k].synchronize()
        self.bar.wait()
        t.copy_(acc)
        cur.synchronize()
        self.bar.wait()


@pytest.mark.parametrize("driver,pair", [("python", "0"), ("library", "0"), ("library", "2"), ("python-dense", "0"),
                                         ("library-peer", "0"), ("library-peer", "2")])
@pytest.mark.parametrize("with_volume,world,level,freq,tile", [
    (False, 2, 2, 16, 64), (True, 2, 2, 16, 64), (False, 3, 2, 16, 64), (False, 2, 0, 16, 64), (True, 3, 0, 16, 64),
    (False, 4, 2, 160, 256),  # 512 000 facets, default tile size, 4 shards: sizes near the headline
    (True, 3, 2, 40, 200),  # tiles of 200 rows on the 256-thread instances: the shards' row ranges follow the rows
])
def test_shards_match_single_context(with_volume, world, level, freq, tile, driver, pair, monkeypatch):
    """driver "python": parallel.ShardedStepper drives the phase API; "library": the same control
    flow inside the library (ms_shard_step) with the in-process all-gather plugged in where
    ncclAllGather goes.  pair "2": every search that can starts with a pair launch (trials 0 and 1 in one energy
    launch and ONE exchange; MS_PAIR) -- same trajectory, fewer exchanges."""
    _run_shard_case(legacy_case(with_volume, world, level, freq, tile), driver, pair, monkeypatch)


def test_config4_full_size_eight_shards(monkeypatch):
    """BASELINE configs[3] at its own size: the 2 048 000-facet icosphere cut into 8 facet-block shards (8 contexts on
    this one GPU, the library driver with the in-process all-gather where ncclAllGather goes), six CG steps with
    fixed-order vertex sums, against the single-context run step for step."""
    _run_shard_case(legacy_case(False, 8, 2, 320, 256), "library", "0", monkeypatch)


@pytest.mark.parametrize("case_id,driver", [
    (c.id, d) for c in NEW_CASES for d in ("python", "library", "library-peer", "python-dense")
    if d != "python-dense" or c.id in OPEN_IDS])
def test_shard_lanes_match_single_context_and_port(case_id, driver, monkeypatch):
    """The lanes of ms_shard_step / ShardedStepper that the displaced uniform sphere under CG never takes (the table in
    shard_cases.py): volume penalty, GD, surface only, open surface with boundary rows, per-vertex / per-facet
    parameters, a volume row over a facet subset, guarded trials, reuse level 1, the implicit steepest-descent restart,
    the edge_fraction clamp.  Each against the single context (as above, plus trials and guard rejections per step),
    the single context against oracle.minimizer_port on the CPU, and each on the condition that it takes its lane.
    "python-dense" runs the open cases only (the dense all-reduce over rows whose flags belong to another rank)."""
    _run_shard_case(BY_ID[case_id], driver, "0", monkeypatch)


def _run_shard_case(case, driver, pair, monkeypatch):
    import torch

    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.parallel import HipShardBackend, LibraryShardedStepper, ShardedStepper

    monkeypatch.setenv("MS_PAIR", pair)
    if case.deterministic:
        monkeypatch.setenv("MS_DETERMINISTIC", "1")  # (why: case.deterministic_why)
    a = materialize(case)
    P, T, fixed = a.P, a.T, a.fixed
    world, tile, level, mods = case.world, case.tile, case.level, case.modules
    n_steps, step0 = case.n_steps, case.step0
    cfg = configure_kwargs(case, a)

    # single context reference
    dm = DeviceMesh(P, T, fixed=fixed, boundary=a.boundary, body_facets=a.body_facets, tile_vertices=tile)
    dm.set_surface_tension(a.gamma)
    dm.set_bending_params(a.kappa, a.c0)
    dm.set_params(modules=mods, **cfg)
    if case.penalty:
        # the penalty lane is taken: the start is off the target volume and the penalty energy slot is not zero
        e_start = dm.energy()
        v_start = dm.fetch_scalars()[L.MS_S_VOL]
        print(f"[{case.id}] start: V={v_start!r} V0={a.V0!r} E_penalty={e_start[2]!r}")
        assert abs(v_start - a.V0) > 1e-3 * abs(a.V0) and e_start[2] > 0.0
        assert abs(a.V_start - a.V0) > 1e-3 * abs(a.V0)
    ref_log, ref_tr, ref_alpha, ref_step_in, step = [], [], [], [], step0
    for _ in range(n_steps):
        r = dm.step(stepper=case.stepper, step_size=step, tol=1e-9, **case.params)
        ref_log.append((float(r.success), r.next_step, r.energy, r.grad_norm))
        ref_tr.append((int(r.trials), int(r.guard_rejects)))
        ref_alpha.append(float(r.alpha))
        ref_step_in.append(step)
        step = r.next_step
        if not r.success:
            dm.reset_stepper()
    x_ref = dm.get_positions()
    dm.close()
    ref = np.array(ref_log)

    if case.anchor:
        _check_against_port(case, a, ref, ref_tr, ref_alpha, ref_step_in, x_ref)

    grp = ThreadGroup(world)
    logs, finals, errors = [None] * world, [None] * world, []
    n_exchanges = [0] * world
    trial_counts = [None] * world
    first_eval = [None] * world  # python drivers, open cases: (owned rows of G in mesh order, folded scalars)
    msg_sizes, bnd = [None] * world, [None] * world
    want_first_eval = case.id in OPEN_IDS and not driver.startswith("library")

    def run(rank):
        try:
            grp.bind(rank)
            be = HipShardBackend(P, T, rank=rank, world=world, device=0, tile_vertices=tile, fixed=fixed,
                                 boundary=a.boundary, body_facets=a.body_facets, group=grp,
                                 debug_poison=not driver.startswith("library"),
                                 exchange="dense" if driver == "python-dense" else "halo")
            be.configure(modules=mods, gamma=a.gamma, kappa=a.kappa, c0=a.c0, **cfg)
            bnd[rank] = dict(be.boundary, header=be.dm.exchange_bytes(()),
                             factors=be.dm.exchange_bytes((L.MS_BUF_FK, L.MS_BUF_FA)))
            if driver == "library":
                be.enable_library_driver()
                drv = LibraryShardedStepper(be, stepper=case.stepper, reuse_energy0=level, **case.params)
            elif driver == "library-peer":
                # no all-gather at all: every rank's pack kernel writes into every peer's slab, flag words order it
                be.enable_peer_exchange()
                drv = LibraryShardedStepper(be, stepper=case.stepper, reuse_energy0=level, **case.params)
            else:
                drv = ShardedStepper(be, stepper=case.stepper, reuse_energy0=level, **case.params)
            if want_first_eval:
                _capture_first_gradient(be, drv, first_eval, rank)
            log, step, tr = [], step0, []
            for _ in range(n_steps):
                r = drv.step(step, tol=1e-9)
                log.append((float(r.success), r.next_step, r.energy, r.grad_norm))
                tr.append((int(r.trials), int(r.guard_rejects)))
                step = r.next_step
                if not r.success:
                    drv.reset()
            logs[rank] = np.array(log)
            n_exchanges[rank] = drv.exchanges
            trial_counts[rank] = tr
            msg_sizes[rank] = list(grp.sizes[rank])
            finals[rank] = be.gather_positions()
            torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            import traceback

            errors.append(traceback.format_exc())
            grp.bar.abort()
            raise e

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors[0]
    if case.anchor:
        print(f"[{case.id}/{driver}] sharded vs single: relerr x {max(relerr(f, x_ref) for f in finals):.3e}, "
              f"E {np.max(np.abs(logs[0][:, 2] / ref[:, 2] - 1)):.3e}, trials {trial_counts[0]}")
    assert ref[:, 0].sum() >= 2
    for rank in range(world):
        got = logs[rank]
        assert np.array_equal(got[:, 0], ref[:, 0]), (got, ref)
        assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12)
        assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-12)
        assert np.allclose(got[:, 3], ref[:, 3], rtol=1e-9)
        assert relerr(finals[rank], x_ref) < 1e-11
        if case.anchor or pair == "0":
            assert trial_counts[rank] == ref_tr, (rank, trial_counts[rank], ref_tr)
    for rank in range(1, world):
        assert np.array_equal(finals[0], finals[rank]), "ranks diverged"
    assert len(set(n_exchanges)) == 1 and n_exchanges[0] > 0
    if level == 2 and not case.constraint and not case.penalty:
        # expected exchange count: one for the energy pass when the factors are not carried over, one for the
        # direction, one per trial.  The library driver sends the gradient rows with the direction, so a
        # steepest-descent restart after a search that failed before its first trial (non-descent direction)
        # needs no direction exchange
        expect, carried, prev_failed_without_trials = 0, False, False
        for i in range(n_steps):
            ok = bool(ref[i, 0])
            trials, guards = trial_counts[0][i]
            implicit = driver.startswith("library") and carried and prev_failed_without_trials
            expect += (0 if carried else 1) + (0 if implicit else 1) + trials + guards
            carried = ok or (trials + guards == 0 and carried)
            prev_failed_without_trials = (not ok) and trials + guards == 0
        if pair == "0":
            assert n_exchanges[0] == expect, (n_exchanges[0], expect, trial_counts[0], ref[:, 0])
        else:
            # a pair evaluates two trials per exchange: every search that reached its second trial saves one
            saved = sum(1 for tr, gd in trial_counts[0] if tr >= 2 and gd == 0)
            assert expect - saved <= n_exchanges[0] <= expect, (n_exchanges[0], expect, saved, trial_counts[0])
            assert saved == 0 or n_exchanges[0] < expect
    if want_first_eval:
        _check_first_evaluation(case, a, first_eval)
    if case.id == "surf_cg":
        _check_trials_carry_no_rows(L, driver, bnd, msg_sizes, n_exchanges[0], trial_counts[0], n_steps)


def _check_against_port(case, a, ref, ref_tr, ref_alpha, ref_step_in, x_ref):
    """The single-context log against oracle.minimizer_port (the loop and the tolerances of
    test_parallel_gloo._worker), and the lane conditions of the case on both runs."""
    port = run_port(case, a)
    dx = float(np.max(np.abs(x_ref - port.x)))
    print(f"[{case.id}] single context vs port: max|dx| {dx:.3e}, "
          f"E {np.max(np.abs(ref[:, 2] / port.log[:, 2] - 1)):.3e}, "
          f"next_step {np.max(np.abs(ref[:, 1] / port.log[:, 1] - 1)):.3e}; success {ref[:, 0].astype(int).tolist()} "
          f"(trials, guards) {ref_tr} port {list(zip(port.trials, port.guards))}")
    assert np.array_equal(ref[:, 0], port.log[:, 0]), (ref[:, 0], port.log[:, 0])
    assert np.allclose(ref[:, 1], port.log[:, 1], rtol=1e-12)
    assert np.allclose(ref[:, 2], port.log[:, 2], rtol=1e-10)
    assert dx < 1e-9
    # the port takes a guard rejection where check_max_normal_change_positions returns False
    assert ref_tr == list(zip(port.trials, port.guards)), (ref_tr, port.trials, port.guards)
    tr, gd = [t for t, _g in ref_tr], [g for _t, g in ref_tr]
    beta = float(case.params.get("beta", 0.7))
    assert not lane_report(case, ref[:, 0], tr, gd, ref_alpha, ref_step_in), lane_report(
        case, ref[:, 0], tr, gd, ref_alpha, ref_step_in)
    assert not lane_report(case, port.log[:, 0], port.trials, port.guards, port.alpha, port.step_in)
    if case.id == "edge_fraction":
        assert clamped_steps(ref[:, 0], tr, gd, ref_alpha, ref_step_in, beta) == clamped_steps(
            port.log[:, 0], port.trials, port.guards, port.alpha, port.step_in, beta)


def _capture_first_gradient(be, drv, first_eval, rank):
    """Hook the Python driver's first gradient pass: right after it (the energy pass, its exchange of the bending
    factors and the fused gradient + direction pass have run) keep this rank's OWNED rows of MS_BUF_G, in mesh
    order, and the folded scalars.  The rows a rank does not own are marked NaN for the read-out and restored."""
    from membrane_solver_amd import _lib as L

    inner = be.phase_gradient_direction

    def hooked(stepper, use_history):
        inner(stepper, use_history)
        if first_eval[rank] is None:
            view = be._view(L.MS_BUF_G)
            keep = view.clone()
            r0, r1 = be.rank * be.rows, (be.rank + 1) * be.rows
            view[:r0] = float("nan")
            view[r1:] = float("nan")
            be.stream.synchronize()
            g = be.dm.get_vertex_buffer(L.MS_BUF_G)
            view.copy_(keep)
            be.stream.synchronize()
            first_eval[rank] = (g, drv.scal.copy())

    be.phase_gradient_direction = hooked


def _check_first_evaluation(case, a, first_eval):
    """Every vertex is owned by exactly one rank, and on its owner the first gradient is the oracle's (G_TOL / E_TOL
    of test_gpu_kernels.py); the folded energies are the oracle's.  A wrong factor on a halo row shows here, on the
    rank that owns the vertex it feeds."""
    from membrane_solver_amd import _lib as L
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc
    from shard_cases import port_problem

    G_TOL, E_TOL = 1e-10, 1e-12
    p, _stepper = port_problem(case, a)
    _E, g_ref = mp.energy_and_gradient(p, p.positions)
    e_surf = orc.surface_energy_and_gradient(a.P, p.tri, a.gamma, None)
    e_bend = orc.bending_energy(a.P, p.tri, a.kappa, a.c0, p.is_boundary)
    owners = np.zeros(len(a.P), dtype=int)
    scale = float(np.max(np.abs(g_ref)))
    for rank, (g, scal) in enumerate(first_eval):
        own = np.isfinite(g).all(axis=1)
        owners += own
        err = float(np.max(np.abs(g[own] - g_ref[own]))) / scale
        print(f"[{case.id}] rank {rank}: {int(own.sum())} owned rows, gradient relerr {err:.3e}, "
              f"E_surf {abs(scal[L.MS_S_ESURF] / e_surf - 1):.3e}, E_bend {abs(scal[L.MS_S_EBEND] / e_bend - 1):.3e}")
        assert own.any()
        assert err < G_TOL, (rank, np.flatnonzero(own)[np.argmax(np.abs(g[own] - g_ref[own]).max(axis=1))])
        assert abs(scal[L.MS_S_ESURF] - e_surf) <= E_TOL * abs(e_surf)
        assert abs(scal[L.MS_S_EBEND] - e_bend) <= E_TOL * abs(e_bend)
    assert np.array_equal(owners, np.ones(len(a.P), dtype=int)), "a vertex is owned by no rank or by two"


def _check_trials_carry_no_rows(L, driver, bnd, msg_sizes, n_exchanges, trials, n_steps):
    """Without bending a trial's exchange is the scalar header alone (n_fb == 0): the shards do have boundary rows, a
    factor exchange would carry them, and of the messages that went through the all-gather only the direction
    exchanges -- at most one per step -- are longer than the header."""
    for b in bnd:
        assert b["max_rows"] > 0 and b["header"] == 8 * L.MS_NSCAL
        assert b["factors"] == 8 * (L.MS_NSCAL + 5 * b["max_rows"])
    if driver == "library-peer":
        return  # (nothing goes through an all-gather; the row buffers of a trial are chosen by the same n_fb)
    for sizes in msg_sizes:
        header_only = sum(1 for n in sizes if n == L.MS_NSCAL)
        assert len(sizes) == n_exchanges
        assert len(sizes) - header_only <= n_steps, sizes
        assert header_only >= sum(t + g for t, g in trials), sizes


def _raw_shard_step(dm, **flags):
    """ms_shard_step with the stepper parameters DeviceMesh.shard_step does not pass.  -> (return code, message)"""
    import ctypes

    from membrane_solver_amd import _lib as L

    sp = L.ms_stepper_params(int(L.MS_STEPPER_CG), 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2,
                             int(flags.get("enforce_volume", 0)), int(flags.get("precondition", 0)),
                             int(flags.get("enforce_pins", 0)))
    r = L.ms_step_result()
    rc = L.lib().ms_shard_step(dm._h, ctypes.byref(sp), 1e-3, 1e-9, ctypes.byref(r))
    return rc, L.lib().ms_last_error(dm._h).decode()


def test_shard_step_refusals_launch_nothing_and_leave_the_context_usable():
    """What ms_shard_step does not shard it refuses by name -- ConjugateGradient(precondition=True), the volume
    projection of every trial, pin tables, the tilt modules -- before any kernel or exchange, and the context goes on
    working.  (body_area_penalty: test_gpu_area.py and test_area_host.py; what HipShardBackend.configure refuses:
    test_area_host.py and test_parallel_gloo.py.)"""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh
    from test_gpu_pins import MODS, _case_mesh, _mz

    P, T = meshgen.icosphere(6)
    P = meshgen.smooth_displace(P, 0.05)
    dm = DeviceMesh(P, T, tile_vertices=64)
    dm.set_surface_tension(np.ones(len(T)))
    dm.set_bending_params(np.full(len(P), 0.9), np.full(len(P), 0.1))
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    e0, g0 = dm.energy_and_gradient()

    def refused(ctx, message, **flags):
        ctx.profile_enable(True)
        ctx.profile_read()
        x0, n0 = ctx.get_positions(), ctx.shard_exchange_count()
        rc, msg = _raw_shard_step(ctx, **flags)
        assert rc == -4 and message in msg, (rc, msg)  # MS_ERR_STATE
        launches = {k: n for k, (_ms, n) in ctx.profile_read().items() if n}
        assert not launches, launches
        assert ctx.shard_exchange_count() == n0 and np.array_equal(ctx.get_positions(), x0)
        ctx.profile_enable(False)

    refused(dm, "ConjugateGradient(precondition=True) is not sharded", precondition=1)
    refused(dm, "volume_projection_during_minimization", enforce_volume=1)
    refused(dm, "pin_to_plane / pin_to_circle are not sharded", enforce_pins=1)
    e1, g1 = dm.energy_and_gradient()
    assert np.array_equal(e0, e1) and relerr(g1, g0) < 1e-12
    r = dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, tol=1e-9)
    assert r.success and r.trials >= 1
    for bit in TILT_BITS(L):
        dm.set_params(modules=L.MS_MOD_SURFACE | bit)
        refused(dm, "the tilt modules are not sharded yet")
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    e2, _g2 = dm.energy_and_gradient()
    assert np.all(np.isfinite(e2)) and e2[0] > 0.0
    dm.close()

    # pin tables on the context, no flag in the stepper parameters
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "pin_cases.npz"))
    mesh = _case_mesh(z, str(z["names"][0]), ["surface"])
    _mirror, pinned = _mz(mesh, MODS, tile=64)._device()
    refused(pinned, "pin_to_plane / pin_to_circle are not sharded")
    pinned.enforce_pins()
    assert pinned.pin_stats()["enforce_launches"] == 1

