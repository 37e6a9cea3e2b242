"""What test_gpu_multi_trial.py rests on, checked on the CPU with the oracle alone: the meshes of multi_trial_cases.py
have the tile counts the block map is tested at, and their Armijo ladders are long, monotone behind the first
accepted alpha and clear of rounding."""

import ctypes

import numpy as np
import pytest

import multi_trial_cases as mt


@pytest.mark.parametrize("name", list(mt.MESHES))
def test_multi_trial_ladders_are_long_monotone_and_clear_of_rounding(name):
    from membrane_solver_amd import _lib as L

    cs = mt.case(name)
    freq, tile, tiles, _seed, beta = mt.MESHES[name]
    assert len(cs.P) == 10 * freq * freq + 2
    st = (ctypes.c_int64 * 8)()
    assert L.lib().ms_plan_tiling(len(cs.P), len(cs.T), cs.P.ctypes.data_as(L._D), cs.T.ctypes.data_as(L._I32), tile, 1,
                                  st, None) == 0
    assert st[0] == tiles == -(-len(cs.P) // (tile or 256))
    lad = mt.check_preconditions(name)
    # 20 <= R <= max_iter - 4, the whole ladder below the safe limit (the queued regime), exact alphas
    assert mt.MIN_REJECTED <= lad.R <= mt.MAX_ITER - 4
    assert lad.alphas[0] == cs.alpha0 < cs.safe and np.array_equal(lad.alphas, mt.alphas_from(cs.alpha0, lad.R + 4, beta))
    assert lad.gdd < 0.0


@pytest.mark.parametrize("name", ["ico6", "ico15"])
def test_starts_above_the_accepted_alpha_accept_at_the_same_alpha(name):
    """test_acceptance_at_every_slot starts k = 0 ... 15 alphas above the accepted one: every start stays below the safe
    limit and the oracle's search from it takes k + 1 trials."""
    from oracle import minimizer_port as mp

    cs = mt.case(name)
    lad = mt.check_preconditions(name)
    a_acc = lad.alphas[lad.R]
    for k in range(16):
        a0 = a_acc / cs.beta ** k
        assert a0 < cs.safe
        ls = mp.line_search(mt.problem(cs), -cs.g, cs.g, a0, max_iter=mt.MAX_ITER, beta=cs.beta, c=mt.C1,
                            gamma=mt.GAMMA, alpha_max_factor=mt.ALPHA_MAX_FACTOR)
        assert ls.success and ls.trials == k + 1 and abs(ls.alpha - a_acc) <= 1e-14 * a_acc, (k, ls)
