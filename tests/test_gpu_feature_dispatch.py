"""The launches pick their kernels by the options that are on (csrc/yk_optarg.h): one
engine taken through the opt-in search features in sequence computes, after every change, exactly what a fresh
engine given only that setting computes - every field of the records, the error word and the counters.  A wrong
instantiation, or state left over from the setting before, is a mismatch.

Root noise is part of an engine's configuration (yk_engine_config_t), not a setter, so no one engine can run both
with and without it: the engine made without it takes every setting but "root temperature + root noise", and a
second engine made with it takes that one between two others of its own (the noise under forced playouts without
pruning + move temperature before it, the noise alone after it), each checked the same way.

The fixed small case of test_gpu_fpu.py: 3 games x 30 simulations, hash prior, cpuct 1.0, seed 2026, envs 300..302.
Three games are one group whatever is asked for (a group is at least 16 games), so the two-group run - every
launch once per group, on the group's own view of the engine - is the same sequence at 32 games."""
import numpy as np
import pytest

import temper_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
SEED, BASE, SIMS, CPUCT, TT = 2026, 300, 30, 1.0, 15
K, RED = 2.0, 0.25
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)  # test_gpu_root_noise.py's
MOVE = dict(move_temperature=T.MOVE_SCHEDULE["final"], move_temperature_early=T.MOVE_SCHEDULE["early"],
            temperature_halflife=T.MOVE_SCHEDULE["halflife"])
ROOT = dict(root_policy_temperature=T.ROOT_SCHEDULE["final"], root_policy_temperature_early=T.ROOT_SCHEDULE["early"],
            temperature_halflife=T.ROOT_SCHEDULE["halflife"])
NONE = dict()
FORCED_PRUNE = dict(forced_playouts_k=K)
FORCED_FPU = dict(forced_playouts_k=K, fpu_reduction=RED)
FPU = dict(fpu_reduction=RED)
FPU_MOVE = dict(fpu_reduction=RED, **MOVE)
FORCED_RAW_MOVE = dict(forced_playouts_k=K, forced_prune=False, **MOVE)
# (name, the constructor's knobs, the counters the setting must move: the feature did run)
PLAIN = [("none", NONE, ()), ("forced+prune", FORCED_PRUNE, ("forced_picks", "pruned_visits")),
         ("forced+fpu", FORCED_FPU, ("forced_picks", "pruned_visits", "fpu_picks")), ("fpu", FPU, ("fpu_picks",)),
         ("fpu+move_t", FPU_MOVE, ("fpu_picks",)), ("forced-prune+move_t", FORCED_RAW_MOVE, ("forced_picks",)),
         ("root_t", ROOT, ()), ("none again", NONE, ())]
NOISY = [("noise+forced-prune+move_t", FORCED_RAW_MOVE, ("forced_picks",)), ("root_t+noise", ROOT, ()), ("noise", NONE, ())]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import engine
    return engine


def _make(E, n, groups, **kw):
    return E.SelfPlayEngine(n, SIMS, CPUCT, TT, prior="hash", max_moves=48, groups=groups, **kw)


def _set(eng, forced_playouts_k=0.0, forced_prune=True, fpu_reduction=None, move_temperature=None,
         move_temperature_early=None, root_policy_temperature=None, root_policy_temperature_early=None,
         temperature_halflife=None):
    """The constructor's knobs through the library's setters, every one of them each time: what is not named is off."""
    from yacht_amd._lib import call
    call("yk_engine_set_forced_playouts", eng.handle, float(forced_playouts_k), int(forced_prune))
    call("yk_engine_set_fpu", eng.handle, int(fpu_reduction is not None), fpu_reduction or 0.0, fpu_reduction or 0.0)
    call("yk_engine_set_temperatures", eng.handle, move_temperature_early or 0.0, move_temperature or 0.0,
         root_policy_temperature_early or 0.0, root_policy_temperature or 0.0, temperature_halflife or 0.0)


def _result(eng):
    eng.run(SEED, BASE)
    return eng.records(), eng.stats()


def _walk(E, n, groups, settings, **fixed):
    """Every setting's (records, stats) on one engine, after checking each against a fresh engine's."""
    eng = _make(E, n, groups, **fixed)
    out = []
    for name, kw, moved in settings:
        _set(eng, **kw)
        rec, st = _result(eng)
        fresh = _make(E, n, groups, **fixed, **kw)
        rec0, st0 = _result(fresh)
        fresh.close()
        assert st0["errors"] == 0 and st0["groups"] == groups, (name, st0)
        for k in moved:
            assert st0[k] > 0, (name, k)
        for k in FIELDS:
            assert np.array_equal(rec[k], rec0[k]), (name, k)
        assert st == st0, (name, st, st0)  # the error word and every counter of yk_engine_counters among them
        out.append((rec, st))
    eng.close()
    return out


@pytest.mark.parametrize("n,groups", [(3, 1), (32, 2)])
def test_one_engine_through_the_settings_is_a_fresh_engine_each_time(E, n, groups):
    plain = _walk(E, n, groups, PLAIN)
    noisy = _walk(E, n, groups, NOISY, **NOISE)
    # the last setting is the first: nothing of the seven between is left
    for k in FIELDS:
        assert np.array_equal(plain[-1][0][k], plain[0][0][k]), k
    assert plain[-1][1] == plain[0][1]
    assert len(noisy) == len(NOISY)
    # the move schedule's T is not 1 on any temp-1 move: every one of them is a tempered draw
    mt = T.MOVE_SCHEDULE
    assert all(mt["final"] + (mt["early"] - mt["final"]) * 2.0 ** (-m / mt["halflife"]) != 1.0 for m in range(TT - 1))
