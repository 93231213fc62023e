"""Forced playouts and policy target pruning, the parts that need no GPU: the knobs checked
before anything touches the device, the C entry points and the argument checks they make on the host, and the
properties of the rule's restatement (tests/forced_ref.py) on rows made by hand.  An engine cannot be made
without a GPU: the setter's error returns on a live engine are in tests/test_gpu_forced_playouts.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import forced_ref as F
from conftest import REPO

BASE = dict(numMCTSSims=12, cpuct=1.5, tempThreshold=15)


# ------------------------------------------------------------------ 1. knobs
def test_check_forced_knobs_accepts():
    pytest.importorskip("torch")
    from yacht_amd.replay import check_forced_knobs as ck
    assert ck() == (0.0, True) and ck(None, None) == (0.0, True) and ck(0, True) == (0.0, True)
    assert ck(2) == (2.0, True) and ck(2.0, False) == (2.0, False) and ck(np.float32(0.5), None) == (0.5, True)
    assert ck(np.int64(3), np.bool_(False)) == (3.0, False)


BAD = [dict(forcedPlayoutsK=-1), dict(forcedPlayoutsK=-1e-9), dict(forcedPlayoutsK=float("nan")),
       dict(forcedPlayoutsK=float("inf")), dict(forcedPlayoutsK=True), dict(forcedPlayoutsK="2"),
       dict(forcedPlayoutsK=2, forcedPrune=1), dict(forcedPlayoutsK=2, forcedPrune="no"),
       dict(forcedPrune=False), dict(forcedPlayoutsK=0, forcedPrune=False)]  # (the last two would silently do nothing)


@pytest.mark.parametrize("extra", BAD)
def test_bad_knobs_raise_before_any_device_call(extra):
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.replay import check_forced_knobs
    from yacht_amd.utils import dotdict
    args = dotdict(BASE, **extra)
    with pytest.raises(ValueError, match="forcedPlayoutsK|forcedPrune"):
        check_forced_knobs(args.get("forcedPlayoutsK"), args.get("forcedPrune"))
    with pytest.raises(ValueError, match="forcedPlayoutsK|forcedPrune"):
        Coach(None, None, args)  # (nothing of the game or the net is touched before the check)


def test_coach_defaults_are_off_and_knobs_are_kept():
    pytest.importorskip("torch")
    import inspect

    from yacht_amd import engine
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE))
    assert (c.forced_k, c.forced_prune) == (0.0, True)
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE, forcedPlayoutsK=2, forcedPrune=False))
    assert (c.forced_k, c.forced_prune) == (2.0, False)
    sig = inspect.signature(engine.SelfPlayEngine.__init__).parameters
    assert sig["forced_playouts_k"].default == 0.0 and sig["forced_prune"].default is True
    assert engine.SelfPlayEngine.COUNTER_NAMES[5:7] == ("forced_picks", "pruned_visits")
    assert engine.SelfPlayEngine.COUNTER_NAMES[:5] == ("scan_edges", "prior_window", "prior_sparse", "prior_general",
                                                       "fast_moves")


# ------------------------------------------------------------------ 2. the C ABI
def _header():
    src = open(os.path.join(REPO, "include", "yacht_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_and_binding_declare_the_feature():
    import yacht_amd
    from yacht_amd import _lib, kernels, replay
    src = _header()
    lib = yacht_amd.lib()
    for name in ("yk_engine_set_forced_playouts", "yk_policy_prune"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
        assert name in _lib._NEWER
    P, L, I, D = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert _lib.SIGNATURES["yk_engine_set_forced_playouts"] == [P, D, I]
    assert _lib.SIGNATURES["yk_policy_prune"] == [P, P, P, P, P, P, L, D, D, P, P]
    assert re.search(r"int yk_engine_set_forced_playouts\(yk_engine_t\* eng, double k, int prune\);", src)
    assert re.search(r"int yk_policy_prune\(const int64_t\* indptr, const int32_t\* cols, const int32_t\* counts, "
                     r"const double\* q, const float\* p,\s+const int32_t\* ns, int64_t n, double k, double cpuct, "
                     r"int32_t\* out, void\* stream\);", src)
    assert replay.policy_prune is kernels.policy_prune and "check_forced_knobs" in replay.__all__


def test_entry_points_reject_bad_arguments_without_a_device_call():
    import yacht_amd
    from yacht_amd._lib import YK_ERR_ARG
    lib = yacht_amd.lib()
    # no engine: the setter tests its handle first
    for k, prune in ((2.0, 1), (0.0, 0)):
        assert lib.yk_engine_set_forced_playouts(None, k, prune) == YK_ERR_ARG
    # yk_policy_prune: every check below is made before anything touches the device (host buffers stand in)
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    ok = [p, p + 8, p + 16, p + 24, p + 32, p + 40, 0, 2.0, 1.5, p + 48, None]
    for i in (0, 1, 2, 3, 4, 5, 9):  # a NULL pointer
        a = list(ok)
        a[i] = None
        assert lib.yk_policy_prune(*a) == YK_ERR_ARG, i
    for n in (-1, -2**40):
        a = list(ok)
        a[6] = n
        assert lib.yk_policy_prune(*a) == YK_ERR_ARG
    for k in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        a = list(ok)
        a[7] = k
        assert lib.yk_policy_prune(*a) == YK_ERR_ARG, k
    a = list(ok)
    a[9] = a[2]  # the output is one of the inputs
    assert lib.yk_policy_prune(*a) == YK_ERR_ARG


# ------------------------------------------------------------------ 3. the rule on rows made by hand
def _puct(Q, P, Ns, c, n):
    return Q + (c * float(np.float32(P))) * math.sqrt(Ns) / (1 + n)


def test_forced_test_by_hand():
    P = np.float32(0.25)
    # (k P) Ns = 2 * 0.25 * 18 = 9: forced while N^2 < 9
    assert [F.forced(N, P, 18, 2.0) for N in range(5)] == [False, True, True, False, False]
    assert not F.forced(1, P, 0, 2.0) and not F.forced(1, P, 18, 0.0)
    assert not F.forced(0, np.float32(1.0), 10**6, 10.0)  # unvisited: never
    assert [F.floor_root(x) for x in (-1.0, 0.0, 0.99, 1.0, 8.99, 9.0, 9.01, 1e18)] == [0, 0, 0, 1, 2, 3, 3, 10**9]
    assert F.floor_root(float("nan")) == 0


def test_best_child_is_never_changed_and_bounds_hold():
    rng = np.random.default_rng(5)
    for _ in range(300):
        m = int(rng.integers(1, 12))
        acts = sorted(int(a) for a in rng.choice(3226, m, replace=False))
        N = [int(x) for x in rng.integers(1, 40, m)]
        Q = [float(x) for x in rng.uniform(-1, 1, m)]
        P = rng.dirichlet(np.ones(m)).astype(np.float32)
        Ns, k, c = sum(N) + int(rng.integers(0, 3)), float(rng.choice([0.5, 2.0, 8.0])), 1.5
        out = F.prune_row(acts, N, Q, P, Ns, k, c)
        star = N.index(max(N))  # the lowest action among the largest counts (acts ascend)
        assert out[star] == N[star]
        bound = _puct(Q[star], P[star], Ns, c, N[star])
        for i in range(m):
            f = F.floor_root((k * float(P[i])) * float(Ns))
            # at most f visits are taken - but for the lone visit left over by that, which is dropped
            assert N[i] - f <= out[i] <= N[i] or (out[i] == 0 and N[i] - f == 1)
            assert out[i] != 1 or N[i] == 1  # a 1 is only ever an untouched single visit
            if i != star and not _puct(Q[i], P[i], Ns, c, N[i] - 1) < bound:
                assert out[i] == N[i]  # its PUCT at N - 1 is not below the bound: nothing is taken


def test_an_edge_reduced_to_one_becomes_zero():
    # edge 1 (P 1/32, Q -1): f = floor_root(2 * 100 / 32) = floor_root(6.25) = 2, so N = 3 can fall to 1 - and is dropped
    acts, N, Q, P = [4, 9], [97, 3], [0.5, -1.0], np.array([0.9, 0.03125], dtype=np.float32)
    assert F.floor_root((2.0 * float(P[1])) * 100.0) == 2
    assert F.prune_row(acts, N, Q, P, 100, 2.0, 1.5) == [97, 0]
    # with N = 4 it stops at 2 and stays
    assert F.prune_row(acts, [96, 4], Q, P, 100, 2.0, 1.5) == [96, 2]
    # a lone visit that nothing was taken from stays (k = 0: f = 0)
    assert F.prune_row(acts, [99, 1], Q, P, 100, 0.0, 1.5) == [99, 1]
    # and one that the loop takes goes to 0 through the loop itself
    assert F.prune_row(acts, [99, 1], Q, P, 100, 2.0, 1.5) == [99, 0]


def test_single_edge_and_equal_counts():
    P1 = np.array([1.0], dtype=np.float32)
    assert F.prune_row([7], [25], [0.3], P1, 25, 2.0, 1.5) == [25]
    # equal counts: the lowest action is c*, and the others are judged against its PUCT
    P = np.array([0.25, 0.25, 0.25, 0.25], dtype=np.float32)
    out = F.prune_row([3, 10, 11, 500], [5, 5, 5, 5], [0.0, 0.9, -0.9, 0.0], P, 20, 2.0, 1.5)
    assert out[0] == 5
    assert out[1] == 5  # a higher Q: its PUCT at N - 1 is above the bound
    # f = floor_root(2 * 0.25 * 20) = 3 for each; Q = -0.9 falls the whole way (5 -> 2), the equal-Q edge too: at
    # n - 1 = 4 its PUCT equals the bound (not below), so it keeps 5
    assert out == [5, 5, 2, 5]
    # the tie rule follows the action, not the position
    assert F.prune_row([10, 3], [5, 5], [-0.9, 0.0], P[:2], 10, 2.0, 1.5)[1] == 5


def test_numpy_policy_prune_rows():
    indptr = np.array([0, 2, 2, 5], dtype=np.int64)
    cols = np.array([4, 9, 1, 2, 3], dtype=np.int32)
    counts = np.array([97, 3, 0, 6, 6], dtype=np.int32)
    q = np.array([0.5, -1.0, 0.0, 0.1, 0.1])
    p = np.array([0.9, 0.03125, 0.5, 0.25, 0.25], dtype=np.float32)
    ns = np.array([100, 0, 12], dtype=np.int32)
    out = F.policy_prune(indptr, cols, counts, q, p, ns, 2.0, 1.5)
    assert out.dtype == np.int32 and out.tolist() == [97, 0, 0, 6, 6]
    assert np.array_equal(F.policy_prune(indptr, cols, counts, q, p, ns, 0.0, 1.5), counts)
