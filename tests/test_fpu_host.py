"""First-play urgency, the parts that need no GPU: the knobs checked before anything
touches the device, the C entry points and the argument checks they make on the host, and the properties of the
rule's restatement (tests/fpu_ref.py) on nodes made by hand.  An engine cannot be made without a GPU: the setter's
error returns on a live engine are in tests/test_gpu_fpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fpu_ref as FR
from conftest import REPO

BASE = dict(numMCTSSims=12, cpuct=1.5, tempThreshold=15)


# ------------------------------------------------------------------ 1. knobs
def test_check_fpu_knobs_accepts():
    pytest.importorskip("torch")
    from yacht_amd.replay import check_fpu_knobs as ck
    from yacht_amd.replay import fpu_knobs_of
    assert ck() == (None, None) and ck(None, None) == (None, None)
    assert ck(0) == (0.0, 0.0) and ck(0.25) == (0.25, 0.25) and ck(0.25, 0) == (0.25, 0.0)  # (0 is legal, not off)
    assert ck(np.float32(0.5), np.int64(2)) == (0.5, 2.0)
    assert fpu_knobs_of(dict(BASE)) == dict(fpu_reduction=None, fpu_root_reduction=None)
    assert fpu_knobs_of(dict(BASE, fpuReduction=0.3)) == dict(fpu_reduction=0.3, fpu_root_reduction=0.3)


BAD = [dict(fpuReduction=-1), dict(fpuReduction=-1e-9), dict(fpuReduction=float("nan")), dict(fpuReduction=float("inf")),
       dict(fpuReduction=True), dict(fpuReduction="0.25"), dict(fpuReduction=0.25, fpuRootReduction=-0.5),
       dict(fpuReduction=0.25, fpuRootReduction=float("nan")), dict(fpuReduction=0.25, fpuRootReduction="0"),
       dict(fpuRootReduction=0.25)]  # (the last would silently do nothing)


@pytest.mark.parametrize("extra", BAD)
def test_bad_knobs_raise_before_any_device_call(extra):
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.replay import check_fpu_knobs
    from yacht_amd.utils import dotdict
    args = dotdict(BASE, **extra)
    with pytest.raises(ValueError, match="fpuReduction|fpuRootReduction"):
        check_fpu_knobs(args.get("fpuReduction"), args.get("fpuRootReduction"))
    with pytest.raises(ValueError, match="fpuReduction|fpuRootReduction"):
        Coach(None, None, args)  # (nothing of the game or the net is touched before the check)


def test_coach_defaults_are_off_and_knobs_are_kept():
    pytest.importorskip("torch")
    import inspect

    from yacht_amd import engine, replay
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE))
    assert (c.fpu_reduction, c.fpu_root_reduction) == (None, None)
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE, fpuReduction=0.25, fpuRootReduction=0))
    assert (c.fpu_reduction, c.fpu_root_reduction) == (0.25, 0.0)
    sig = inspect.signature(engine.SelfPlayEngine.__init__).parameters
    assert sig["fpu_reduction"].default is None and sig["fpu_root_reduction"].default is None
    sig = inspect.signature(replay.reanalyse).parameters
    assert sig["fpu_reduction"].default is None and sig["fpu_root_reduction"].default is None
    assert engine.SelfPlayEngine.COUNTER_NAMES[7:9] == ("fpu_unvisited_picks", "fpu_picks")
    assert engine.SelfPlayEngine.COUNTER_NAMES[:7] == ("scan_edges", "prior_window", "prior_sparse", "prior_general",
                                                       "fast_moves", "forced_picks", "pruned_visits")


# ------------------------------------------------------------------ 2. the C ABI
def _header():
    src = open(os.path.join(REPO, "include", "yacht_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_and_binding_declare_the_feature():
    import yacht_amd
    from yacht_amd import _lib, kernels, replay
    src = _header()
    lib = yacht_amd.lib()
    for name in ("yk_engine_set_fpu", "yk_fpu_pick"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
        assert name in _lib._NEWER
    P, L, I, D = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert _lib.SIGNATURES["yk_engine_set_fpu"] == [P, I, D, D]
    assert _lib.SIGNATURES["yk_fpu_pick"] == [P, P, P, P, P, L, D, D, P, P, P]
    assert re.search(r"int yk_engine_set_fpu\(yk_engine_t\* eng, int on, double reduction, double root_reduction\);", src)
    assert re.search(r"int yk_fpu_pick\(const int64_t\* indptr, const float\* p, const int32_t\* counts, "
                     r"const double\* q, const int32_t\* ns,\s+int64_t n, double cpuct, double reduction, "
                     r"int32_t\* pick, int32_t\* unvisited, void\* stream\);", src)
    assert "fpu_pick" in kernels.__all__ and "check_fpu_knobs" in replay.__all__
    # engine state, not a config field: the struct is what it was
    assert C.sizeof(_lib.YkEngineConfigFull) == 88


def test_entry_points_reject_bad_arguments_without_a_device_call():
    import yacht_amd
    from yacht_amd._lib import YK_ERR_ARG
    lib = yacht_amd.lib()
    # no engine: the setter tests its handle first
    for on, r, rr in ((1, 0.25, 0.25), (0, 0.0, 0.0)):
        assert lib.yk_engine_set_fpu(None, on, r, rr) == YK_ERR_ARG
    # yk_fpu_pick: every check below is made before anything touches the device (host buffers stand in)
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    ok = [p, p + 8, p + 16, p + 24, p + 32, 0, 1.0, 0.25, p + 40, p + 48, None]
    for i in (0, 1, 2, 3, 4, 8, 9):  # a NULL pointer
        a = list(ok)
        a[i] = None
        assert lib.yk_fpu_pick(*a) == YK_ERR_ARG, i
    for n in (-1, -2**40):
        a = list(ok)
        a[5] = n
        assert lib.yk_fpu_pick(*a) == YK_ERR_ARG
    for r in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        a = list(ok)
        a[7] = r
        assert lib.yk_fpu_pick(*a) == YK_ERR_ARG, r
    for c in (float("nan"), float("inf")):
        a = list(ok)
        a[6] = c
        assert lib.yk_fpu_pick(*a) == YK_ERR_ARG, c
    for i, j in ((8, 2), (8, 4), (9, 2), (9, 4), (9, 8)):  # an output is an input, or the other output
        a = list(ok)
        a[i] = a[j]
        assert lib.yk_fpu_pick(*a) == YK_ERR_ARG, (i, j)


# ------------------------------------------------------------------ 3. the rule on nodes made by hand
def _node(rng, V, nvis, Ns=None, c=1.0):
    """A node of V edges, nvis of them visited: (u_vis, x_unv, terms, Ns) as fpu_ref.pick takes them."""
    P = rng.dirichlet(np.full(V, 0.3)).astype(np.float32)
    vis = sorted(rng.choice(V, nvis, replace=False).tolist())
    N = {j: int(rng.integers(1, 30)) for j in vis}
    Q = {j: float(rng.choice([-1.0, 1.0, 0.0, rng.uniform(-1, 1), float(np.float32(rng.uniform(-1, 1)))])) for j in vis}
    Ns = sum(N.values()) if Ns is None else Ns
    sq, sqe = np.float32(math.sqrt(Ns)), np.float32(math.sqrt(Ns + 1e-8))
    c32 = np.float32(c)
    u = {j: np.float32(Q[j]) + ((c32 * P[j]) * sq) / np.float32(N[j] + 1) for j in vis}
    x = {j: (c32 * P[j]) * sqe for j in range(V) if j not in N}
    return u, x, [(N[j], Q[j], P[j]) for j in vis], Ns


def _old_rule(u, x):
    both = dict(u)
    both.update(x)
    return min(both, key=lambda j: (-both[j], j))


def test_the_sums_are_integers_and_fq_does_not_depend_on_their_order():
    rng = np.random.default_rng(7)
    for _ in range(50):
        _, _, terms, Ns = _node(rng, 40, 17)
        W = sum(FR.w_term(N, Q) for N, Q, _ in terms)
        Mi = sum(FR.m_term(P) for _, _, P in terms)
        assert isinstance(W, int) and isinstance(Mi, int) and abs(W) <= Ns * 2**32 and Mi <= 2**40 + len(terms)
        want = FR.fpu_value(W, Mi, Ns, 0.25)
        assert want.dtype == np.float32
        for _ in range(5):
            perm = rng.permutation(len(terms))
            t2 = [terms[i] for i in perm]
            got = FR.fpu_value(sum(FR.w_term(N, Q) for N, Q, _ in t2), sum(FR.m_term(P) for _, _, P in t2), Ns, 0.25)
            assert got.view(np.uint32) == want.view(np.uint32)
    # the terms by hand: ties to even at Q 2^32, truncation at P 2^40, a P below 2^-40 adds nothing
    assert FR.w_term(3, 0.5) == 3 * 2**31 and FR.w_term(2, -1.0) == -2 * 2**32
    assert FR.w_term(1, 0.5 * 2.0**-32) == 0 and FR.w_term(1, 1.5 * 2.0**-32) == 2 and FR.w_term(1, 2.5 * 2.0**-32) == 2
    assert FR.m_term(np.float32(2.0**-41)) == 0 and FR.m_term(np.float32(0.0)) == 0 and FR.m_term(np.float32(1.0)) == 2**40
    assert FR.m_term(np.float32(1.75 * 2.0**-40)) == 1
    # fq by hand: two children, W / Ns = -0.5, the whole prior mass tried
    assert FR.fpu_value(FR.w_term(3, -1.0) + FR.w_term(1, 1.0), 2**40, 4, 0.25) == np.float32(-0.75)


def test_a_larger_reduction_never_turns_a_visited_win_into_an_unvisited_one():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(200):
        u, x, terms, Ns = _node(rng, int(rng.integers(2, 60)), 1)
        nv = int(rng.integers(1, max(len(x), 2)))
        u, x, terms, Ns = _node(rng, len(u) + len(x), min(nv, len(u) + len(x) - 1))
        prev = None
        for r in (0.0, 0.1, 0.25, 0.5, 1.0, 4.0):
            j, won, decided = FR.pick(u, x, terms, Ns, r)
            assert decided and (j in x) == won
            if prev is False:
                assert not won  # once the visited candidate wins, it wins for every larger r
            prev = won
            seen.add(won)
    assert seen == {True, False}


def test_ns_zero_and_single_kind_nodes_follow_the_old_rule():
    rng = np.random.default_rng(13)
    for V in (1, 5, 64):
        u, x, terms, Ns = _node(rng, V, V)  # all visited
        assert FR.pick(u, x, terms, Ns, 0.25) == (_old_rule(u, x), False, False)
        u, x, terms, _ = _node(rng, V, 0, Ns=0)  # a fresh node
        assert FR.pick(u, x, terms, 0, 0.25) == (_old_rule(u, x), True, False)
        u, x, terms, _ = _node(rng, V, 0, Ns=9)  # none visited
        assert FR.pick(u, x, terms, 9, 0.25) == (_old_rule(u, x), True, False)
    assert FR.pick({}, {}, [], 0, 0.25) == (-1, False, False)
    # equal priors: the lowest index
    x = {j: np.float32(0.125) for j in range(8)}
    assert FR.pick({}, x, [], 0, 0.0)[0] == 0


def test_the_mover_behind_and_the_mover_ahead_by_hand():
    """The two cases of the issue: with every visited Q < 0 the reference rule takes any unvisited edge, with every
    visited Q > 0 it never does at a small P - the sign of Q decides.  Under the rule the unvisited edges start
    from the children's mean, so the sign drops out: what decides is the reduction against the exploration terms
    (here one child with Q = q, N = 10, P = 0.01: u = q + 0.0029, fq + x = q - 0.1 r + 0.0316)."""
    c32, Ns = np.float32(1.0), 10
    sq, sqe = np.float32(math.sqrt(Ns)), np.float32(math.sqrt(Ns + 1e-8))
    P = np.full(100, 0.01, dtype=np.float32)
    x = {j: (c32 * P[j]) * sqe for j in range(1, 100)}
    for q, old_unvisited in ((-0.5, True), (0.5, False)):
        u = {0: np.float32(q) + ((c32 * P[0]) * sq) / np.float32(11)}
        terms = [(10, q, P[0])]
        assert (_old_rule(u, x) != 0) == old_unvisited
        assert FR.pick(u, x, terms, Ns, 0.0)[:2] == (1, True)   # r = 0: the larger exploration term of N = 0 wins
        assert FR.pick(u, x, terms, Ns, 0.25)[:2] == (1, True)  # 0.025 < 0.0316 - 0.0029
        assert FR.pick(u, x, terms, Ns, 0.5)[:2] == (0, False)  # 0.05 > 0.0287: the visited child again
        assert FR.pick(u, x, terms, Ns, 4.0)[:2] == (0, False)


def test_an_exact_tie_goes_to_the_lower_index():
    # fq + x == u exactly: Q = 0.5 visited with P = 0 (u = 0.5), the unvisited x = 0.25 and fq = 0.25 (mean 0.5,
    # r sqrt(mass) = 0.25 with mass 2^-2... made of a second visited edge that carries the mass and loses)
    c32, Ns = np.float32(1.0), 4
    sqe = np.float32(math.sqrt(Ns + 1e-8))
    x_val = (c32 * np.float32(0.125)) * sqe
    assert x_val == np.float32(0.25)
    for vis_j, unv_j in ((0, 1), (1, 0)):
        u = {vis_j: np.float32(0.5), 2: np.float32(-1.0)}
        x = {unv_j: x_val}
        terms = [(2, 0.5, np.float32(0.0)), (2, 0.5, np.float32(0.25))]  # W / Ns = 0.5, mass 0.25: fq = 0.5 - 0.5 r
        assert FR.fpu_value(sum(FR.w_term(N, Q) for N, Q, _ in terms), sum(FR.m_term(p) for _, _, p in terms), Ns, 0.5) \
            == np.float32(0.25)
        j, won, decided = FR.pick(u, x, terms, Ns, 0.5)
        assert decided and j == min(vis_j, unv_j) and won == (unv_j < vis_j)


def test_numpy_fpu_pick_rows():
    indptr = np.array([0, 3, 3, 5], dtype=np.int64)
    p = np.array([0.5, 0.25, 0.25, 0.5, 0.5], dtype=np.float32)
    counts = np.array([4, 0, 0, 0, 0], dtype=np.int32)
    q = np.array([-0.5, 0, 0, 0, 0], dtype=np.float64)
    ns = np.array([4, 0, 0], dtype=np.int32)
    pick, unv = FR.fpu_pick(indptr, p, counts, q, ns, 1.0, 0.25)
    # row 0: u = -0.5 + 0.5 * 2 / 5 = -0.3; fq = -0.5 - 0.25 sqrt(0.5), x = 0.5: the unvisited entry 1 wins
    assert pick.tolist() == [1, -1, 0] and unv.tolist() == [1, 0, 1]
    pick, unv = FR.fpu_pick(indptr, p, counts, q, ns, 1.0, 4.0)
    assert pick.tolist() == [0, -1, 0] and unv.tolist() == [0, 0, 1]
