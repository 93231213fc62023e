"""The score-margin utility, the parts that need no GPU: the knobs checked before anything
touches the device, the C entry points and the checks they make on the host, and the properties of the rule's
restatement (tests/utility_ref.py) on final boards of reference games.  An engine cannot be made without a GPU:
the setter's error returns on a live engine and the kernels are in tests/test_gpu_score_utility.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import utility_ref as UR
import value_ref as V
from conftest import REPO
from oracle import oracle as O

BASE = dict(numMCTSSims=12, cpuct=1.5, tempThreshold=15)


# ------------------------------------------------------------------ 1. knobs
def test_check_score_knobs_accepts():
    pytest.importorskip("torch")
    from yacht_amd.replay import check_score_knobs as ck
    from yacht_amd.replay import score_knobs_of
    assert ck() == (None, None) and ck(None, None) == (None, None)
    assert ck(0, 20000) == (0.0, 20000.0)  # (0 is legal, and is on)
    assert ck(0.5, 1e-3) == (0.5, 1e-3) and ck(1, 1e9) == (1.0, 1e9)
    assert ck(np.float32(0.5), np.int64(1000)) == (0.5, 1000.0)
    assert score_knobs_of(dict(BASE)) == dict(score_utility=None, score_scale=None)
    assert score_knobs_of(dict(BASE, scoreUtility=0.5, scoreScale=20000)) == dict(score_utility=0.5, score_scale=20000.0)


BAD = [(dict(scoreScale=20000), "scoreScale needs scoreUtility"),  # (alone it would silently do nothing)
       (dict(scoreUtility=0.5), "scoreUtility needs scoreScale"),  # (there is no default scale)
       (dict(scoreUtility=-0.1, scoreScale=1000), r"scoreUtility must lie in \[0, 1\]"),
       (dict(scoreUtility=1.5, scoreScale=1000), r"scoreUtility must lie in \[0, 1\]"),
       (dict(scoreUtility=float("nan"), scoreScale=1000), r"scoreUtility must lie in \[0, 1\]"),
       (dict(scoreUtility=True, scoreScale=1000), "scoreUtility must be a number"),
       (dict(scoreUtility="0.5", scoreScale=1000), "scoreUtility must be a number"),
       (dict(scoreUtility=0.5, scoreScale=0), "scoreScale must be finite and > 0"),
       (dict(scoreUtility=0.5, scoreScale=-1000), "scoreScale must be finite and > 0"),
       (dict(scoreUtility=0.5, scoreScale=float("nan")), "scoreScale must be finite and > 0"),
       (dict(scoreUtility=0.5, scoreScale=float("inf")), "scoreScale must be finite and > 0"),
       (dict(scoreUtility=0.5, scoreScale="1000"), "scoreScale must be a number")]


@pytest.mark.parametrize("extra,message", BAD)
def test_bad_knobs_raise_before_any_device_call(extra, message):
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.replay import check_score_knobs
    from yacht_amd.utils import dotdict
    args = dotdict(BASE, **extra)
    with pytest.raises(ValueError, match=message):
        check_score_knobs(args.get("scoreUtility"), args.get("scoreScale"))
    with pytest.raises(ValueError, match=message):
        Coach(None, None, args)  # (nothing of the game or the net is touched before the check)


def test_coach_defaults_are_off_and_knobs_are_kept():
    pytest.importorskip("torch")
    import inspect

    from yacht_amd import engine, replay
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE))
    assert (c.score_utility, c.score_scale) == (None, None)
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE, scoreUtility=0, scoreScale=20000))
    assert (c.score_utility, c.score_scale) == (0.0, 20000.0)
    for fn in (engine.SelfPlayEngine.__init__, replay.reanalyse, replay.examples_from_images):
        sig = inspect.signature(fn).parameters
        assert sig["score_utility"].default is None and sig["score_scale"].default is None
    assert engine.SelfPlayEngine.COUNTER_NAMES[9] == "utility_terminals"
    assert engine.SelfPlayEngine.COUNTER_NAMES[:9] == (
        "scan_edges", "prior_window", "prior_sparse", "prior_general", "fast_moves", "forced_picks", "pruned_visits",
        "fpu_unvisited_picks", "fpu_picks")


# ------------------------------------------------------------------ 2. the C ABI
def test_header_and_binding_declare_the_feature():
    import yacht_amd
    from yacht_amd import _lib, kernels, replay
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "yacht_hip.h")).read(), flags=re.S)
    lib = yacht_amd.lib()
    for name in ("yk_engine_set_score_utility", "yk_score_utility", "yk_examples_utility_targets"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
        assert name in _lib._NEWER
    P, L, I, D = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert _lib.SIGNATURES["yk_engine_set_score_utility"] == [P, I, D, D]
    assert _lib.SIGNATURES["yk_score_utility"] == [P, P, I, D, D, P, P, P]
    vt = _lib.SIGNATURES["yk_examples_value_targets"]
    assert _lib.SIGNATURES["yk_examples_utility_targets"] == vt[:10] + [D, D] + vt[10:]  # its arguments plus two
    assert "score_utility" in kernels.__all__
    assert "check_score_knobs" in replay.__all__ and "score_knobs_of" in replay.__all__
    assert C.sizeof(_lib.YkEngineConfigFull) == 88  # engine state, not a config field


def test_entry_points_reject_bad_arguments_without_a_device_call():
    import yacht_amd
    from yacht_amd._lib import YK_ERR_ARG
    lib = yacht_amd.lib()
    bad = [(-0.1, 1000.0), (1.5, 1000.0), (float("nan"), 1000.0), (float("inf"), 1000.0), (0.5, 0.0), (0.5, -1.0),
           (0.5, float("nan")), (0.5, float("inf")), (0.5, -float("inf"))]
    for on, w, c in ((1, 0.5, 20000.0), (0, 0.0, 1.0)):  # no engine: the setter tests its handle first
        assert lib.yk_engine_set_score_utility(None, on, w, c) == YK_ERR_ARG
    buf = (C.c_int64 * 32)()
    p = C.addressof(buf)
    for w, c in bad:  # (host buffers stand in: the checks come before anything touches the device)
        assert lib.yk_score_utility(p, p + 64, 1, w, c, p + 128, p + 192, None) == YK_ERR_ARG, (w, c)
        assert lib.yk_examples_utility_targets(p, 1, 1, 1, 1, 1, 0, 0, 0.0, 1.0, w, c, p, None, None, None) == YK_ERR_ARG
    assert lib.yk_score_utility(p, p + 64, -1, 0.5, 1000.0, p + 128, p + 192, None) == YK_ERR_ARG
    for i in (0, 1, 5):  # a NULL pointer
        a = [p, p + 64, 1, 0.5, 1000.0, p + 128, p + 192, None]
        a[i] = None
        assert lib.yk_score_utility(*a) == YK_ERR_ARG, i
    assert lib.yk_score_utility(None, None, 0, 0.5, 1000.0, None, None, None) == 0  # no states: nothing to do
    # yk_examples_value_targets' own checks, with good knobs
    for beta, lam in ((-0.1, 1.0), (0.0, 1.5), (float("nan"), 1.0)):
        assert lib.yk_examples_utility_targets(p, 1, 1, 1, 1, 1, 0, 0, beta, lam, 0.5, 1000.0, p, None, None,
                                               None) == YK_ERR_ARG
    assert lib.yk_examples_utility_targets(None, 1, 1, 1, 1, 1, 0, 0, 0.0, 1.0, 0.5, 1000.0, p, None, None, None) == YK_ERR_ARG


# ------------------------------------------------------------------ 3. the rule
WS = (0.0, 0.25, 0.5, 1.0)
CS = (1e-3, 1000.0, 20000.0, 1e9)


def _greedy_final(env):
    """The final board of a game between two greedy players (the oracle plays it): a terminal state."""
    board, ctr = O.init_board(77, [env])
    board, c, cur = board[0], int(ctr[0]), 1
    while float(O.ended(board, cur)[0][0]) == 0:
        a, cc = O.greedy_play(O.canonical(board, cur)[0], 77, [env], c)
        nxt, npl, st, cc = O.step(board, cur, int(a[0]), 77, env, int(cc[0]))
        assert st[0] == 0
        board, cur, c = nxt[0], int(npl[0]), int(cc[0])
    return np.asarray(board, dtype=np.uint64)


@pytest.fixture(scope="module")
def finals():
    out = [_greedy_final(env) for env in range(6)]
    for f in out:
        assert float(O.ended(f, 1)[0][0]) != 0
    return out


def _draw_state():
    """A terminal state with equal totals, made by hand: every category of both players used, all scores 0."""
    from yacht_amd.state import PlayerState, YachtState, pack
    w = pack(YachtState(round_no=13, p1=PlayerState(used_mask=0xFFF), p2=PlayerState(used_mask=0xFFF)))
    ended, tot = O.ended(w, 1)
    assert float(ended[0]) == 1e-4 and int(tot[0][0]) == int(tot[0][1])
    return w


def test_rule_is_bounded_odd_and_monotone(finals):
    for f in finals:
        m = UR.margin(f)
        for w in WS:
            for c in CS:
                u1, u2 = UR.utility(f, 1, w, c), UR.utility(f, -1, w, c)
                assert isinstance(u1, np.float64) and abs(u1) <= 1.0 and abs(u2) <= 1.0
                if m != 0:  # (a draw's 1e-4 is the same for both players)
                    assert u2 == -u1
                else:
                    assert u1 == u2 == (1.0 - w) * 1e-4
    # g is odd, bounded and monotone in m at every scale; u adds the step of z at m = 0
    ms = [-300000, -271000, -1000, -1, 0, 1, 1000, 291000, 300000]
    for c in CS:
        g = [UR.squash(1, m, c) for m in ms]
        assert all(abs(x) < 1.0 for x in g)
        assert all(a <= b for a, b in zip(g, g[1:])) and g[4] == 0.0
        assert [UR.squash(-1, m, c) for m in ms] == [-x for x in g]
        for w in WS:
            u = [UR.blend(np.sign(m) if m else 1e-4, x, w) for m, x in zip(ms, g)]
            assert all(a <= b for a, b in zip(u, u[1:])), (c, w)
            assert max(abs(x) for x in u) <= 1.0


def test_weight_zero_is_the_outcome_and_weight_one_the_squash(finals):
    for f in finals:
        for player in (1, -1):
            z = np.float64(O.ended(f, player)[0][0])
            for c in CS:
                u0 = UR.utility(f, player, 0.0, c)
                assert u0.tobytes() == z.tobytes()  # bit for bit
                assert UR.utility(f, player, 1.0, c) == UR.squash(player, UR.margin(f), c)


def test_a_draw_is_terminal_with_utility_zero_at_weight_one():
    d = _draw_state()
    assert UR.margin(d) == 0
    for player in (1, -1):
        assert UR.utility(d, player, 1.0, 20000.0) == 0.0
        assert UR.utility(d, player, 0.0, 20000.0) == 1e-4
        assert UR.utility(d, player, 0.5, 20000.0) == 0.5 * 1e-4
    # the search still ends there: Es decides, not u
    m = UR.mcts_class(1.0, 20000.0)(1, 0, None, 1, 1.0)
    assert m.search(d) == 0.0 and m.terminal_returns == 1 and not m.Ps


def test_a_state_that_is_not_terminal_has_utility_zero():
    board, _ = O.init_board(77, [0])
    assert UR.utility(board[0], 1, 0.5, 20000.0) == 0.0 and UR.margin(board[0]) == 0


# ------------------------------------------------------------------ 4. the value targets' restatement
def test_value_targets_at_weight_zero_are_value_refs():
    rng = np.random.default_rng(5)
    for T, beta, lam in ((48, 0.0, 1.0), (48, 0.5, 1.0), (48, 0.0, 0.7), (7, 0.3, 0.5), (1, 0.3, 0.5)):
        players = rng.choice([-1, 1], T)
        z = players * rng.choice([-1.0, 1.0])
        q = rng.uniform(-1, 1, T).astype(np.float32)
        want = V.value_targets(q, z, players, T, beta, lam)
        for g1 in (-0.9, 0.0, 0.37):
            got = UR.value_targets(q, z, players, T, beta, lam, g1, 0.0)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (T, beta, lam)
        on = UR.value_targets(q, z, players, T, beta, lam, 0.37, 0.5)
        assert not np.array_equal(on, want) and np.all(np.abs(on) <= 1.0)
    # at (0, 1) the target is float32(p_t * U_t)
    players, z = np.array([1, -1, 1]), np.array([1.0, -1.0, 1.0])
    got = UR.value_targets(np.zeros(3, np.float32), z, players, 3, 0.0, 1.0, 0.25, 0.5)
    assert got.tolist() == [np.float32(0.625), np.float32(-0.625), np.float32(0.625)]
