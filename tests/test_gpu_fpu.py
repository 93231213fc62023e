"""First-play urgency on the GPU: opt-in, in every search of an engine it is set on.

* off is off: unset, on = 0 through the setter, and on = 0 after a setter call - every record and counter is the
  default engine's;
* on, every game equals tests/fpu_ref.play_episode bit for bit - the plain-Python Coach / MCTS of noise_ref and
  forced_ref with the rule at every node that has both kinds of edge - with a root reduction of its own, on every
  scan path, under root noise with forced playouts and pruning, and under the playout cap (fast moves too);
* yk_mcts_search, the MCTS plugin and both arenas against the same searches;
* yk_fpu_pick against the numpy restatement on nodes made by hand, exactly; the Coach's engines."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import forced_ref as F
import fpu_ref as FR
import noise_ref as R
import playout_ref as PR
from conftest import REPO
from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
ALPHA, EPS = 0.3, 0.25  # test_gpu_root_noise.py's
NOISE = dict(dirichlet_alpha=ALPHA, dirichlet_eps=EPS)
TT = 15
# the fixed case: 3 games x 30 simulations, hash prior, cpuct 1.0
SEED, BASE, SIMS, CPUCT, RED = 2026, 300, 30, 1.0, 0.25
COUNTERS = ("fpu_unvisited_picks", "fpu_picks")


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import yacht_amd
    from yacht_amd import engine, nnet
    return yacht_amd, engine, nnet


@pytest.fixture(scope="module")
def net(Y):
    _, _, N = Y
    return N.YkNet(spec.closed_form_weights(256, 6), 256, 6)


def _run(E, n, sims, seed, base, net=None, priors=False, setter=None, cpuct=1.5, **kw):
    eng = E.SelfPlayEngine(n, sims, cpuct, TT, net=net, prior="hash" if net is None else "net", max_moves=48, **kw)
    if setter is not None:
        setter(eng)
    eng.run(seed, base)
    st, rec = eng.stats(), eng.records()
    pri = eng.root_priors() if priors else None
    eng.close()
    assert st["errors"] == 0, st
    return (rec, st, pri) if priors else (rec, st)


def _same(r1, r0):
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k


def _injector(before, after, e, full=None):
    """test_gpu_forced_playouts.py's: the move's recorded P' handed to the reference."""
    def inject(move, P):
        assert full is None or full[move]
        assert np.array_equal(P.view(np.uint32), before[e, move].view(np.uint32)), (e, move)
        return after[e, move].copy()
    return inject


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("prior,n,groups", [("hash", 48, 1), ("hash", 48, 2), ("net", 6, 1), ("net", 6, 2)])
def test_off_is_off(Y, net, prior, n, groups):
    """The shapes of test_gpu_forced_playouts.py's test_off_is_off.  Unset is the default engine; so is on = 0
    through the setter, whatever reductions come with it, and on = 0 after the rule had been set on."""
    _, E, _ = Y
    from yacht_amd._lib import call
    nt = net if prior == "net" else None
    r0, s0 = _run(E, n, 12, 707, 900, net=nt, groups=groups)
    assert s0["fpu_unvisited_picks"] == 0 and s0["fpu_picks"] == 0

    def on_then_off(eng):
        call("yk_engine_set_fpu", eng.handle, 1, 0.25, 0.0)
        call("yk_engine_set_fpu", eng.handle, 0, 0.25, 0.0)

    cases = [dict(fpu_reduction=None), dict(setter=lambda eng: call("yk_engine_set_fpu", eng.handle, 0, 0.0, 0.0)),
             dict(setter=lambda eng: call("yk_engine_set_fpu", eng.handle, 0, 0.3, 4.0)), dict(setter=on_then_off)]
    for kw in cases:
        r1, s1 = _run(E, n, 12, 707, 900, net=nt, groups=groups, **kw)
        _same(r1, r0)
        assert s1 == s0
    # and on is not off (r = 0 included: the unvisited edges then start at the parent's estimate)
    r2, s2 = _run(E, n, 12, 707, 900, net=nt, groups=groups, fpu_reduction=0.0)
    assert s2["fpu_picks"] > 0 and not np.array_equal(r2["visits"], r0["visits"])


def test_setter_rejects_bad_arguments_and_leaves_the_engine(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_ARG, YkError, call
    lib = __import__("yacht_amd").lib()
    for kw in (dict(fpu_reduction=-1.0), dict(fpu_reduction=float("nan")), dict(fpu_reduction=float("inf")),
               dict(fpu_reduction=0.25, fpu_root_reduction=-1.0), dict(fpu_reduction=0.25, fpu_root_reduction=float("nan"))):
        with pytest.raises(YkError) as ei:
            E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, **kw)
        assert ei.value.code == YK_ERR_ARG, kw
    with pytest.raises(ValueError, match="fpu_root_reduction"):
        E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, fpu_root_reduction=0.25)
    r0, s0 = _run(E, 2, 12, 5, 0)
    eng = E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48)
    bad = (-1.0, -1e-300, float("nan"), float("inf"), -float("inf"))
    for on in (0, 1):
        for x in bad:
            assert lib.yk_engine_set_fpu(C.c_void_p(eng.handle), on, x, 0.25) == YK_ERR_ARG, (on, x)
            assert lib.yk_engine_set_fpu(C.c_void_p(eng.handle), on, 0.25, x) == YK_ERR_ARG, (on, x)
    eng.run(5, 0)  # still off
    _same(eng.records(), r0)
    assert eng.stats() == s0
    call("yk_engine_set_fpu", eng.handle, 1, 0.0, 1e300)  # the bounds themselves are legal
    call("yk_engine_set_fpu", eng.handle, 1, 1e-300, 0.0)
    eng.close()


# ------------------------------------------------------------------ 2. bit for bit
def _reference(root=None, **kw):
    games = [FR.play_episode(SEED, BASE + e, SIMS, r=RED, r_root=root, cpuct=CPUCT, **kw) for e in range(3)]
    tot = {k: [sum(g[k][i] for g in games) for i in (0, 1)] for k in ("vis_wins", "unv_wins", "differs")}
    tot.update({k: sum(g[k] for g in games) for k in COUNTERS})
    return games, tot


@pytest.fixture(scope="module")
def fixed_ref():
    return _reference()


@pytest.fixture(scope="module")
def fixed_run(Y):
    _, E, _ = Y
    return _run(E, 3, SIMS, SEED, BASE, cpuct=CPUCT, fpu_reduction=RED)


def test_fixed_case_is_the_reference(fixed_run, fixed_ref):
    """Chosen on the CPU with the rule restated: the reference takes 3880 / 121 visited / unvisited wins at roots
    and 8434 / 836 at interior nodes; 2080 root picks and 5055 interior picks differ from the reference rule's."""
    rec, st = fixed_run
    games, tot = fixed_ref
    print("reference:", tot)
    for k in ("vis_wins", "unv_wins", "differs"):  # every branch, at both depth classes, on the reference alone
        assert tot[k][0] >= 100 and tot[k][1] >= 100, (k, tot[k])
    for e, g in enumerate(games):
        R.assert_game_equals_records(g, rec, e)
    assert tot["fpu_picks"] == sum(tot["vis_wins"]) + sum(tot["unv_wins"])
    assert (st["fpu_unvisited_picks"], st["fpu_picks"]) == (tot["fpu_unvisited_picks"], tot["fpu_picks"])
    assert st["forced_picks"] == 0 and st["pruned_visits"] == 0


def test_root_reduction_is_its_own(Y, fixed_run):
    """Root reduction 0, interior 0.25: other games than the fixed case's, and the reference's."""
    _, E, _ = Y
    rec, st = _run(E, 3, SIMS, SEED, BASE, cpuct=CPUCT, fpu_reduction=RED, fpu_root_reduction=0.0)
    games, tot = _reference(root=0.0)
    for e, g in enumerate(games):
        R.assert_game_equals_records(g, rec, e)
    assert (st["fpu_unvisited_picks"], st["fpu_picks"]) == (tot["fpu_unvisited_picks"], tot["fpu_picks"])
    assert tot["unv_wins"][0] >= 100  # (r = 0 at the root: the unvisited candidate wins more often there)
    assert not np.array_equal(rec["visits"], fixed_run[0]["visits"])


# ------------------------------------------------------------------ 3. every scan path
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "nypc-yacht-auction_amd"))
from oracle import spec
from yacht_amd import engine as E, nnet as N
net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6)
VARS = ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY")
out = {}
for tag, env in (("full", {"YK_ROOT_SCAN": "0"}), ("k5", {"YK_ROOT_K": "5"}), ("nosum", {"YK_NODE_SUMMARY": "0"})):
    for k in VARS:
        os.environ.pop(k, None)
    os.environ.update(env)  # (read when the engine is made)
    for case, eng in (("hash", E.SelfPlayEngine(3, 30, 1.0, 15, prior="hash", max_moves=48, fpu_reduction=0.25)),
                      ("net", E.SelfPlayEngine(8, 30, 1.5, 15, net=net, max_moves=48, fpu_reduction=0.25,
                                               fpu_root_reduction=0.1))):
        eng.run(2026, 300)
        st, rec = eng.stats(), eng.records()
        eng.close()
        assert st["errors"] == 0, st
        for f in ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits"):
            out["%s_%s_%s" % (tag, case, f)] = rec[f]
        out["%s_%s_counters" % (tag, case)] = np.array(
            [st[c] for c in ("fpu_unvisited_picks", "fpu_picks", "expansions", "path_edges", "scanned")], dtype=np.int64)
np.savez(sys.argv[2], **out)
"""


def test_every_scan_path_picks_alike(Y, net, fixed_run, tmp_path, monkeypatch):
    """The fixed case (which the reference settles) and 8 net-prior games with a root reduction of their own: the
    default engine (root_scan over the sorted root order and the visited list, node summaries, full scans for bid
    roots and a move's first simulation) against, in a fresh child process, YK_ROOT_SCAN=0 (every root pick a
    full scan), YK_ROOT_K=5 (the walks outrun the kept order and root_scan returns -1) and YK_NODE_SUMMARY=0 (a
    node's first pick is a full scan over unvisited edges only).  Equal records and counters; the modes differ
    in the entries they read."""
    _, E, _ = Y
    for k in ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY"):
        monkeypatch.delenv(k, raising=False)
    base = {"hash": fixed_run,
            "net": _run(E, 8, 30, 2026, 300, net=net, fpu_reduction=0.25, fpu_root_reduction=0.1)}
    assert base["net"][1]["fpu_unvisited_picks"] > 0 and base["net"][1]["fpu_picks"] > base["net"][1]["fpu_unvisited_picks"]
    path = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY")}
    p = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(path)
    for tag in ("full", "k5", "nosum"):
        for case, (r0, s0) in base.items():
            for f in FIELDS:
                assert np.array_equal(got["%s_%s_%s" % (tag, case, f)], r0[f]), (tag, case, f)
            c = got["%s_%s_counters" % (tag, case)]
            assert [int(x) for x in c[:4]] == [s0[k] for k in COUNTERS + ("expansions", "path_edges")], (tag, case)
            assert int(c[4]) != s0["scanned"], (tag, case)  # the other path did run: it read other entries
    assert int(got["full_net_counters"][4]) > base["net"][1]["scanned"]  # (full scans read every entry every time)


# ------------------------------------------------------------------ 4. with the other search features
K = 2.0


def test_noise_forced_playouts_pruning_and_fpu_compose(Y):
    """Root noise (0.3, 0.25), forced playouts k = 2 with pruning and the rule together against the composed
    reference: the sums read the noised P at a noised root, a forced edge's +inf beats every fq + x."""
    _, E, _ = Y
    rec, st, (before, after) = _run(E, 3, SIMS, SEED, BASE, cpuct=CPUCT, priors=True, record_predictions=True,
                                    forced_playouts_k=K, fpu_reduction=RED, **NOISE)
    tot = dict.fromkeys(("forced_picks", "pruned_visits") + COUNTERS, 0)
    for e in range(3):
        g = FR.play_episode(SEED, BASE + e, SIMS, r=RED, k=K, cpuct=CPUCT, root_prior=_injector(before, after, e))
        assert g["forced_picks"] >= 1 and g["pruned_visits"] >= 1 and g["unv_wins"][0] >= 1 and g["vis_wins"][0] >= 1, e
        R.assert_game_equals_records(g, rec, e)
        for k in tot:
            tot[k] += g[k]
    assert {k: st[k] for k in tot} == tot


SIMS4, FAST4, PROB4 = 30, 4, 0.4  # (test_gpu_playout_cap.py's schedule at (2026, 300): 28 fast moves)


def test_fast_and_full_moves_are_both_searched_under_fpu(Y):
    _, E, _ = Y
    full = PR.schedule(SEED, BASE, PROB4, 48)
    assert full.any() and (~full).any()
    cap = dict(playout_fast_sims=FAST4, playout_full_prob=PROB4)
    rec, st = _run(E, 3, SIMS4, SEED, BASE, cpuct=CPUCT, fpu_reduction=RED, **cap)
    picks = unv = 0
    for e in range(3):
        g = FR.play_episode(SEED, BASE + e, SIMS4, r=RED, cpuct=CPUCT, full=full, fast_sims=FAST4)
        R.assert_game_equals_records(g, rec, e)
        picks += g["fpu_picks"]
        unv += g["fpu_unvisited_picks"]
    assert (st["fpu_unvisited_picks"], st["fpu_picks"], st["fast_moves"]) == (unv, picks, int((~full).sum()))
    # every move fast: the rule still decides picks, and the games are not the plain engine's under the same cap
    none = dict(playout_fast_sims=FAST4, playout_full_prob=0.0)
    r1, s1 = _run(E, 3, SIMS4, SEED, BASE, cpuct=CPUCT, fpu_reduction=RED, **none)
    r0, s0 = _run(E, 3, SIMS4, SEED, BASE, cpuct=CPUCT, **none)
    assert s1["fast_moves"] == 48 and s1["fpu_picks"] > 0 and s0["fpu_picks"] == 0
    assert not np.array_equal(r1["visits"], r0["visits"])


# ------------------------------------------------------------------ 5. external roots, the plugin, the arenas
def test_mcts_search_of_external_roots(Y, fixed_ref):
    """yk_mcts_search on fresh trees from four positions of the fixed case's first game (a bid root, score roots,
    early and late), each on its own stream, with a root reduction of its own."""
    _, E, _ = Y
    from yacht_amd import kernels as Kn
    from yacht_amd._lib import call, stream_ptr
    moves = (0, 5, 20, 40)
    roots = fixed_ref[0][0]["states"][list(moves)]
    n, sims, seed = len(moves), 24, 77
    want = [FR.search_counts(seed, 900 + i, roots[i], sims, CPUCT, r=RED, r_root=0.5) for i in range(n)]
    eng = E.SelfPlayEngine(n, sims, CPUCT, prior="hash", max_moves=1, fpu_reduction=RED, fpu_root_reduction=0.5)
    call("yk_mcts_reset", eng.handle)
    dev = Kn.states_to_device(np.ascontiguousarray(roots))
    env = torch.arange(900, 900 + n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros((n, Kn.ACTION_SIZE), dtype=torch.int32, device="cuda")
    call("yk_mcts_search", eng.handle, dev.data_ptr(), seed, env.data_ptr(), ctr.data_ptr(), sims, counts.data_ptr(),
         stream_ptr())
    st = eng.stats()
    eng.close()
    got = counts.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], want[i][0]), i
        assert int(ctr[i].item()) == want[i][1], i
    assert st["errors"] == 0
    assert (st["fpu_unvisited_picks"], st["fpu_picks"]) == (sum(w[2].fpu_unvisited_picks for w in want),
                                                            sum(w[2].fpu_picks for w in want))
    assert st["fpu_picks"] > st["fpu_unvisited_picks"] > 0


def test_mcts_plugin_passes_the_knob(Y):
    Ymod, _, N = Y
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.utils import dotdict
    args = dotdict(numMCTSSims=24, cpuct=CPUCT, fpuReduction=RED, fpuRootReduction=0.5)
    game = YachtGame(seed=77, env_id=910)
    canon = game.getCanonicalForm(game.getInitBoard(), 1)
    c0 = game.rng.ctr
    mcts = MCTS(game, N.HashPriorNet(game), args)
    got = mcts.search_counts(canon)
    assert (mcts._engine.fpu_reduction, mcts._engine.fpu_root_reduction) == (RED, 0.5)
    want, ctr, ref = FR.search_counts(77, 910, np.asarray(Ymod.pack(canon), dtype=np.uint64).reshape(8), 24, CPUCT, r=RED,
                                      r_root=0.5, ctr=c0)
    assert np.array_equal(np.asarray(got, dtype=np.int32), want) and game.rng.ctr == ctr
    assert ref.fpu_picks > 0
    plain = MCTS(YachtGame(seed=77, env_id=910), N.HashPriorNet(game), dotdict(numMCTSSims=24, cpuct=CPUCT))
    plain._eng()
    assert (plain._engine.fpu_reduction, plain._engine.fpu_root_reduction) == (None, None)


def _check_arena(last, games, max_moves):
    for i, g in enumerate(games):
        m = len(g["actions"])
        assert int(last["n_moves"][i]) == m, i
        assert last["actions"][i, :m].tolist() == g["actions"], i
        assert float(last["result"][i]) == g["result"], i
        assert np.array_equal(last["totals"][i], g["totals"]), i
        assert np.array_equal(last["final"][i], g["final"]) and int(last["ctr"][i]) == g["ctr"], i


def test_both_arenas_search_under_fpu(Y):
    """A 2-game MCTSArena (the agent against the random player) and a 2-game dual-tree GatingArena (both seats
    search, each in its own tree) against Arena.playGame in plain Python over the reference's searches."""
    _, _, N = Y
    from yacht_amd.arena import GatingArena, MCTSArena
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    sims = 12
    args = dotdict(numMCTSSims=sims, cpuct=CPUCT, fpuReduction=RED, arenaCompare=2)
    game = YachtGame(seed=21, env_id=500)
    arena = MCTSArena(game, N.HashPriorNet(game), args)
    arena.playGames(2)
    want = [FR.arena_game(21, 500 + i, seat, sims, CPUCT, r=RED) for i, seat in enumerate((1, -1))]
    assert sum(g["fpu_picks"] for g in want) > 0
    _check_arena(arena.last, want, 64)
    plain = [FR.arena_game(21, 500 + i, seat, sims, CPUCT) for i, seat in enumerate((1, -1))]
    assert [g["actions"] for g in plain] != [g["actions"] for g in want]  # (the knob changes these games)
    gate = GatingArena(game, N.HashPriorNet(game), N.HashPriorNet(game), args)
    gate.playGames(2, env_base=600)
    want = [FR.arena_game(21, 600 + i, seat, sims, CPUCT, r=RED, opponent="mcts", max_moves=48)
            for i, seat in enumerate((1, -1))]
    _check_arena(gate.last, want, 48)


# ------------------------------------------------------------------ 6. yk_fpu_pick
SIZES = (1, 4, 63, 64, 65, 255, 256, 257, 3024)


def _tie_row(r, unvisited_first):
    """An exact tie fq + x == u at Ns = 4, cpuct 1 (sq = sqe = 2 in float32): visited A (Q 0.75, N 2, P 0: u = 0.75),
    visited B (Q 0.25, N 2, P 1/4: u = 5/12, it carries the tried mass: sqrt = 1/2) - W / Ns = 1/2, fq = 1/2 - r / 2 -
    and an unvisited edge with x = 2 P = 1/4 + r / 2."""
    pu = np.float32((0.25 + r / 2) / 2)
    assert float(pu) * 2 == 0.25 + r / 2  # (exact for the r of the test)
    vis = [(0.0, 2, 0.75), (0.25, 2, 0.25)]
    unv = [(float(pu), 0, 0.0)]
    rows = unv + vis if unvisited_first else vis + unv
    return [np.array([x[i] for x in rows]) for i in range(3)] + [4]


def _pick_rows(r):
    """Nodes as one CSR (p, counts, q per entry; ns per row), the rule's cases by hand."""
    rng = np.random.default_rng(2027)
    rows = []
    for L in SIZES:
        for layout in ("mixed", "all", "none", "one"):
            p = rng.dirichlet(np.full(L, 0.3)).astype(np.float32) if L > 1 else np.ones(1, dtype=np.float32)
            cnt = np.zeros(L, dtype=np.int32)
            if layout == "all":
                cnt[:] = rng.integers(1, 40, L)
            elif layout == "one":
                cnt[rng.integers(0, L)] = int(rng.integers(1, 40))
            elif layout == "mixed":
                k = rng.choice(L, max(L // 3, 1), replace=False)
                cnt[k] = rng.integers(1, 40, len(k))
            q = rng.choice([-1.0, 0.0, 1.0, 0.125, -0.37, float(np.float32(0.3))], L)
            p[rng.integers(0, L, max(L // 16, 1))] = 0.0                     # P = 0
            p[rng.integers(0, L, max(L // 16, 1))] = np.float32(2.0 ** -41)  # below 2^-40: adds nothing to Mi
            ns = int(cnt.sum()) + (int(rng.integers(0, 3)) if cnt.any() else int(rng.integers(0, 2)) * 7)
            rows.append([p, cnt, q, ns])
    # bands of equal x that cross a 64-lane and a 256-entry boundary (and the four entries of a lane), the best of
    # the row: the lowest index wins.  The two visited edges carry no prior mass (fq is their mean and the band
    # wins for every r) or a little (the band wins at r = 0 only)
    for L, lo, hi in ((300, 60, 70), (300, 250, 262), (3024, 1020, 1030), (3024, 2000, 2600)):
        for q0, pv in ((-1.0, 0.0), (1.0, 2.0 ** -12)):
            p = np.full(L, 2.0 ** -12, dtype=np.float32)
            p[lo:hi] = np.float32(2.0 ** -9)
            p[[5, hi + 3]] = np.float32(pv)
            cnt = np.zeros(L, dtype=np.int32)
            cnt[[5, hi + 3]] = (3, 2)
            q = np.zeros(L)
            q[[5, hi + 3]] = q0
            rows.append([p, cnt, q, 5])
    # bands of equal u among the visited edges across the same boundaries
    for L, lo, hi in ((300, 250, 262), (300, 60, 70)):
        p = np.full(L, 2.0 ** -10, dtype=np.float32)
        cnt = np.zeros(L, dtype=np.int32)
        cnt[lo:hi] = 2
        q = np.full(L, 0.5)
        rows.append([p, cnt, q, 2 * (hi - lo)])
    rows.append(_tie_row(r, True))
    rows.append(_tie_row(r, False))
    # N up to 65535 and Q at the ends of its range: |W| reaches Ns 2^32
    for q0 in (-1.0, 1.0):
        rows.append([np.array([0.5, 0.25, 0.25], dtype=np.float32), np.array([65535, 0, 1], dtype=np.int32),
                     np.array([q0, 0.0, -q0]), 65536])
    rows.append([np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32), np.zeros(0), 0])  # an empty row
    indptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in rows])]).astype(np.int64)
    return (indptr, np.concatenate([x[0] for x in rows]).astype(np.float32),
            np.concatenate([x[1] for x in rows]).astype(np.int32), np.concatenate([x[2] for x in rows]).astype(np.float64),
            np.array([x[3] for x in rows], dtype=np.int32))


@pytest.mark.parametrize("r", [0.0, 0.25, 4.0])
def test_fpu_pick_is_the_numpy_reference(Y, r):
    from yacht_amd import kernels as Kn
    rows = _pick_rows(r)
    indptr, p, counts, q, ns = rows
    dev = [torch.from_numpy(a).cuda() for a in rows]
    pick, unv = Kn.fpu_pick(*dev, 1.0, r)
    assert pick.dtype == torch.int32 and unv.dtype == torch.int32 and pick.shape == unv.shape == (len(ns),)
    want_pick, want_unv = FR.fpu_pick(indptr, p, counts, q, ns, 1.0, r)
    got_pick, got_unv = pick.cpu().numpy(), unv.cpu().numpy()
    bad = np.flatnonzero((got_pick != want_pick) | (got_unv != want_unv))
    assert len(bad) == 0, [(int(i), int(indptr[i + 1] - indptr[i]), int(got_pick[i]), int(want_pick[i])) for i in bad[:8]]
    # the rows do exercise the rule: both winners where it decides, and the hand-made ties are exact
    both = np.array([(counts[indptr[i]:indptr[i + 1]] > 0).any() and (counts[indptr[i]:indptr[i + 1]] <= 0).any()
                     and ns[i] > 0 for i in range(len(ns))])
    assert (want_unv[both] == 1).any() and (want_unv[both] == 0).any()
    n = len(ns)
    assert want_pick[n - 5] == 0 and want_unv[n - 5] == 1 and want_pick[n - 4] == 0 and want_unv[n - 4] == 0  # the ties
    for row, first in ((n - 5, True), (n - 4, False)):
        a = int(indptr[row])
        vis = a + (1 if first else 0)
        terms = [(2, 0.75, np.float32(0.0)), (2, 0.25, np.float32(0.25))]
        fq = FR.fpu_value(sum(FR.w_term(N, Q) for N, Q, _ in terms), sum(FR.m_term(x) for _, _, x in terms), 4, r)
        x = (np.float32(1.0) * p[a if first else a + 2]) * np.float32(math.sqrt(4 + 1e-8))
        assert fq + x == np.float32(0.75) and q[vis] == 0.75
    assert want_pick[n - 1] == -1
    p2, u2 = Kn.fpu_pick(*dev, 1.0, r)  # equal inputs, equal bits
    assert torch.equal(p2, pick) and torch.equal(u2, unv)
    assert np.array_equal(dev[2].cpu().numpy(), counts)  # the input is not modified


def test_fpu_pick_error_returns(Y):
    from yacht_amd import kernels as Kn
    from yacht_amd._lib import YK_ERR_ARG, YK_ERR_RANGE, stream_ptr
    lib = __import__("yacht_amd").lib()
    rows = _pick_rows(0.25)
    dev = [torch.from_numpy(a).cuda() for a in rows]
    n = len(rows[4])
    pick = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    unv = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def rc(indptr, r=0.25, n=n, c=1.0):
        return lib.yk_fpu_pick(indptr.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                               dev[4].data_ptr(), n, c, r, pick.data_ptr(), unv.data_ptr(), stream_ptr())

    for bad in (-1.0, float("nan"), float("inf")):
        assert rc(dev[0], r=bad) == YK_ERR_ARG
    assert rc(dev[0], n=-1) == YK_ERR_ARG and rc(dev[0], c=float("nan")) == YK_ERR_ARG
    down = dev[0].clone()
    down[3] = down[2] - 1  # decreases
    assert rc(down) == YK_ERR_RANGE
    neg = dev[0].clone()
    neg[0] = -1
    assert rc(neg) == YK_ERR_RANGE
    assert (pick == -7).all() and (unv == -7).all()  # nothing was written
    with pytest.raises(ValueError, match="indptr"):
        Kn.fpu_pick(down, *dev[1:], 1.0, 0.25)
    with pytest.raises(TypeError):
        Kn.fpu_pick(dev[0].to(torch.int32), *dev[1:], 1.0, 0.25)
    # no rows
    e = Kn.fpu_pick(torch.zeros(1, dtype=torch.int64, device="cuda"), *(d[:0] for d in dev[1:]), 1.0, 0.25)
    assert e[0].numel() == 0 and e[1].numel() == 0
    assert rc(dev[0]) == 0


# ------------------------------------------------------------------ 7. the Coach
ARGS = dict(numIters=2, numEps=4, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
            arenaCompare=2, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=1,
            batch_size=48, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3, amp=False)


def test_coach_iteration_carries_the_knobs(Y, monkeypatch, tmp_path):
    """Two tiny iterations (the second one reanalyses the first) with the knobs set: every engine built for the
    Coach - self-play, the reanalysis, the gate - carries them, and the self-play report has the two counters."""
    _, E, _ = Y
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    ck = str(tmp_path / "ck")
    torch.manual_seed(5)
    net = NNetWrapper(YachtGame(seed=21, env_id=500), dotdict(
        ARGS, checkpoint=ck, load_folder_file=(ck, "best.pth.tar"), fpuReduction=RED, fpuRootReduction=0.1,
        reanalyseFraction=0.5))
    coach = Coach(net.game, net, net.args)
    made = []
    init = E.SelfPlayEngine.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append((kw.get("max_moves"), bool(kw.get("dual_trees")), self.fpu_reduction, self.fpu_root_reduction))

    monkeypatch.setattr(E.SelfPlayEngine, "__init__", spy)
    coach.learn()
    kinds = {(m, d) for m, d, _, _ in made}
    assert kinds == {(48, False), (1, False), (48, True)}  # self-play, the reanalysis, the gate
    assert all((r, rr) == (RED, 0.1) for _, _, r, rr in made), made
    assert set(coach.last_selfplay) == {"searched", "kept", "sims", "fpu_unvisited_picks", "fpu_picks"}
    assert coach.last_selfplay["fpu_picks"] > 0
    assert coach.last_reanalysis and coach.last_reanalysis[0]["reanalysed"] > 0
