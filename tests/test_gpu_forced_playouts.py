"""Forced playouts and policy target pruning on the GPU: opt-in, at the roots of
self-play's full moves.

* off is off: unset or k = 0, every record and counter is the default engine's;
* on, every game equals tests/forced_ref.play_episode bit for bit - the plain-Python Coach / MCTS of
  noise_ref with the forced test in the root's selection and the pruning after the move - with and without the
  pruning, under root noise, on every path the root's pick can take, and with the playout cap (fast moves are
  neither forced nor pruned);
* yk_policy_prune against the numpy restatement, exactly; the Coach's two paths."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import forced_ref as F
import noise_ref as R
import playout_ref as PR
from conftest import REPO
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
ALPHA, EPS = 0.3, 0.25  # test_gpu_root_noise.py's
NOISE = dict(dirichlet_alpha=ALPHA, dirichlet_eps=EPS)
K = 2.0
TT = 15


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


def _run(E, n, sims, seed, base, net=None, priors=False, setter=None, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, TT, net=net, prior="hash" if net is None else "net", max_moves=48, **kw)
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
    """The move's recorded P' handed to the reference at the top of getActionProb, after checking that the Ps it
    replaces is the recorded P (as test_search_under_noise_is_the_reference_search)."""
    def inject(move, P):
        assert full is None or full[move]
        assert np.array_equal(P.view(np.uint32), before[e, move].view(np.uint32)), (e, move)
        return after[e, move].copy()
    return inject


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("prior,n,groups", [("hash", 48, 1), ("hash", 48, 2), ("net", 6, 1), ("net", 6, 2)])
def test_off_is_off(Y, net, prior, n, groups):
    """The shapes of test_gpu_playout_cap.py's test_off_is_off.  Unset is the default engine; k = 0 through the
    constructor (which then makes no call) and through the setter itself, with either prune flag."""
    _, E, _ = Y
    from yacht_amd._lib import call
    nt = net if prior == "net" else None
    r0, s0 = _run(E, n, 12, 707, 900, net=nt, groups=groups)
    assert s0["forced_picks"] == 0 and s0["pruned_visits"] == 0
    cases = [dict(forced_playouts_k=0.0), dict(forced_playouts_k=0, forced_prune=False),
             dict(setter=lambda eng: call("yk_engine_set_forced_playouts", eng.handle, 0.0, 1)),
             dict(setter=lambda eng: call("yk_engine_set_forced_playouts", eng.handle, 0.0, 0))]
    for kw in cases:
        r1, s1 = _run(E, n, 12, 707, 900, net=nt, groups=groups, **kw)
        _same(r1, r0)
        assert s1 == s0


def test_setter_rejects_bad_arguments_and_leaves_the_engine(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_ARG, YkError, call
    lib = __import__("yacht_amd").lib()
    for kw in (dict(forced_playouts_k=-1.0), dict(forced_playouts_k=float("nan")), dict(forced_playouts_k=float("inf"))):
        with pytest.raises(YkError) as ei:
            E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, **kw)
        assert ei.value.code == YK_ERR_ARG, kw
    r0, s0 = _run(E, 2, 12, 5, 0)
    eng = E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48)
    for k, prune in ((-1.0, 1), (-1e-300, 1), (float("nan"), 1), (float("inf"), 0), (2.0, 2), (2.0, -1), (0.0, 7)):
        assert lib.yk_engine_set_forced_playouts(C.c_void_p(eng.handle), k, prune) == YK_ERR_ARG, (k, prune)
    eng.run(5, 0)  # still off
    _same(eng.records(), r0)
    assert eng.stats() == s0
    call("yk_engine_set_forced_playouts", eng.handle, 1e-300, 0)  # the bounds themselves are legal
    call("yk_engine_set_forced_playouts", eng.handle, 1e300, 1)
    eng.close()


# ------------------------------------------------------------------ 2. bit for bit
# 3 games, hash prior, 30 simulations, root noise, k = 2.  Chosen on the CPU with the restated sampler's noise
# (noise_ref.eta; the test itself hands the reference the engine's recorded P'): per game (seed 11, envs 3, 4, 5)
# forced picks 44 / 52 / 42, visits pruned 96 / 112 / 91, edges pruned to 0: 44 / 50 / 39, edges pruned but left
# above 1: 11 / 16 / 14.
SEED2, BASE2, SIMS2 = 11, 3, 30


@pytest.fixture(scope="module")
def forced_games(Y):
    """The engine's records, counters and recorded root priors, with and without the pruning."""
    _, E, _ = Y
    return {prune: _run(E, 3, SIMS2, SEED2, BASE2, priors=True, record_predictions=True, forced_playouts_k=K,
                        forced_prune=prune, **NOISE) for prune in (True, False)}


@pytest.mark.parametrize("prune", [True, False])
def test_forced_games_are_the_reference_games(forced_games, prune):
    rec, st, (before, after) = forced_games[prune]
    picks = cut = 0
    to_zero = partly = 0
    for e in range(3):
        g = F.play_episode(SEED2, BASE2 + e, SIMS2, K, prune=prune, root_prior=_injector(before, after, e))
        # the conditions the case was chosen for, on the reference alone
        assert g["forced_picks"] >= 1, e
        for raw, kept in zip(g["raw"], g["kept"]):
            to_zero += sum(1 for a in raw if a not in kept)
            partly += sum(1 for a in kept if 1 < kept[a] < raw[a])
            assert prune or kept == raw
        R.assert_game_equals_records(g, rec, e)
        picks += g["forced_picks"]
        cut += g["pruned_visits"]
    print(f"prune {prune}: forced picks {picks}, visits pruned {cut}, edges to 0: {to_zero}, partly: {partly}")
    if prune:
        assert to_zero >= 1 and partly >= 1
    else:
        assert cut == 0
    assert (st["forced_picks"], st["pruned_visits"]) == (picks, cut)
    # info[4] stays the raw Ns: with the pruning on, some move's recorded counts sum to less
    off = rec["visits_off"]
    sums = np.array([[int(rec["visits"][int(off[e * 48 + m]):int(off[e * 48 + m + 1]), 1].sum()) for m in range(48)]
                     for e in range(3)])
    assert (sums <= rec["info"][:, :48, 4]).all()
    assert int((rec["info"][:, :48, 4] - sums).sum()) == cut


def test_pruning_changes_the_record_only_until_the_first_other_draw(forced_games):
    """Forcing alone and forcing with pruning search the same tree until a pruned move draws another action: move
    0's raw search is the same, so its root Ns and its stream counters agree, and its counts differ only by the
    pruning."""
    (r1, _, _), (r0, _, _) = forced_games[True], forced_games[False]
    assert np.array_equal(r1["info"][:, 0, 4], r0["info"][:, 0, 4])
    assert np.array_equal(r1["ctr"][:, 0, 0], r0["ctr"][:, 0, 0])
    assert not np.array_equal(r1["visits"], r0["visits"])


# ------------------------------------------------------------------ 3. every root path
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "nypc-yacht-auction_amd"))
from oracle import spec
from yacht_amd import engine as E, nnet as N
net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6)
out = {}
for tag, env in (("full", {"YK_ROOT_SCAN": "0"}), ("k5", {"YK_ROOT_K": "5"})):
    for k in ("YK_ROOT_SCAN", "YK_ROOT_K"):
        os.environ.pop(k, None)
    os.environ.update(env)  # (read when the engine is made)
    eng = E.SelfPlayEngine(16, 30, 1.5, 15, net=net, max_moves=48, dirichlet_alpha=0.3, dirichlet_eps=0.25,
                           forced_playouts_k=2.0)
    eng.run(707, 900)
    st, rec = eng.stats(), eng.records()
    eng.close()
    assert st["errors"] == 0, st
    for f in ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits"):
        out[tag + "_" + f] = rec[f]
    out[tag + "_counters"] = np.array([st[c] for c in ("forced_picks", "pruned_visits", "expansions", "path_edges",
                                                       "scanned")], dtype=np.int64)
np.savez(sys.argv[2], **out)
"""


def test_every_root_path_forces_alike(Y, net, tmp_path, monkeypatch):
    """16 net-prior games x 30 sims, noise, k = 2: the default engine (the sorted root order with its visited
    list; bid roots, at most 256 entries, by full scans; every move's first simulation by a full scan) against,
    in a fresh child process, YK_ROOT_SCAN=0 (every root pick a full scan - the code a visited list past RV_CAP
    = 1024 entries falls back to, which no quick test reaches) and YK_ROOT_K=5 (a kept order of 5 entries: the
    walks outrun it and root_scan returns -1, the fallback a score root's 3024 entries against RO_K = 512 would
    need hundreds of visited edges for).  Equal records and counters; the modes differ in the entries they read."""
    _, E, _ = Y
    for k in ("YK_ROOT_SCAN", "YK_ROOT_K"):
        monkeypatch.delenv(k, raising=False)
    r0, s0 = _run(E, 16, 30, 707, 900, net=net, forced_playouts_k=K, **NOISE)
    assert s0["forced_picks"] > 0 and s0["pruned_visits"] > 0
    assert (np.diff(r0["visits_off"])[:16 * 48].reshape(16, 48) == r0["info"][:, :, 5]).all()
    path = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("YK_ROOT_SCAN", "YK_ROOT_K")}
    p = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(path)
    for tag in ("full", "k5"):
        for f in FIELDS:
            assert np.array_equal(got[tag + "_" + f], r0[f]), (tag, f)
        c = got[tag + "_counters"]
        assert [int(x) for x in c[:4]] == [s0[k] for k in ("forced_picks", "pruned_visits", "expansions", "path_edges")]
        assert int(c[4]) != s0["scanned"], tag  # the other path did run: it read other entries
    assert int(got["full_counters"][4]) > s0["scanned"]  # (full scans read every entry every time)


# ------------------------------------------------------------------ 4. with the playout cap
SEED4, BASE4, SIMS4, FAST4, PROB4 = 2026, 300, 30, 4, 0.4  # (test_gpu_playout_cap.py's schedule, 28 fast moves)


def test_fast_moves_are_neither_forced_nor_pruned(Y):
    """3 games under the fixed schedule with noise and k = 2 against the reference loop with cap[m] simulations
    per move: a fast move runs the unforced search of its cap and records its raw counts, a full move is forced
    and pruned.  (On the CPU, with the restated sampler: forced picks 11 / 12 / 5, visits pruned 22 / 18 / 15.)"""
    _, E, _ = Y
    full = PR.schedule(SEED4, BASE4, PROB4, 48)
    assert full.any() and (~full).any()
    cap = dict(playout_fast_sims=FAST4, playout_full_prob=PROB4)
    rec, st, (before, after) = _run(E, 3, SIMS4, SEED4, BASE4, priors=True, record_predictions=True,
                                    forced_playouts_k=K, **cap, **NOISE)
    picks = cut = 0
    for e in range(3):
        g = F.play_episode(SEED4, BASE4 + e, SIMS4, K, root_prior=_injector(before, after, e, full), full=full,
                           fast_sims=FAST4)
        assert g["forced_picks"] >= 1, e
        for m in np.nonzero(~full)[0]:
            assert g["kept"][m] == g["raw"][m]
        R.assert_game_equals_records(g, rec, e)
        picks += g["forced_picks"]
        cut += g["pruned_visits"]
    assert cut >= 1
    assert (st["forced_picks"], st["pruned_visits"], st["fast_moves"]) == (picks, cut, int((~full).sum()))
    # every move fast: nothing is forced or pruned, and the games are the unforced engine's under the same cap
    none = dict(playout_fast_sims=FAST4, playout_full_prob=0.0)
    r1, s1 = _run(E, 3, SIMS4, SEED4, BASE4, forced_playouts_k=K, **none, **NOISE)
    r0, s0 = _run(E, 3, SIMS4, SEED4, BASE4, **none, **NOISE)
    assert s1["fast_moves"] == 48 and s1["forced_picks"] == 0 and s1["pruned_visits"] == 0
    _same(r1, r0)
    assert s1 == s0


def test_arena_is_never_forced(Y):
    _, E, _ = Y
    seat = np.array([1, -1, 1, -1], dtype=np.int32)
    out = []
    for kw in ({}, dict(forced_playouts_k=K)):
        eng = E.SelfPlayEngine(4, 30, 1.5, TT, prior="hash", max_moves=48, **kw)
        eng.arena(seat, 21, 500, agent="mcts", opponent="random")
        st = eng.stats()
        assert st["errors"] == 0 and st["forced_picks"] == 0 and st["pruned_visits"] == 0
        out.append((eng.arena_results(), eng.records()))
        eng.close()
    for k, v in out[0][0].items():
        assert np.array_equal(out[1][0][k], v), k
    _same(out[1][1], out[0][1])


# ------------------------------------------------------------------ 5. yk_policy_prune
def _rows():
    """Crafted rows as one CSR: 1 edge; 63, 64, 65 and 3226 edges (the wave-stride boundaries); all-equal counts;
    Q at -1, 0, 1 and equal to the best child's; Ns whose square root is inexact; entries without visits."""
    rng = np.random.default_rng(2024)
    rows = []
    for L in (1, 63, 64, 65, 3226, 2, 7, 130):
        cnt = rng.integers(1, 40, L).astype(np.int32)
        if L > 4:
            cnt[rng.integers(0, L, L // 5)] = 0  # no visited edge here
            cnt[rng.integers(0, L, 3)] = 40      # the largest count more than once: the tie rule
        p = rng.dirichlet(np.full(L, 0.3)).astype(np.float32)
        q = rng.choice([-1.0, 0.0, 1.0, 0.125, -0.37], L)
        best = int(np.flatnonzero(cnt == cnt.max())[0])
        q[rng.integers(0, L, max(L // 8, 1))] = q[best]  # Q equal to the best child's
        rows.append((np.arange(L, dtype=np.int32) * (3226 // L), cnt, q, p, int(cnt.sum()) + int(rng.integers(0, 3))))
    L = 9  # all-equal counts and all-equal Q: the lowest column is c*
    rows.append((np.arange(L, dtype=np.int32) + 100, np.full(L, 5, dtype=np.int32), np.zeros(L),
                 np.full(L, 1.0 / L, dtype=np.float32), 45))
    rows.append((np.array([5, 2], dtype=np.int32), np.array([5, 5], dtype=np.int32), np.array([-0.9, 0.0]),
                 np.array([0.5, 0.5], dtype=np.float32), 10))  # columns that descend: c* is column 2, the second entry
    rows.append((np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0, dtype=np.float32), 0))
    rows.append((np.array([4, 9], dtype=np.int32), np.array([97, 3], dtype=np.int32), np.array([0.5, -1.0]),
                 np.array([0.9, 0.03125], dtype=np.float32), 100))  # 3 -> 1 -> 0
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    cat = [np.concatenate([r[i] for r in rows]) for i in range(4)]
    ns = np.array([r[4] for r in rows], dtype=np.int32)
    assert any(math_sqrt_inexact(int(x)) for x in ns)
    return indptr, cat[0].astype(np.int32), cat[1].astype(np.int32), cat[2].astype(np.float64), cat[3].astype(np.float32), ns


def math_sqrt_inexact(n):
    import math
    return math.isqrt(n) ** 2 != n


@pytest.fixture(scope="module")
def prune_rows(Y):
    return _rows()


@pytest.mark.parametrize("k", [0.0, 2.0, 0.5, 1e6])  # (1e6: f exceeds every N - only the PUCT test stops the loop)
def test_policy_prune_is_the_numpy_reference(Y, prune_rows, k):
    from yacht_amd import replay
    indptr, cols, counts, q, p, ns = prune_rows
    dev = [torch.from_numpy(a).cuda() for a in prune_rows]
    got = replay.policy_prune(*dev, k, 1.5)
    assert got.dtype == torch.int32 and got.shape == (len(counts),)
    want = F.policy_prune(indptr, cols, counts, q, p, ns, k, 1.5)
    assert np.array_equal(got.cpu().numpy(), want)
    if k == 0.0:
        assert np.array_equal(want, counts)
    else:  # the rows do exercise the rule: counts cut, edges dropped, and edges left between
        assert (want < counts).any() and ((want == 0) & (counts > 0)).any() and ((want > 1) & (want < counts)).any()
        for r in range(len(ns)):  # c* keeps its count
            a, b = int(indptr[r]), int(indptr[r + 1])
            if b > a and counts[a:b].max() > 0:
                top = np.flatnonzero(counts[a:b] == counts[a:b].max())
                star = a + top[np.argmin(cols[a:b][top])]
                assert want[star] == counts[star]
    assert np.array_equal(replay.policy_prune(*dev, k, 1.5).cpu().numpy(), want)  # equal inputs, equal bits
    assert np.array_equal(dev[2].cpu().numpy(), counts)  # the input is not modified


def test_policy_prune_error_returns(Y, prune_rows):
    from yacht_amd import replay
    from yacht_amd._lib import YK_ERR_ARG, YK_ERR_RANGE, stream_ptr
    lib = __import__("yacht_amd").lib()
    dev = [torch.from_numpy(a).cuda() for a in prune_rows]
    n = len(prune_rows[5])
    out = torch.full_like(dev[2], -7)

    def rc(indptr, k=2.0, n=n):
        return lib.yk_policy_prune(indptr.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                   dev[4].data_ptr(), dev[5].data_ptr(), n, k, 1.5, out.data_ptr(), stream_ptr())

    for bad in (-1.0, float("nan"), float("inf")):
        assert rc(dev[0], k=bad) == YK_ERR_ARG
    assert rc(dev[0], n=-1) == YK_ERR_ARG
    down = dev[0].clone()
    down[3] = down[2] - 1  # decreases
    assert rc(down) == YK_ERR_RANGE
    neg = dev[0].clone()
    neg[0] = -1
    assert rc(neg) == YK_ERR_RANGE
    assert (out == -7).all()  # nothing was written
    with pytest.raises(ValueError, match="indptr"):
        replay.policy_prune(down, *dev[1:], 2.0, 1.5)
    with pytest.raises(TypeError):
        replay.policy_prune(dev[0].to(torch.int32), *dev[1:], 2.0, 1.5)
    # no rows, and rows without entries
    e = replay.policy_prune(torch.zeros(1, dtype=torch.int64, device="cuda"), *(d[:0] for d in dev[1:]), 2.0, 1.5)
    assert e.numel() == 0
    assert rc(dev[0]) == 0


# ------------------------------------------------------------------ 6. the Coach
def test_coach_trains_on_the_pruned_counts(Y):
    Ymod, E, N = Y
    from yacht_amd.coach import Coach, examples_from_records
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    seed, env, sims = SEED2, BASE2, SIMS2
    args = dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=TT, dirichletAlpha=ALPHA, dirichletEpsilon=EPS,
                   forcedPlayoutsK=K)
    coach = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(), args)
    knobs = dict(forced_playouts_k=K, **NOISE)
    # the tuple path: streams env .. env + 2
    rec, st = _run(E, 3, sims, seed, env, **knobs)
    assert st["pruned_visits"] > 0
    raw, _ = _run(E, 3, sims, seed, env, forced_playouts_k=K, forced_prune=False, **NOISE)

    def flat(games):
        return [([int(x) for x in Ymod.pack(s)], pi, v) for g in games for s, pi, v in g]

    got = flat(coach.executeEpisodes(3))
    assert got == flat(examples_from_records(rec, 3))
    assert got != flat(examples_from_records(raw, 3))
    # the device path: the next batch starts at stream env + 3
    shard = coach.selfPlayExamples(4)
    rec2, st2 = _run(E, 4, sims, seed, env + 3, **knobs)
    assert st2["forced_picks"] > 0 and st2["pruned_visits"] > 0
    assert coach.last_selfplay == dict(searched=4 * 48, kept=4 * 48, sims=48 * sims, forced_picks=st2["forced_picks"],
                                       pruned_visits=st2["pruned_visits"])
    assert np.array_equal(shard.states.cpu().numpy().view(np.uint64).reshape(-1, 8), rec2["states"][:, :48].reshape(-1, 8))
    P = {k: v.cpu().numpy() for k, v in shard.policies.items()}
    off, k = rec2["visits_off"], 0
    for e in range(4):
        for m in range(48):
            v = rec2["visits"][int(off[e * 48 + m]):int(off[e * 48 + m + 1])]
            a0, a1 = int(P["pi_indptr"][k]), int(P["pi_indptr"][k + 1])
            if rec2["info"][e, m, 0]:  # temp 1: the recorded (pruned) counts, normalised
                assert len(v) == rec2["info"][e, m, 5] and (v[:, 1] > 0).all()
                assert np.array_equal(P["pi_cols"][a0:a1], v[:, 0])
                assert np.array_equal(P["pi_vals"][a0:a1], v[:, 1].astype(np.float64) / float(v[:, 1].sum()))
            else:
                assert P["pi_cols"][a0:a1].tolist() == [int(rec2["info"][e, m, 2])] and P["pi_vals"][a0:a1].tolist() == [1.0]
            k += 1
    assert k == len(shard)
    # off: the report has no such keys
    plain = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(), dotdict(numMCTSSims=8, cpuct=1.5, tempThreshold=TT))
    plain.selfPlayExamples(2)
    assert set(plain.last_selfplay) == {"searched", "kept", "sims"}
