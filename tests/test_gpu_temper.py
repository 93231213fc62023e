"""The self-play temperatures on the GPU: off by default and then unobservable; the move
draw from N^(1/T) and the root prior P^(1/T) renormalised equal tests/temper_ref.py - the stand-alone entry points
on crafted rows, whole games bit for bit - on every root-scan path, whatever the grouping; the arenas, the plugin
and the reanalysis never apply them; the Coach passes them to self-play."""
import numpy as np
import pytest

import noise_ref as R
import temper_ref as T
from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
ALPHA, EPS = 0.3, 0.25
NOISE = dict(dirichlet_alpha=ALPHA, dirichlet_eps=EPS)
MOVE = dict(move_temperature=T.MOVE_SCHEDULE["final"], move_temperature_early=T.MOVE_SCHEDULE["early"],
            temperature_halflife=T.MOVE_SCHEDULE["halflife"])
ROOT = dict(root_policy_temperature=T.ROOT_SCHEDULE["final"], root_policy_temperature_early=T.ROOT_SCHEDULE["early"],
            temperature_halflife=T.ROOT_SCHEDULE["halflife"])
BOTH = dict(MOVE, **ROOT)  # (one halflife, 8, for both)
MT = T.schedule(n_moves=48, **T.MOVE_SCHEDULE)
RT = T.schedule(n_moves=48, **T.ROOT_SCHEDULE)


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


def _run(E, n, sims, prior, net, seed, base, priors=False, thr=15, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, thr, net=net if prior == "net" else None, prior=prior, max_moves=48, **kw)
    eng.run(seed, base)
    st = eng.stats()
    rec = eng.records()
    pri = eng.root_priors() if priors else None
    eng.close()
    assert st["errors"] == 0, st
    return (rec, st, pri) if priors else (rec, st)


def _same(r1, r0):
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to("cuda")


# ------------------------------------------------------------------ 0. the engine's tables and its setter
def test_engine_holds_the_host_tables_and_rejects_bad_schedules(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_ARG, lib
    eng = E.SelfPlayEngine(2, 2, 1.5, 15, prior="hash", max_moves=48, **BOTH)
    mt, rt = eng.temperatures()
    assert np.array_equal(mt.view(np.uint64), MT.view(np.uint64)) and np.array_equal(rt.view(np.uint64), RT.view(np.uint64))
    h = eng.handle
    nan, inf = float("nan"), float("inf")
    for a in ((0.04, 0.3, 0, 0, 8.0), (1.3, 101.0, 0, 0, 8.0), (0.0, 0.3, 0, 0, 8.0), (1.3, 0.0, 0, 0, 8.0),
              (nan, 0.3, 0, 0, 8.0), (0, 0, 0.2, 1.1, 8.0), (0, 0, 1.25, 10.5, 8.0), (0, 0, 0.0, 1.1, 8.0),
              (0, 0, 1.25, nan, 8.0), (1.3, 0.3, 0, 0, 0.0), (1.3, 0.3, 0, 0, -1.0), (1.3, 0.3, 0, 0, nan),
              (1.3, 0.3, 0, 0, inf), (0, 0, 1.25, 1.1, 0.0)):
        assert lib().yk_engine_set_temperatures(h, *[float(x) for x in a]) == YK_ERR_ARG, a
    assert lib().yk_engine_set_temperatures(None, 1.3, 0.3, 0.0, 0.0, 8.0) == YK_ERR_ARG
    m2, r2 = eng.temperatures()  # unchanged by the rejected calls
    assert np.array_equal(m2, mt) and np.array_equal(r2, rt)
    assert lib().yk_engine_set_temperatures(h, 0.5, 0.5, 0.0, 0.0, 0.0) == 0  # flat: no halflife; the root's off
    m3 = np.zeros(48)
    r3 = np.ones(48)
    assert lib().yk_engine_temperatures(h, m3.ctypes.data, r3.ctypes.data) == 0
    assert (m3 == 0.5).all() and (r3 == 0.0).all()
    eng.close()
    one = E.SelfPlayEngine(2, 2, 1.5, 15, prior="hash", max_moves=48, root_policy_temperature=1.1)
    assert one.temperatures()[0] is None and (one.temperatures()[1] == 1.1).all()
    one.close()
    with pytest.raises(ValueError):
        E.SelfPlayEngine(2, 2, 1.5, 15, prior="hash", max_moves=48, move_temperature_early=0.75)


# ------------------------------------------------------------------ 1. the draw on crafted rows
def test_pick_rows_are_the_reference(Y):
    """One entry; two equal counts; {1, 65535} at T = 0.05 and 100; 3024 entries of count 1; 100 random counts at
    T in {0.15, 0.75, 1.3}; each at u = 0, u = 1 - 2^-53 and three more.  Exact picks wherever the reference's own
    margin is >= 1e-9 (every row but those that sit on a boundary by construction); totals within 1e-12."""
    from yacht_amd import kernels as K
    rng = np.random.default_rng(5)
    rnd = rng.integers(1, 400, size=100).tolist()
    base = [([5], 0.3), ([7, 7], 0.75), ([1, 65535], 0.05), ([1, 65535], 100.0), ([65535, 1], 0.05), ([1] * 3024, 0.15),
            ([1] * 3024, 1.3), (rnd, 0.15), (rnd, 0.75), (rnd, 1.3), (rnd, 1.0), (list(range(1, 131)), 0.75)]
    rows = [(c, t, u) for c, t in base for u in (0.0, 1.0 - 2.0 ** -53, 0.3, 0.5, 0.7)]
    indptr = np.cumsum([0] + [len(c) for c, _, _ in rows])
    counts = np.concatenate([np.asarray(c, dtype=np.int32) for c, _, _ in rows])
    pick, total = K.temperature_pick(_dev(indptr, np.int64), _dev(counts, np.int32),
                                     _dev([t for _, t, _ in rows], np.float64), _dev([u for _, _, u in rows], np.float64))
    pick, total = pick.cpu().numpy(), total.cpu().numpy()
    exact, worst = 0, 0.0
    for i, (c, t, u) in enumerate(rows):
        want, tot, margin = T.pick(c, t, u)
        worst = max(worst, abs(total[i] - tot) / tot)
        assert abs(total[i] - tot) <= 1e-12 * tot, (i, total[i], tot)
        assert 0 <= pick[i] < len(c)
        if margin >= T.MARGIN:
            assert pick[i] == want, (i, t, u, int(pick[i]), want)
            exact += 1
        if u == 0.0 or len(c) == 1:  # c_0 > 0 = u: 1 / 65535^20 is 5e-97, no underflow
            assert pick[i] == 0
    print(f"{exact} of {len(rows)} rows off the boundaries; worst relative total difference {worst:.3g}")
    # (u = 1 - 2^-53 sits within 2^-53 of the last c_i / last = 1 by construction, [7, 7] at u = 0.5 on c_0, and u = 0
    # within w_0 / total of 0 where that is tiny: those rows are held to the range and the total only; the
    # restatement puts 44 of the 60 rows off the boundaries, and those are held to the pick)
    assert exact == 44
    # an empty row and a row of zeros: nothing to draw from
    p2, t2 = K.temperature_pick(_dev([0, 0, 3], np.int64), _dev([0, 0, 0], np.int32), _dev([0.5, 0.5], np.float64),
                                _dev([0.3, 0.3], np.float64))
    assert p2.tolist() == [-1, -1] and t2.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        K.temperature_pick(_dev([0, 2, 1], np.int64), _dev([1, 1], np.int32), _dev([0.5, 0.5], np.float64),
                           _dev([0.3, 0.3], np.float64))
    with pytest.raises(ValueError):
        K.temperature_pick(_dev([0, 2], np.int64), _dev([1, 1], np.int32), _dev([0.0], np.float64), _dev([0.3], np.float64))


# ------------------------------------------------------------------ 2. the root transform on crafted rows
def test_root_temper_rows_are_the_reference(Y):
    """V in {1, 2, 5, 202, 3024} x T in {0.25, 0.8, 1.1, 1.25, 10}, a hash-prior row and the same row with every
    third entry an exact zero: no entry more than one float32 ulp from the float64 restatement, at most 0.1 % of
    a row's entries different at all, zeros stay zero, rows sum to 1 within 1e-6, V = 1 gives exactly [1]."""
    from yacht_amd import kernels as K
    boards, _ = O.init_board(77, [5, 6, 7, 8, 9])
    pri = [O.hash_prior(b)[0][0].astype(np.float32) for b in boards]
    rows, Vs, Ts = [], [], []
    for vi, V in enumerate((1, 2, 5, 202, 3024)):
        for temp in (0.25, 0.8, 1.1, 1.25, 10.0):
            for zeros in (False, True):
                p = pri[vi][:V].copy()
                if zeros and V > 1:
                    p[::3] = 0.0
                p = (p / p.sum(dtype=np.float32)).astype(np.float32)
                row = np.zeros(3226, dtype=np.float32)
                row[:V] = p
                row[V:] = 0.5  # (past nvalid: never read, and written as 0)
                rows.append(row)
                Vs.append(V)
                Ts.append(temp)
    got = K.root_temper(_dev(np.stack(rows), np.float32), _dev(Vs, np.int32), _dev(Ts, np.float64)).cpu().numpy()
    differ = 0
    for i, (row, V, temp) in enumerate(zip(rows, Vs, Ts)):
        want = T.root_temper(row[:V], temp)
        g = got[i, :V]
        assert not got[i, V:].any()
        assert np.array_equal(g == 0, row[:V] == 0), i
        ulps = np.abs(g.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (i, V, temp, int(ulps.max()))
        assert (ulps != 0).sum() <= 0.001 * V, (i, V, temp, int((ulps != 0).sum()))
        differ += int((ulps != 0).sum())
        assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 1e-6, (i, float(g.astype(np.float64).sum()))
        if V == 1:
            assert g.tolist() == [1.0]
        elif V >= 5:  # flatter above 1, sharper below
            assert (g.max() < row[:V].max()) if temp > 1 else (g.max() > row[:V].max())
    print(f"{differ} entries of {sum(Vs)} differ from the restatement by one ulp")
    # T == 1.0 exactly copies the row
    same = K.root_temper(_dev(np.stack(rows[:4]), np.float32), _dev(Vs[:4], np.int32), _dev([1.0] * 4, np.float64))
    for i in range(4):
        assert np.array_equal(same[i, :Vs[i]].cpu().numpy().view(np.uint32), rows[i][:Vs[i]].view(np.uint32))
    with pytest.raises(ValueError):
        K.root_temper(_dev(np.stack(rows[:1]), np.float32), _dev(Vs[:1], np.int32), _dev([-1.0], np.float64))


# ------------------------------------------------------------------ 3. off is off
@pytest.mark.parametrize("n,sims,prior", [(32, 25, "hash"), (8, 10, "net")])
def test_unset_or_exactly_one_is_the_plain_engine(Y, net, n, sims, prior):
    _, E, _ = Y
    r0, s0 = _run(E, n, sims, prior, net, 707, 900)
    r1, s1 = _run(E, n, sims, prior, net, 707, 900, move_temperature=None, root_policy_temperature=None)
    _same(r1, r0)
    assert s1 == s0
    ones = dict(move_temperature=1.0, move_temperature_early=1.0, root_policy_temperature=1.0,
                root_policy_temperature_early=1.0)
    r2, s2 = _run(E, n, sims, prior, net, 707, 900, **ones)
    _same(r2, r0)
    assert s2 == s0


# ------------------------------------------------------------------ 4. the move schedule alone, exact
@pytest.mark.parametrize("thr", T.THRESHOLDS)
def test_tempered_games_are_the_reference_games(Y, thr):
    """2 games x 6 sims, hash prior, 1.3 -> 0.3 with halflife 8, tempThreshold 49 (a draw at every move) and 15
    (argmax from move 14 on): every record field equals temper_ref.play_episode."""
    _, E, _ = Y
    rec, _ = _run(E, T.N_GAMES, T.SIMS, "hash", None, T.SEED, T.ENV_BASE, thr=thr, **MOVE)
    plain, _ = _run(E, T.N_GAMES, T.SIMS, "hash", None, T.SEED, T.ENV_BASE, thr=thr)
    if thr == 49:  # other moves are played (at 6 sims the first 14 moves' counts are nearly all 1: 1^(1/T) = 1)
        assert not np.array_equal(rec["info"][:, :, 2], plain["info"][:, :, 2])
    # the game's stream before move 0's step does not depend on T: one uniform either way
    assert np.array_equal(rec["ctr"][:, 0], plain["ctr"][:, 0])
    for e in range(T.N_GAMES):
        game = T.play_episode(T.SEED, T.ENV_BASE + e, T.SIMS, move_t=MT, temp_threshold=thr)
        assert game["margin"] >= T.MARGIN
        R.assert_game_equals_records(game, rec, e)
    assert (rec["info"][:, :thr - 1, 0] == 1).all()
    if thr == 15:
        assert (rec["info"][:, 14:48, 0] == 0).all()


# ------------------------------------------------------------------ 5. the root priors, bit for bit
@pytest.mark.parametrize("noise", [False, True])
def test_root_priors_are_the_device_transform(Y, noise):
    """4 games x 8 sims, record_predictions: for every move the tempered prior is yk_root_temper on `before` under
    the move's T - the same device function; `after` is that prior itself without the noise and
    f32((1 - eps) tempered + eps eta) with it."""
    _, E, _ = Y
    from yacht_amd import kernels as K
    seed, base, n = 31, 100, 4
    rec, _, (before, after) = _run(E, n, 8, "hash", None, seed, base, priors=True, record_predictions=True,
                                   **dict(ROOT, **(NOISE if noise else {})))
    assert (rec["n_moves"] == 48).all()
    mask, cnt = O.valid(rec["states"].reshape(-1, 8), 1)
    mask = mask.astype(bool)
    mv = np.tile(np.arange(48), n)
    before, after = before.reshape(-1, 3226), after.reshape(-1, 3226)
    assert 202 in cnt and cnt.max() > 256  # bid roots (full scans) and score roots (the sorted order)
    compact = np.zeros_like(before)
    for i in range(n * 48):
        assert np.array_equal(before[i] != 0, mask[i]), i
        compact[i, :cnt[i]] = before[i][mask[i]]
    temp = K.root_temper(_dev(compact, np.float32), _dev(cnt, np.int32), _dev(RT[mv], np.float64)).cpu().numpy()
    if noise:
        env = np.repeat(np.arange(base, base + n), 48)
        eta = K.dirichlet_noise(seed, env, mv, cnt, ALPHA).cpu().numpy()
    for i in range(n * 48):
        dense = np.zeros(3226, dtype=np.float32)
        dense[mask[i]] = temp[i, :cnt[i]]
        if noise:
            d_eta = np.zeros(3226)
            d_eta[mask[i]] = eta[i, :cnt[i]]
            dense = R.mix(dense, EPS, d_eta)
        assert np.array_equal(after[i].view(np.uint32), dense.view(np.uint32)), i
        assert cnt[i] == 1 or not np.array_equal(after[i], before[i])
        # and the transform is the restatement's, to the ulp
        if not noise and i % 12 == 0:
            want = T.root_temper(compact[i, :cnt[i]], float(RT[mv[i]]))
            ulps = np.abs(temp[i, :cnt[i]].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert ulps.max() <= 1


def test_root_priors_need_records_and_a_root_edit(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_STATE, YkError
    for kw in (dict(record_predictions=True), ROOT, dict(record_predictions=True, **MOVE)):
        eng = E.SelfPlayEngine(2, 2, 1.5, 15, prior="hash", max_moves=48, **kw)
        eng.run(1, 0)
        with pytest.raises(YkError) as ei:
            eng.root_priors()
        assert ei.value.code == YK_ERR_STATE
        eng.close()


# ------------------------------------------------------------------ 6. exact search under the root schedule
@pytest.mark.parametrize("kw,ref", [(ROOT, dict()),
                                    (dict(BOTH, forced_playouts_k=2.0, **NOISE), dict(move_t=MT, k=2.0))],
                         ids=["root", "all"])
def test_search_under_the_root_schedule_is_the_reference_search(Y, kw, ref):
    """2 games x 6 sims, tempThreshold 49.  The plain-Python Coach / MCTS, handed each move's recorded `after` at the
    top of getActionProb (after asserting that the Ps it replaces is the recorded `before`, bit for bit),
    reproduces every record - with the root schedule alone, and with the noise, the move schedule and forced
    playouts all on."""
    _, E, _ = Y
    rec, _, (before, after) = _run(E, T.N_GAMES, T.SIMS, "hash", None, T.SEED, T.ENV_BASE, priors=True, thr=49,
                                   record_predictions=True, **kw)
    # (P^(1/T) keeps the order of P: at 6 sims the root schedule alone need not change a single visit, and with the
    # hash prior it does not; the priors the search scanned did change, and the run with everything on does differ)
    assert not np.array_equal(after, before)
    if "dirichlet_alpha" in kw:
        plain, _ = _run(E, T.N_GAMES, T.SIMS, "hash", None, T.SEED, T.ENV_BASE, thr=49)
        assert not np.array_equal(rec["visits"], plain["visits"])
    for e in range(T.N_GAMES):
        seen = []

        def inject(move, P, e=e, seen=seen):
            assert P.dtype == np.float32
            assert np.array_equal(P.view(np.uint32), before[e, move].view(np.uint32)), (e, move)
            seen.append(move)
            return after[e, move].copy()

        game = T.play_episode(T.SEED, T.ENV_BASE + e, T.SIMS, temp_threshold=49, root_prior=inject, **ref)
        assert seen == list(range(48))
        assert game["margin"] >= T.MARGIN  # (exact actions are demanded of games that keep off the boundaries)
        R.assert_game_equals_records(game, rec, e)


# ------------------------------------------------------------------ 7. independent scan paths agree
def test_scan_paths_agree_under_the_root_schedule(Y, monkeypatch):
    """64 games x 40 sims: the default (sorted root order + node summary), full root scans, a kept order of 8
    entries (the fallback walks) and full first scans all see P' - identical records."""
    _, E, _ = Y
    out = []
    for env in ({}, {"YK_ROOT_SCAN": "0"}, {"YK_ROOT_K": "8"}, {"YK_NODE_SUMMARY": "0"}):
        for k in ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(_run(E, 64, 40, "hash", None, 707, 900, **ROOT))
    (r0, s0) = out[0]
    for r, s in out[1:]:
        _same(r, r0)
        assert s["expansions"] == s0["expansions"] and s["path_edges"] == s0["path_edges"]
    plain, _ = _run(E, 64, 40, "hash", None, 707, 900)
    assert not np.array_equal(plain["visits"], r0["visits"])


# ------------------------------------------------------------------ 8. invariances
def test_temperatures_do_not_depend_on_groups(Y, net):
    _, E, _ = Y
    (r1, s1), (r2, s2) = (_run(E, 32, 25, "net", net, 515, 300, groups=g, thr=49, **BOTH) for g in (1, 2))
    assert s1["groups"] == 1 and s2["groups"] == 2
    _same(r2, r1)


def test_temperatures_do_not_depend_on_sharding(Y):
    """4 games at env_base 100 = 2 games at 100 and 2 at 102: T is a function of the move alone."""
    _, E, _ = Y
    whole, _ = _run(E, 4, 10, "hash", None, 77, 100, thr=49, **BOTH)
    for lo in (0, 2):
        part, _ = _run(E, 2, 10, "hash", None, 77, 100 + lo, thr=49, **BOTH)
        for k in ("states", "info", "ctr", "values", "final", "n_moves"):
            assert np.array_equal(part[k], whole[k][lo:lo + 2]), k
        off = whole["visits_off"]
        a, b = int(off[lo * 48]), int(off[(lo + 2) * 48])
        assert np.array_equal(part["visits"], whole["visits"][a:b])
        assert np.array_equal(part["visits_off"], off[lo * 48:(lo + 2) * 48 + 1] - a)


# ------------------------------------------------------------------ 9. not applied elsewhere
def test_arena_plugin_and_reanalysis_are_untempered(Y, monkeypatch):
    _, E, N = Y
    from yacht_amd import replay
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.utils import dotdict
    seats = np.array([1, -1] * 4, dtype=np.int32)
    res = []
    for kw in ({}, BOTH):
        eng = E.SelfPlayEngine(8, 10, 1.5, 49, prior="hash", max_moves=48, **kw)  # (48: every record slot is written)
        eng.arena(seats, 21, 500, agent="mcts", opponent="random")
        res.append((eng.arena_results(), eng.records()))
        eng.close()
    for k, v in res[0][0].items():
        assert np.array_equal(res[1][0][k], v), k
    _same(res[1][1], res[0][1])
    probs = []
    args = dict(moveTemperature=0.3, moveTemperatureEarly=1.3, rootPolicyTemperature=1.1,
                rootPolicyTemperatureEarly=1.25, temperatureHalflife=8)
    for extra in ({}, args):
        game = YachtGame(seed=13, env_id=600)
        mcts = MCTS(game, N.HashPriorNet(game), dotdict(numMCTSSims=10, cpuct=1.5, **extra))
        board = game.getInitBoard()
        probs.append((mcts.getActionProb(game.getCanonicalForm(board, 1), temp=1), game.rng.ctr))
    assert probs[0] == probs[1]
    # the reanalysis: its searches are yk_mcts_search's, also on an engine that has the knobs set
    eng = E.SelfPlayEngine(4, 8, 1.5, 15, prior="hash", max_moves=48)
    eng.run(29, 700)
    img = eng.pack_records()
    eng.close()
    shard = replay.examples_from_images(img.reshape(1, -1), 4, 48, 8)
    idx = torch.arange(3, 4 * 48, 10, dtype=torch.int32, device="cuda")
    outs = []
    init = E.SelfPlayEngine.__init__
    for knobs in ({}, BOTH):
        def with_knobs(self, *a, knobs=knobs, **kw):
            init(self, *a, **dict(kw, **knobs))
        with monkeypatch.context() as mp:
            mp.setattr(E.SelfPlayEngine, "__init__", with_knobs)
            outs.append(replay.reanalyse(shard, idx, prior="hash", sims=8, cpuct=1.5, seed=29, env_base=3000))
    assert torch.equal(outs[0].targets, outs[1].targets)
    for k in ("pi_indptr", "pi_cols", "pi_vals"):
        assert torch.equal(outs[0].policies[k], outs[1].policies[k]), k


# ------------------------------------------------------------------ 10. Coach
def test_coach_passes_the_knobs_to_self_play(Y):
    Ymod, E, N = Y
    from yacht_amd.coach import Coach, examples_from_records
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    seed, env, sims = 17, 700, 8
    rec, _ = _run(E, 2, sims, "hash", None, seed, env, thr=49, **BOTH)
    want = examples_from_records(rec, 2)
    args = dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=49, moveTemperature=0.3, moveTemperatureEarly=1.3,
                   rootPolicyTemperature=1.1, rootPolicyTemperatureEarly=1.25, temperatureHalflife=8)
    got = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(), args).executeEpisodes(2)
    plain = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(),
                  dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=49)).executeEpisodes(2)

    def flat(games):
        return [([int(x) for x in Ymod.pack(s)], pi, v) for g in games for s, pi, v in g]

    assert flat(got) == flat(want)
    assert flat(got) != flat(plain)
    with pytest.raises(ValueError):
        Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(),
              dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=49, temperatureHalflife=8))


# ------------------------------------------------------------------ 11. direction
def test_direction_of_both_temperatures(Y):
    """32 games x 25 sims, tempThreshold 49.  A lower move temperature plays a most-visited action more often (hash
    prior: 0.900 of the moves at T = 0.3 against 0.613 at T = 1.0); a root policy temperature above 1 visits more
    distinct root children.

    The second is measured where the knob is meant to act, chosen by reasoning and not by result.  P^(1/T)
    renormalised keeps the order of P and moves mass from the entries above the prior's mean to those below it, so
    it can widen a root only (a) where the prior is sharp and (b) where the prior, not the sign of the values,
    decides whether an unvisited child is tried: under the reference's Q = 0 start an unvisited edge is tried or
    not by the sign of the visited children's Q, whatever P's shape.  So: a net whose policy head
    is sharp (random init, the head's last layer scaled by 3) searched under first-play urgency (r = 0.25), on both
    sides.  Measured elsewhere, for the record: hash prior (flat: no entry far above twice the mean), no FPU -
    7.19 distinct children per move at T = 1.25 against 7.31 off; the closed-form test net, no FPU - 15.71 against
    15.71, the same games move for move."""
    _, E, N = Y
    n, sims = 32, 25
    torch.manual_seed(0)
    sd = N.YachtNNet(hidden=64, nblocks=1).state_dict()
    sd["pi_head.2.weight"] = sd["pi_head.2.weight"] * 3.0
    sd["pi_head.2.bias"] = sd["pi_head.2.bias"] * 3.0
    sharp = N.YkNet(sd, 64, 1)

    def greedy_share(rec):
        off, vis, hit = rec["visits_off"], rec["visits"], 0
        for e in range(n):
            for m in range(48):
                v = vis[int(off[e * 48 + m]):int(off[e * 48 + m + 1])]
                hit += int(rec["info"][e, m, 2]) in v[v[:, 1] == v[:, 1].max(), 0].tolist()
        return hit / (n * 48)

    cold, _ = _run(E, n, sims, "hash", None, 909, 40, thr=49, move_temperature=0.3)
    unit, _ = _run(E, n, sims, "hash", None, 909, 40, thr=49, move_temperature=1.0)
    a, b = greedy_share(cold), greedy_share(unit)
    print(f"share of moves that are a most-visited action: T = 0.3 {a:.3f}, T = 1.0 {b:.3f}")
    assert a > b
    wide, _ = _run(E, n, sims, "net", sharp, 909, 40, thr=49, fpu_reduction=0.25, root_policy_temperature=1.25)
    off, _ = _run(E, n, sims, "net", sharp, 909, 40, thr=49, fpu_reduction=0.25)
    c, d = float(wide["info"][:, :48, 5].mean()), float(off["info"][:, :48, 5].mean())
    print(f"distinct visited root children per move: T = 1.25 {c:.2f}, off {d:.2f}")
    assert c > d


# ------------------------------------------------------------------ 12. profile classes
def test_root_temper_launches_are_class_six(Y, net):
    _, E, _ = Y
    n, sims = 16, 6
    for kw in (ROOT, dict(ROOT, **NOISE), MOVE):
        eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net, max_moves=48, **kw)
        eng.profile(True, stride=1)
        eng.run(5, 0)
        st, kt = eng.stats(), eng.kernel_times()
        eng.close()
        moves = int(st["moves"])
        assert st["errors"] == 0 and moves == 48
        assert kt["forward"][1] == moves * sims and kt["expand_backup_select"][1] == moves * sims
        assert kt["move_begin"][1] == moves and kt["move_end"][1] == moves and kt["select"][1] == moves
        if "root_policy_temperature" in kw:
            assert kt["root_temper"][1] == 2 * moves and kt["root_temper"][0] > 0
        else:
            assert "root_temper" not in kt
        if "dirichlet_alpha" in kw:
            assert kt["root_noise"] == kt["root_temper"]  # the same launches
        else:
            assert "root_noise" not in kt
