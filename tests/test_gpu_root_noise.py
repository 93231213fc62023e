"""Dirichlet root noise of self-play on the GPU: off by default and then
unobservable; on, each real move's root prior becomes P' = f32((1 - eps) P + eps eta) once, before any UCB
scan of that root in the move, with eta ~ Dir(alpha) from the device sampler (yk_dirichlet_noise) - and the
search under P' is still the reference's search, bit for bit, whichever scan path the engine takes."""
import numpy as np
import pytest

import noise_ref as R
from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
ALPHA, EPS = 0.3, 0.25
NOISE = dict(dirichlet_alpha=ALPHA, dirichlet_eps=EPS)


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


def _run(E, n, sims, prior, net, seed, base, priors=False, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net if prior == "net" else None, prior=prior, max_moves=48, **kw)
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


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 1.5])
def test_device_sampler_is_the_restatement(Y, alpha):
    """16 rows per alpha, V in {1, 2, 5, 202, 3024}: |d eta| <= 1e-9 eta + 1e-15 against the float64
    restatement (libm differences of a few 1e-16, amplified by at most |ln u| / alpha ~ 1e-12; one float32
    ulp is 6e-8), rows sum to 1 within 1e-12, columns past V are 0."""
    from yacht_amd import kernels as K
    seed = 2024 + (5 << 32)
    V = np.array([1, 2, 5, 202, 3024] * 3 + [3024], dtype=np.int32)
    env = np.array([7, 8, 9, 10, 2**31 - 1, 0, 1, 2, 3, 4, 100, 2**31, 2**32 - 16, 103, 104, 65536], dtype=np.int64)
    mv = np.array([0, 1, 2, 3, 4, 47, 46, 45, 44, 43, 10, 11, 12, 13, 14, 30], dtype=np.int32)
    got = K.dirichlet_noise(seed, env, mv, V, alpha).cpu().numpy()
    assert got.shape == (16, 3226) and got.dtype == np.float64
    worst = 0.0
    for i in range(16):
        ref = R.eta(seed, int(env[i]), int(mv[i]), int(V[i]), alpha)
        g = got[i, :V[i]]
        err = np.abs(g - ref)
        worst = max(worst, float((err / np.maximum(ref, 1e-300)).max()))
        assert np.all(err <= 1e-9 * ref + 1e-15), (i, int(V[i]), float(err.max()))
        assert abs(float(g.sum()) - 1.0) <= 1e-12
        assert not got[i, V[i]:].any()
    print(f"alpha {alpha}: worst relative difference {worst:.3g}")
    # the same rows again, and one row alone: a function of (seed, env, move, V, alpha) only
    assert np.array_equal(K.dirichlet_noise(seed, env, mv, V, alpha).cpu().numpy(), got)
    assert np.array_equal(K.dirichlet_noise(seed, env[15:], mv[15:], V[15:], alpha).cpu().numpy()[0], got[15])


# ------------------------------------------------------------------ 2. off is off
@pytest.mark.parametrize("n,sims,prior", [(32, 25, "hash"), (8, 10, "net")])
def test_alpha_or_eps_zero_is_the_plain_engine(Y, net, n, sims, prior):
    _, E, _ = Y
    r0, s0 = _run(E, n, sims, prior, net, 707, 900)
    for knobs in (dict(dirichlet_alpha=0.0, dirichlet_eps=EPS), dict(dirichlet_alpha=ALPHA, dirichlet_eps=0.0)):
        r1, s1 = _run(E, n, sims, prior, net, 707, 900, **knobs)
        _same(r1, r0)
        assert s1 == s0


# ------------------------------------------------------------------ 3. plumbing, bit for bit
def test_root_priors_are_the_mix_of_the_device_noise(Y):
    """4 games x 8 sims: for every move after == f32((1 - eps) before + eps eta) with eta from
    yk_dirichlet_noise for (seed, env, move, V); before is nonzero exactly on the move's valid mask; the
    game stream is untouched (move 0 starts at the noise-off run's counter)."""
    _, E, _ = Y
    from yacht_amd import kernels as K
    seed, base, n = 31, 100, 4
    rec, _, (before, after) = _run(E, n, 8, "hash", None, seed, base, priors=True, record_predictions=True, **NOISE)
    plain, _ = _run(E, n, 8, "hash", None, seed, base)
    # (the counter before move 0's search; the one after it counts the dice the searches rolled, and the
    # noised searches walk other paths - that the noise itself draws nothing from the stream is what
    # test_search_under_noise_is_the_reference_search pins, counter by counter)
    assert np.array_equal(rec["ctr"][:, 0, 0], plain["ctr"][:, 0, 0])
    assert np.array_equal(rec["states"][:, 0], plain["states"][:, 0])
    assert (rec["n_moves"] == 48).all()
    mask, cnt = O.valid(rec["states"].reshape(-1, 8), 1)
    env = np.repeat(np.arange(base, base + n), 48)
    mv = np.tile(np.arange(48), n)
    eta = K.dirichlet_noise(seed, env, mv, cnt, ALPHA).cpu().numpy()
    before, after = before.reshape(-1, 3226), after.reshape(-1, 3226)
    assert 202 in cnt and cnt.max() > 256  # bid roots (full scans) and score roots (the sorted order)
    for i in range(n * 48):
        ok = mask[i].astype(bool)
        assert np.array_equal(before[i] != 0, ok), i
        dense = np.zeros(3226)
        dense[ok] = eta[i, :cnt[i]]
        want = R.mix(before[i], EPS, dense)
        assert np.array_equal(after[i].view(np.uint32), want.view(np.uint32)), i
        assert cnt[i] == 1 or not np.array_equal(after[i], before[i])  # (one valid action: P = eta = [1])


def test_root_priors_need_records_and_noise(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_STATE, YkError
    for kw in (dict(record_predictions=True), NOISE):
        eng = E.SelfPlayEngine(2, 2, 1.5, 15, prior="hash", max_moves=48, **kw)
        eng.run(1, 0)
        with pytest.raises(YkError) as ei:
            eng.root_priors()
        assert ei.value.code == YK_ERR_STATE
        eng.close()


def test_noise_launches_have_their_own_profile_class(Y, net, monkeypatch):
    """With the noise on, the two k_root_noise launches of a move are timed as their own class, and the
    other classes keep their launch counts; with it off the class is not reported."""
    _, E, _ = Y
    n, sims = 16, 6
    for kw, full_root_scans in ((NOISE, False), (NOISE, True), ({}, False)):
        monkeypatch.delenv("YK_ROOT_SCAN", raising=False)
        if full_root_scans:  # simulation 1's descent is then a launch of its own, timed with class 2
            monkeypatch.setenv("YK_ROOT_SCAN", "0")
        eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net, max_moves=48, **kw)
        eng.profile(True, stride=1)
        eng.run(5, 0)
        st, kt = eng.stats(), eng.kernel_times()
        eng.close()
        moves = int(st["moves"])
        assert st["errors"] == 0 and moves == 48
        assert kt["forward"][1] == moves * sims and kt["expand_backup_select"][1] == moves * sims
        assert kt["move_begin"][1] == moves and kt["move_end"][1] == moves and kt["select"][1] == moves
        if kw:
            assert kt["root_noise"][1] == 2 * moves and kt["root_noise"][0] > 0
        else:
            assert "root_noise" not in kt


# ------------------------------------------------------------------ 4. exact search under noise
def test_search_under_noise_is_the_reference_search(Y):
    """2 games x 6 sims.  The plain-Python Coach / MCTS (tests/noise_ref.py) first reproduces the noise-off
    engine's records - that pins the restatement - and then, handed each move's recorded P' at the top of
    getActionProb (after asserting that the Ps it replaces is the recorded P, bit for bit), reproduces every
    record of the noised engine: states, actions, visit counts, values and stream counters."""
    _, E, _ = Y
    seed, base, n, sims = 11, 3, 2, 6
    plain, _ = _run(E, n, sims, "hash", None, seed, base)
    for e in range(n):
        R.assert_game_equals_records(R.play_episode(seed, base + e, sims), plain, e)
    rec, _, (before, after) = _run(E, n, sims, "hash", None, seed, base, priors=True, record_predictions=True,
                                   **NOISE)
    assert not np.array_equal(rec["visits"], plain["visits"])
    for e in range(n):
        seen = []

        def inject(move, P, e=e, seen=seen):
            assert P.dtype == np.float32
            assert np.array_equal(P.view(np.uint32), before[e, move].view(np.uint32)), (e, move)
            seen.append(move)
            return after[e, move].copy()

        game = R.play_episode(seed, base + e, sims, root_prior=inject)
        assert seen == list(range(48))
        R.assert_game_equals_records(game, rec, e)


# ------------------------------------------------------------------ 5. independent scan paths agree
def test_scan_paths_agree_under_noise(Y, monkeypatch):
    """64 games x 40 sims: the default (sorted root order + node summary), full root scans, a kept order of
    8 entries (the fallback walks) and full first scans all see P' - identical records."""
    _, E, _ = Y
    out = []
    for env in ({}, {"YK_ROOT_SCAN": "0"}, {"YK_ROOT_K": "8"}, {"YK_NODE_SUMMARY": "0"}):
        for k in ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(_run(E, 64, 40, "hash", None, 707, 900, **NOISE))
    (r0, s0) = out[0]
    for r, s in out[1:]:
        _same(r, r0)
        assert s["expansions"] == s0["expansions"] and s["path_edges"] == s0["path_edges"]


# ------------------------------------------------------------------ 6. invariances
def test_noise_does_not_depend_on_groups(Y, net):
    _, E, _ = Y
    (r1, s1), (r2, s2) = (_run(E, 32, 25, "net", net, 515, 300, groups=g, **NOISE) for g in (1, 2))
    assert s1["groups"] == 1 and s2["groups"] == 2
    _same(r2, r1)


def test_noise_does_not_depend_on_sharding(Y):
    """4 games at env_base 100 = 2 games at 100 and 2 at 102: the noise is keyed by the env id."""
    _, E, _ = Y
    whole, _ = _run(E, 4, 10, "hash", None, 77, 100, **NOISE)
    for lo in (0, 2):
        part, _ = _run(E, 2, 10, "hash", None, 77, 100 + lo, **NOISE)
        for k in ("states", "info", "ctr", "values", "final", "n_moves"):
            assert np.array_equal(part[k], whole[k][lo:lo + 2]), k
        off = whole["visits_off"]
        a, b = int(off[lo * 48]), int(off[(lo + 2) * 48])
        assert np.array_equal(part["visits"], whole["visits"][a:b])
        assert np.array_equal(part["visits_off"], off[lo * 48:(lo + 2) * 48 + 1] - a)


# ------------------------------------------------------------------ 7. noise changes play, nothing else breaks
def test_noise_changes_the_visit_counts_only(Y):
    """8 games x 25 sims.  Every game's visit counts differ from the noise-off run's in at least one move;
    no device error; and the search calls are the same either way, 25 x 48 per game: every move's visits sum
    to its root's Ns, which is 24 at a root the move itself expanded (its first search returns at the
    expansion) and 25 + the visits earlier searches left at a root that was already in the tree - so the
    sums equal the noise-off run's at move 0 and wherever both runs' roots are new, and never fall below
    24.  (The sums of later moves differ where the two runs reuse differently visited nodes.)"""
    _, E, _ = Y
    n, sims = 8, 25
    (r0, s0), (r1, s1) = _run(E, n, sims, "hash", None, 909, 40), _run(E, n, sims, "hash", None, 909, 40, **NOISE)
    assert s0["errors"] == 0 and s1["errors"] == 0
    assert s0["sims"] == s1["sims"] == sims * 48
    sums = []
    for r in (r0, r1):
        assert (r["n_moves"] == 48).all()
        off = r["visits_off"]
        tot = np.array([[int(r["visits"][int(off[e * 48 + m]):int(off[e * 48 + m + 1]), 1].sum()) for m in range(48)]
                        for e in range(n)])
        assert np.array_equal(tot, r["info"][:, :48, 4])
        assert (tot >= sims - 1).all()
        sums.append(tot)
    fresh = (sums[0] == sims - 1) & (sums[1] == sims - 1)
    assert fresh[:, 0].all() and np.array_equal(sums[0][fresh], sums[1][fresh])
    print(f"moves with equal visit sums: {(sums[0] == sums[1]).sum()} of {n * 48}; new roots in both: {fresh.sum()}")
    for e in range(n):
        differ = 0
        for m in range(48):
            v0 = r0["visits"][int(r0["visits_off"][e * 48 + m]):int(r0["visits_off"][e * 48 + m + 1])]
            v1 = r1["visits"][int(r1["visits_off"][e * 48 + m]):int(r1["visits_off"][e * 48 + m + 1])]
            differ += not np.array_equal(v0, v1)
        assert differ >= 1, e


# ------------------------------------------------------------------ 8. the arena and the plugin ignore it
def test_arena_and_mcts_plugin_add_no_noise(Y):
    _, E, N = Y
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.utils import dotdict
    seats = np.array([1, -1] * 4, dtype=np.int32)
    res = []
    for kw in ({}, NOISE):
        eng = E.SelfPlayEngine(8, 10, 1.5, 15, prior="hash", max_moves=48, **kw)  # (48: every record slot is written)
        eng.arena(seats, 21, 500, agent="mcts", opponent="random")
        res.append((eng.arena_results(), eng.records()))
        eng.close()
    for k, v in res[0][0].items():
        assert np.array_equal(res[1][0][k], v), k
    _same(res[1][1], res[0][1])
    probs = []
    for extra in ({}, dict(dirichletAlpha=ALPHA, dirichletEpsilon=EPS)):
        game = YachtGame(seed=13, env_id=600)
        mcts = MCTS(game, N.HashPriorNet(game), dotdict(numMCTSSims=10, cpuct=1.5, **extra))
        board = game.getInitBoard()
        probs.append((mcts.getActionProb(game.getCanonicalForm(board, 1), temp=1), game.rng.ctr))
    assert probs[0] == probs[1]


# ------------------------------------------------------------------ 9. Coach
def test_coach_passes_the_knobs_to_self_play(Y):
    Ymod, E, N = Y
    from yacht_amd.coach import Coach, examples_from_records
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    seed, env, sims = 17, 700, 8
    rec, _ = _run(E, 2, sims, "hash", None, seed, env, **NOISE)
    want = examples_from_records(rec, 2)
    args = dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=15, dirichletAlpha=ALPHA, dirichletEpsilon=EPS)
    got = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(), args).executeEpisodes(2)
    plain = Coach(YachtGame(seed=seed, env_id=env), N.HashPriorNet(),
                  dotdict(numMCTSSims=sims, cpuct=1.5, tempThreshold=15)).executeEpisodes(2)

    def flat(games):
        return [([int(x) for x in Ymod.pack(s)], pi, v) for g in games for s, pi, v in g]

    assert flat(got) == flat(want)
    assert flat(got) != flat(plain)
