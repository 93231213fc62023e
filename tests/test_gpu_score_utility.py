"""The score-margin utility on the GPU: opt-in, at the terminal states of every search of an
engine it is set on, and in the value targets.

* off is off: unset, on = 0 through the setter, and on = 0 after a setter call - every record and counter is the
  default engine's; on with weight 0 plays the same games and counts its terminal returns;
* yk_score_utility against the numpy rule (tests/utility_ref.py), float64 bit for bit;
* on, every game equals utility_ref.play_episode bit for bit - records, visits and every move's root-value word,
  which is what pins the utility's bits - alone and with the other search features;
* yk_mcts_search, the MCTS plugin and both arenas against the same searches; the arenas report the games' own
  results;
* yk_examples_utility_targets against utility_ref.value_targets, float32 bit for bit; the Coach's plumbing."""
import ctypes as C

import numpy as np
import pytest

import fpu_ref as FR
import noise_ref as R
import playout_ref as PR
import utility_ref as UR
import value_ref as V
from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
TT = 15
# the fixed case: 3 games x 30 simulations, hash prior, cpuct 1.0
SEED, BASE, SIMS, CPUCT = 2026, 300, 30, 1.0
W, SCALE = 0.5, 20000.0
UTIL = dict(score_utility=W, score_scale=SCALE)
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)  # test_gpu_root_noise.py's


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


def _run(E, n, sims, seed, base, net=None, priors=False, setter=None, cpuct=1.5, image=False, **kw):
    eng = E.SelfPlayEngine(n, sims, cpuct, TT, net=net, prior="hash" if net is None else "net", max_moves=48, **kw)
    if setter is not None:
        setter(eng)
    eng.run(seed, base)
    st, rec = eng.stats(), eng.records()
    pri = eng.root_priors() if priors else None
    img = eng.pack_records() if image else None
    eng.close()
    assert st["errors"] == 0, st
    out = (rec, st)
    return out + ((pri,) if priors else ()) + ((img,) if image else ())


def _same(r1, r0):
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k


@pytest.fixture(scope="module")
def plain48(Y):
    """48 hash-prior games x 12 sims with everything off: test 1's baseline and test 3's states."""
    _, E, _ = Y
    return _run(E, 48, 12, 707, 900)


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("prior,n,groups", [("hash", 48, 1), ("hash", 48, 2), ("net", 6, 1)])
def test_off_is_off(Y, net, plain48, prior, n, groups):
    """The shapes of test_gpu_fpu.py's test_off_is_off.  Unset is the default engine; so is on = 0 through the
    setter, whatever weight and scale come with it, and on = 0 after the utility had been set on.  On with weight 0
    returns the outcome's own bits from every terminal descent: the same records, and the counter shows it ran."""
    _, E, _ = Y
    from yacht_amd._lib import call
    nt = net if prior == "net" else None
    r0, s0 = plain48 if (prior, groups) == ("hash", 1) else _run(E, n, 12, 707, 900, net=nt, groups=groups)
    assert s0["utility_terminals"] == 0

    def on_then_off(eng):
        call("yk_engine_set_score_utility", eng.handle, 1, 0.5, 20000.0)
        call("yk_engine_set_score_utility", eng.handle, 0, 0.5, 20000.0)

    cases = [dict(score_utility=None, score_scale=None),
             dict(setter=lambda eng: call("yk_engine_set_score_utility", eng.handle, 0, 0.0, 1.0)),
             dict(setter=lambda eng: call("yk_engine_set_score_utility", eng.handle, 0, 1.0, 1e-3)), dict(setter=on_then_off)]
    for kw in cases:
        r1, s1 = _run(E, n, 12, 707, 900, net=nt, groups=groups, **kw)
        _same(r1, r0)
        assert s1 == s0
    r2, s2 = _run(E, n, 12, 707, 900, net=nt, groups=groups, score_utility=0.0, score_scale=20000.0)
    _same(r2, r0)
    assert s2["utility_terminals"] > 0
    assert {k: v for k, v in s2.items() if k != "utility_terminals"} == {k: v for k, v in s0.items() if k != "utility_terminals"}


# ------------------------------------------------------------------ 2. the setter
def test_setter_rejects_bad_arguments_and_leaves_the_engine(Y):
    _, E, _ = Y
    from yacht_amd._lib import YK_ERR_ARG, YkError, call
    lib = __import__("yacht_amd").lib()
    for kw in (dict(score_utility=-0.5, score_scale=1000.0), dict(score_utility=1.5, score_scale=1000.0),
               dict(score_utility=float("nan"), score_scale=1000.0), dict(score_utility=0.5, score_scale=0.0),
               dict(score_utility=0.5, score_scale=-1.0), dict(score_utility=0.5, score_scale=float("inf")),
               dict(score_utility=0.5, score_scale=float("nan"))):
        with pytest.raises(YkError) as ei:
            E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, **kw)
        assert ei.value.code == YK_ERR_ARG, kw
    with pytest.raises(ValueError, match="score_scale needs score_utility"):
        E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, score_scale=1000.0)
    with pytest.raises(ValueError, match="score_utility needs score_scale"):
        E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48, score_utility=0.5)
    r0, s0 = _run(E, 2, 12, 5, 0)
    eng = E.SelfPlayEngine(2, 12, 1.5, TT, prior="hash", max_moves=48)
    h = C.c_void_p(eng.handle)
    for on in (0, 1):
        for w in (-1.0, -1e-300, 1.0000000000000002, float("nan"), float("inf"), -float("inf")):
            assert lib.yk_engine_set_score_utility(h, on, w, 1000.0) == YK_ERR_ARG, (on, w)
        for c in (0.0, -0.0, -1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
            assert lib.yk_engine_set_score_utility(h, on, 0.5, c) == YK_ERR_ARG, (on, c)
    eng.run(5, 0)  # still off
    _same(eng.records(), r0)
    assert eng.stats() == s0
    call("yk_engine_set_score_utility", eng.handle, 1, 0.0, 1e-300)  # the bounds themselves are legal
    call("yk_engine_set_score_utility", eng.handle, 1, 1.0, 1.7976931348623157e308)
    eng.close()


# ------------------------------------------------------------------ 3. yk_score_utility
def _draw_state():
    """A terminal state with equal totals, made by hand: every category of both players used, every score 0."""
    from yacht_amd.state import PlayerState, YachtState, pack
    return pack(YachtState(round_no=13, p1=PlayerState(used_mask=0xFFF), p2=PlayerState(used_mask=0xFFF)))


@pytest.mark.parametrize("w", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("c", [1e-3, 1000.0, 20000.0, 1e9])
def test_score_utility_is_the_numpy_rule(Y, plain48, w, c):
    """The final boards of 48 hash-prior games for both players, their move-0 states (not terminal) and a draw made
    by hand, for both players: u float64 bit for bit, the margins, 0.0 where the state is not terminal."""
    from yacht_amd import kernels as Kn
    rec = plain48[0]
    draw = _draw_state()
    states = np.concatenate([rec["final"], rec["final"], rec["states"][:, 0], draw[None], draw[None]]).astype(np.uint64)
    players = np.concatenate([np.ones(48), -np.ones(48), np.ones(48), [1, -1]]).astype(np.int32)
    z = np.array([O.ended(s, int(p))[0][0] for s, p in zip(states, players)])
    m = np.array([UR.margin(s) for s in states])
    assert (z[:96] != 0).all() and (z[96:144] == 0).all() and (z[144:] == 1e-4).all() and m[144] == 0
    assert len(set(m[:48].tolist())) > 10 and (m[:48] > 0).any() and (m[:48] < 0).any()
    want = np.array([UR.blend(zi, UR.squash(p, mi, c), w) if zi != 0 else 0.0 for zi, mi, p in zip(z, m, players)])
    for i in (0, 50, 100, 144):  # (the pieces above are utility()'s)
        assert want[i].tobytes() == UR.utility(states[i], players[i], w, c).tobytes()
    u, mg = Kn.score_utility(Kn.states_to_device(states), torch.from_numpy(players).cuda(), w, c)
    assert u.dtype == torch.float64 and mg.dtype == torch.int32 and u.shape == mg.shape == (146,)
    got = u.cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [(int(i), float(got[i]), float(want[i])) for i in bad[:8]]
    assert np.array_equal(mg.cpu().numpy(), m)
    assert np.all(np.abs(got) <= 1.0)
    if w == 0.0:
        assert np.array_equal(got.view(np.uint64), z.view(np.uint64))
    if w == 1.0:
        assert got[144] == 0.0 and got[145] == 0.0  # a draw: terminal, utility 0
    u2, _ = Kn.score_utility(Kn.states_to_device(states), torch.from_numpy(players).cuda(), w, c)  # equal bits
    assert torch.equal(u2, u)


def test_score_utility_rejects_bad_knobs(Y):
    from yacht_amd import kernels as Kn
    st = Kn.states_to_device(_draw_state())
    for w, c in ((-0.1, 1000.0), (1.5, 1000.0), (0.5, 0.0), (0.5, float("inf")), (float("nan"), 1000.0), (None, 1000.0),
                 (0.5, None)):
        with pytest.raises(ValueError):
            Kn.score_utility(st, 1, w, c)


# ------------------------------------------------------------------ 4. the fixed case
@pytest.fixture(scope="module")
def fixed_ref():
    """(off, on): the reference's three games with the utility off and on (root-value words in info[:, 7])."""
    off = [UR.play_episode(SEED, BASE + e, SIMS, cpuct=CPUCT) for e in range(3)]
    on = [UR.play_episode(SEED, BASE + e, SIMS, w=W, c=SCALE, cpuct=CPUCT) for e in range(3)]
    return off, on


def test_fixed_case_is_the_reference(Y, fixed_ref):
    """Measured on the reference alone: 286 terminal returns off and 287 on, at 13 distinct terminal states with
    margins from -271 000 to +291 000; visits differ from the off run in game 0 only and no move differs, so the
    visit counts alone are a weak witness - the root-value words (15 differ) are what pins the utility's bits."""
    _, E, _ = Y
    off, on = fixed_ref
    returns = sum(g["terminal_returns"] for g in on)
    words = sum(int((a["root_words"] != b["root_words"]).sum()) for a, b in zip(off, on))
    print("reference: terminal returns off / on", sum(g["terminal_returns"] for g in off), returns, "; words that differ",
          words, "; margins", sorted({m for g in on for m in g["margins"]}))
    assert returns >= 100
    assert words >= 6
    assert any(not np.array_equal(a["visits"], b["visits"]) for a, b in zip(off, on))
    rec, st = _run(E, 3, SIMS, SEED, BASE, cpuct=CPUCT, record_root_values=True, **UTIL)
    for e, g in enumerate(on):
        R.assert_game_equals_records(g, rec, e)  # (info[:, 7] is the move's root-value word)
        assert np.array_equal(rec["info"][e, :g["n_moves"], 7].view(np.uint32), g["root_words"]), e
    assert st["utility_terminals"] == returns
    # and the off run of the same engine shape is the off reference: the words differ because the utility does
    rec0, st0 = _run(E, 3, SIMS, SEED, BASE, cpuct=CPUCT, record_root_values=True)
    for e, g in enumerate(off):
        R.assert_game_equals_records(g, rec0, e)
    assert st0["utility_terminals"] == 0


# ------------------------------------------------------------------ 5. external roots
def test_mcts_search_of_external_roots(Y, fixed_ref):
    """yk_mcts_search on fresh trees from the move-44 states of the off run's games, 200 simulations each on its own
    stream.  Measured on the reference, off / on: 27 / 28, 29 / 29 and 27 / 30 terminal returns; the counts differ
    from off for two of the three roots."""
    _, E, _ = Y
    from yacht_amd import kernels as Kn
    from yacht_amd._lib import call, stream_ptr
    roots = np.stack([g["states"][44] for g in fixed_ref[0]])
    n, sims = 3, 200
    want = [UR.search_counts(SEED, 500 + i, roots[i], sims, CPUCT, w=W, c=SCALE) for i in range(n)]
    off = [UR.search_counts(SEED, 500 + i, roots[i], sims, CPUCT) for i in range(n)]
    print("terminal returns off / on", [(a[2].terminal_returns, b[2].terminal_returns) for a, b in zip(off, want)])
    assert sum(not np.array_equal(a[0], b[0]) for a, b in zip(off, want)) >= 1
    eng = E.SelfPlayEngine(n, sims, CPUCT, prior="hash", max_moves=1, **UTIL)
    call("yk_mcts_reset", eng.handle)
    dev = Kn.states_to_device(np.ascontiguousarray(roots))
    env = torch.arange(500, 500 + n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros((n, Kn.ACTION_SIZE), dtype=torch.int32, device="cuda")
    call("yk_mcts_search", eng.handle, dev.data_ptr(), SEED, env.data_ptr(), ctr.data_ptr(), sims, counts.data_ptr(),
         stream_ptr())
    st = eng.stats()
    eng.close()
    got = counts.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], want[i][0]), i
        assert int(ctr[i].item()) == want[i][1], i
    assert st["errors"] == 0
    assert st["utility_terminals"] == sum(w[2].terminal_returns for w in want) > 0


# ------------------------------------------------------------------ 6. with the other search features
K, RED = 2.0, 0.25
FAST, PROB = 4, 0.4  # (test_gpu_playout_cap.py's schedule at (2026, 300): 28 fast moves)


class _PerMove(UR.UtilityMCTS):
    """Notes the terminal returns after every move's search."""
    w, c = W, SCALE

    def get_action_counts(self, board, root_prior=None):
        got = super().get_action_counts(board, root_prior)
        self.__dict__.setdefault("marks", []).append(self.terminal_returns)
        return got


def _injector(before, after, e, full):
    """test_gpu_forced_playouts.py's: the move's recorded P' handed to the reference."""
    def inject(move, P):
        assert full[move]
        assert np.array_equal(P.view(np.uint32), before[e, move].view(np.uint32)), (e, move)
        return after[e, move].copy()
    return inject


def test_noise_forced_fpu_playout_cap_and_utility_compose(Y):
    """2 games x 30 sims with root noise (0.3, 0.25), forced playouts k = 2 with pruning, first-play urgency 0.25, the
    playout cap (4 sims, p = 0.4) and the utility together, against the composed reference.  Fast and full moves
    both end descents at terminal states under the utility."""
    _, E, _ = Y
    full = PR.schedule(SEED, BASE, PROB, 48)
    assert full.any() and (~full).any()
    rec, st, (before, after) = _run(E, 2, SIMS, SEED, BASE, cpuct=CPUCT, priors=True, record_predictions=True,
                                    forced_playouts_k=K, fpu_reduction=RED, playout_fast_sims=FAST, playout_full_prob=PROB,
                                    **NOISE, **UTIL)
    total = fast_returns = full_returns = 0
    tot = dict.fromkeys(("forced_picks", "pruned_visits", "fpu_unvisited_picks", "fpu_picks"), 0)
    for e in range(2):
        made = []

        def make(*a):
            made.append(_PerMove(*a))
            return made[0]
        g = FR.play_episode(SEED, BASE + e, SIMS, r=RED, k=K, cpuct=CPUCT, root_prior=_injector(before, after, e, full),
                            full=full, fast_sims=FAST, mcts_class=make)
        R.assert_game_equals_records(g, rec, e)
        marks = np.diff([0] + made[0].marks)
        assert len(marks) == 48
        fast_returns += int(marks[~full].sum())
        full_returns += int(marks[full].sum())
        total += made[0].terminal_returns
        for k in tot:
            tot[k] += g[k]
    assert fast_returns > 0 and full_returns > 0, (fast_returns, full_returns)
    assert st["utility_terminals"] == total and st["fast_moves"] == int((~full).sum())
    assert {k: st[k] for k in tot} == tot and tot["fpu_picks"] > 0


# ------------------------------------------------------------------ 7. the arenas
def _check_arena(last, games):
    for i, g in enumerate(games):
        m = len(g["actions"])
        assert int(last["n_moves"][i]) == m, i
        assert last["actions"][i, :m].tolist() == g["actions"], i
        assert float(last["result"][i]) == g["result"], i  # the game's own result
        assert np.array_equal(last["totals"][i], g["totals"]), i
        assert np.array_equal(last["final"][i], g["final"]) and int(last["ctr"][i]) == g["ctr"], i
        assert g["result"] in (1.0, -1.0, 1e-4, -1e-4)


def test_both_arenas_search_under_the_utility(Y):
    """A 2-game MCTSArena (the agent against the random player) and a 2-game dual-tree GatingArena (both seats
    search, each in its own tree) at 16 sims against Arena.playGame in plain Python over UtilityMCTS searches; the
    results and totals they report are the games' own, and the tallies count wins."""
    _, _, N = Y
    from yacht_amd.arena import GatingArena, MCTSArena
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    sims = 16
    args = dotdict(numMCTSSims=sims, cpuct=CPUCT, scoreUtility=W, scoreScale=SCALE, arenaCompare=2)
    game = YachtGame(seed=21, env_id=500)
    arena = MCTSArena(game, N.HashPriorNet(game), args)
    one, two, draws = arena.playGames(2)
    want = [UR.arena_game(21, 500 + i, seat, sims, w=W, c=SCALE, cpuct=CPUCT) for i, seat in enumerate((1, -1))]
    assert sum(g["terminal_returns"] for g in want) > 0
    _check_arena(arena.last, want)
    agent = [g["result"] * seat for g, seat in zip(want, (1, -1))]
    assert (one, two, draws) == (agent.count(1.0), agent.count(-1.0), 2 - agent.count(1.0) - agent.count(-1.0))
    gate = GatingArena(game, N.HashPriorNet(game), N.HashPriorNet(game), args)
    gate.playGames(2, env_base=600)
    want = [UR.arena_game(21, 600 + i, seat, sims, w=W, c=SCALE, cpuct=CPUCT, opponent="mcts", max_moves=48)
            for i, seat in enumerate((1, -1))]
    assert sum(g["terminal_returns"] for g in want) > 0
    _check_arena(gate.last, want)


# ------------------------------------------------------------------ 8. the value targets
KNOBS = [(0.0, 1.0), (0.5, 1.0), (0.0, 0.7), (0.3, 0.5)]
N_ENVS, VSIMS = 6, 8


@pytest.fixture(scope="module")
def two_images(Y):
    """Two packed images stacked as the all-gather stacks them: 6 hash-prior games x 8 sims each, env_base 0 and
    6, root values recorded, searched under the utility."""
    _, E, _ = Y
    return torch.stack([_run(E, N_ENVS, VSIMS, 31, base, image=True, record_root_values=True, **UTIL)[2] for base in (0, 6)])


def _reference(E, imgs, n_games, beta, lam, w, c):
    """utility_ref over the first n_games games of the stacked images, flat in (image, game, move) order:
    (targets f32, outcomes f64)."""
    v, z = [], []
    host = imgs.cpu().numpy()
    for g in range(n_games):
        u = E.unpack_record_image(host[g // N_ENVS], N_ENVS, 48, VSIMS)
        e = g % N_ENVS
        T = int(u["n_moves"][e])
        q = V.decode(u["info"][e, :, 7].view(np.uint32))
        g1 = UR.squash(1, UR.margin(u["final"][e]), c)
        v.append(UR.value_targets(q, u["values"][e], u["info"][e, :, 1], T, beta, lam, g1, w))
        z.append(u["values"][e, :T])
    return np.concatenate(v), np.concatenate(z)


@pytest.mark.parametrize("beta,lam", KNOBS)
def test_value_targets_are_the_restatement(Y, two_images, beta, lam):
    """12 games; the last 500 of the 576 examples, so the cut falls inside game 1."""
    _, E, _ = Y
    from yacht_amd import replay as Rp
    maxlen = 500
    want, z = _reference(E, two_images, 12, beta, lam, W, SCALE)
    assert len(want) == 576 and (576 - maxlen) % 48
    shard = Rp.examples_from_images(two_images, N_ENVS, 48, VSIMS, maxlen=maxlen, value_mix=beta, value_lambda=lam, **UTIL)
    got = shard.values.cpu().numpy()
    assert got.dtype == np.float32 and len(shard) == maxlen
    bad = np.flatnonzero(got.view(np.uint32) != want[-maxlen:].view(np.uint32))
    assert bad.size == 0, [(int(i), float(got[i]), float(want[-maxlen:][i])) for i in bad[:8]]
    assert np.array_equal(shard.outcomes.cpu().numpy(), z[-maxlen:].astype(np.float32))  # outcomes keep z
    assert np.array_equal(shard.policies["values64"].cpu().numpy(), z[-maxlen:])
    assert float(shard[maxlen - 1][2]) == float(z[-1])  # and so do the tuples
    plain = Rp.examples_from_images(two_images, N_ENVS, 48, VSIMS, maxlen=maxlen, value_mix=beta, value_lambda=lam)
    assert not torch.equal(shard.values, plain.values)
    assert np.all(np.abs(got) <= 1.0)
    if (beta, lam) == (0.0, 1.0):  # float32(p_t * U_t): two values per game
        assert shard.root_values is None
        assert all(len(set(np.abs(got[k:k + 48]).tolist())) == 1 for k in range(500 - 48 * 10, 500, 48))
    # weight 0: the existing path's bits
    zero = Rp.examples_from_images(two_images, N_ENVS, 48, VSIMS, maxlen=maxlen, value_mix=beta, value_lambda=lam,
                                   score_utility=0.0, score_scale=SCALE)
    assert np.array_equal(zero.values.cpu().numpy().view(np.uint32), plain.values.cpu().numpy().view(np.uint32))
    assert torch.equal(zero.states, plain.states) and torch.equal(zero.targets, plain.targets)


def _utility_targets(Y, imgs, n, beta, lam, w, c):
    vals = torch.full((max(n, 1),), 7.0, dtype=torch.float32, device="cuda")
    rv = torch.full((max(n, 1),), 7.0, dtype=torch.float32, device="cuda")
    miss = C.c_int64(-1)
    rc = Y[0].lib().yk_examples_utility_targets(imgs.data_ptr(), imgs.shape[0], N_ENVS, 48, VSIMS, -1, 0, n, beta, lam, w, c,
                                                vals.data_ptr(), rv.data_ptr(), C.byref(miss), None)
    torch.cuda.synchronize()
    return rc, int(miss.value), vals.cpu().numpy()[:n], rv.cpu().numpy()[:n]


def test_utility_targets_error_returns(Y, two_images):
    from yacht_amd import replay as Rp
    from yacht_amd._lib import YK_ERR_ARG, YK_ERR_STATE
    _, E, _ = Y
    n = 576
    for w, c in ((-0.1, SCALE), (1.5, SCALE), (float("nan"), SCALE), (W, 0.0), (W, -1.0), (W, float("inf")), (W, float("nan"))):
        rc, _, vals, _ = _utility_targets(Y, two_images, n, 0.3, 0.5, w, c)
        assert rc == YK_ERR_ARG and (vals == 7.0).all(), (w, c)
    for beta, lam in ((-0.1, 1.0), (0.0, 1.5), (float("nan"), 1.0)):
        assert _utility_targets(Y, two_images, n, beta, lam, W, SCALE)[0] == YK_ERR_ARG
    assert _utility_targets(Y, two_images, n + 1, 0.0, 1.0, W, SCALE)[0] == YK_ERR_ARG  # more than the images hold
    rc, miss, vals, rv = _utility_targets(Y, two_images, n, 0.3, 0.5, W, SCALE)
    assert (rc, miss) == (0, 0)
    assert np.array_equal(vals.view(np.uint32), _reference(E, two_images, 12, 0.3, 0.5, W, SCALE)[0].view(np.uint32))
    assert np.isfinite(rv).all()
    # images without root values: (0, 1) needs none; the others report every example that misses one, as today
    img = _run(E, N_ENVS, VSIMS, 31, 0, image=True, **UTIL)[2].reshape(1, -1)
    n = N_ENVS * 48
    rc, miss, vals, rv = _utility_targets(Y, img, n, 0.0, 1.0, W, SCALE)
    assert (rc, miss) == (0, 0) and np.isnan(rv).all()
    assert np.array_equal(vals.view(np.uint32), _reference(E, img, N_ENVS, 0.0, 1.0, W, SCALE)[0].view(np.uint32))
    for beta, lam, want in ((0.5, 1.0, n), (0.0, 0.5, n - N_ENVS)):  # every example; all but each game's last move
        rc, miss, _, _ = _utility_targets(Y, img, n, beta, lam, W, SCALE)
        assert rc == YK_ERR_STATE and miss == want
        with pytest.raises(ValueError, match="record_root_values"):
            Rp.examples_from_images(img, N_ENVS, 48, VSIMS, value_mix=beta, value_lambda=lam, **UTIL)
    shard = Rp.examples_from_images(img, N_ENVS, 48, VSIMS, **UTIL)  # the knob alone: no root values needed
    assert np.array_equal(shard.values.cpu().numpy().view(np.uint32), vals.view(np.uint32))
    with pytest.raises(ValueError, match="scoreScale needs scoreUtility"):
        Rp.examples_from_images(img, N_ENVS, 48, VSIMS, score_scale=SCALE)


# ------------------------------------------------------------------ 9. plumbing
ARGS = dict(numIters=2, numEps=4, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
            arenaCompare=2, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=1,
            batch_size=48, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3, amp=False)


def test_coach_iteration_carries_the_knobs(Y, monkeypatch, tmp_path):
    """Two tiny iterations (the second one reanalyses the first) with the knobs set and held-out games: every engine
    built for the Coach - self-play, the held-out games, the reanalysis, the gate - carries them, so does every
    examples_from_images call, and the self-play report has the counter."""
    _, E, _ = Y
    from yacht_amd import replay as Rp
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    ck = str(tmp_path / "ck")
    torch.manual_seed(5)
    net = NNetWrapper(YachtGame(seed=21, env_id=500), dotdict(
        ARGS, checkpoint=ck, load_folder_file=(ck, "best.pth.tar"), scoreUtility=W, scoreScale=SCALE, reanalyseFraction=0.5,
        holdoutEps=2))
    coach = Coach(net.game, net, net.args)
    made, built = [], []
    init, from_images = E.SelfPlayEngine.__init__, Rp.examples_from_images

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append((a[0], kw.get("max_moves"), bool(kw.get("dual_trees")), self.score_utility, self.score_scale))

    def spy_images(*a, **kw):
        built.append((kw.get("score_utility"), kw.get("score_scale")))
        return from_images(*a, **kw)

    monkeypatch.setattr(E.SelfPlayEngine, "__init__", spy)
    monkeypatch.setattr(Rp, "examples_from_images", spy_images)
    coach.learn()
    kinds = {(n, m, d) for n, m, d, _, _ in made if m != 1}
    assert kinds == {(4, 48, False), (2, 48, False), (2, 48, True)}  # self-play, the held-out games, the gate
    assert any(m == 1 for _, m, _, _, _ in made)  # the reanalysis
    assert all((w, c) == (W, SCALE) for _, _, _, w, c in made), made
    assert len(built) == 4 and all(b == (W, SCALE) for b in built), built
    assert set(coach.last_selfplay) == {"searched", "kept", "sims", "utility_terminals"}
    assert coach.last_selfplay["utility_terminals"] > 0
    assert coach.last_reanalysis and coach.last_reanalysis[0]["reanalysed"] > 0
    shard = coach.trainExamplesHistory[-1]
    assert not torch.equal(shard.values, shard.outcomes) and set(shard.outcomes.cpu().numpy().tolist()) <= {1.0, -1.0, np.float32(1e-4)}


def test_mcts_plugin_passes_the_knobs(Y, fixed_ref):
    _, _, N = Y
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.state import unpack
    from yacht_amd.utils import dotdict
    root = fixed_ref[0][0]["states"][44]
    args = dotdict(numMCTSSims=200, cpuct=CPUCT, scoreUtility=W, scoreScale=SCALE)
    game = YachtGame(seed=SEED, env_id=500)
    c0 = game.rng.ctr
    mcts = MCTS(game, N.HashPriorNet(game), args)
    got = mcts.search_counts(unpack(root))
    assert (mcts._engine.score_utility, mcts._engine.score_scale) == (W, SCALE)
    want, ctr, ref = UR.search_counts(SEED, 500, root, 200, CPUCT, w=W, c=SCALE, ctr=c0)
    assert np.array_equal(np.asarray(got, dtype=np.int32), want) and game.rng.ctr == ctr
    assert ref.terminal_returns > 0 and mcts._engine.stats()["utility_terminals"] == ref.terminal_returns
    off = UR.search_counts(SEED, 500, root, 200, CPUCT, ctr=c0)[0]
    assert not np.array_equal(off, want)  # (27 / 28 terminal returns: the knob changes this search)
    plain = MCTS(YachtGame(seed=SEED, env_id=500), N.HashPriorNet(game), dotdict(numMCTSSims=24, cpuct=CPUCT))
    plain._eng()
    assert (plain._engine.score_utility, plain._engine.score_scale) == (None, None)
