"""Playout cap randomization on the GPU: with the cap on, a self-play batch searches each
move either in full or with the fast cap, by a per-(batch, move) schedule; only the full moves become examples.

* off is off: an engine with the cap unset, set to 0, or set with full_prob = 1 plays the default engine's games;
* the capped search is the per-move plugin search: every game equals, bit for bit, tests/playout_ref.episode -
  a Coach.executeEpisode loop over the plugin classes with MCTS.search_counts(canon, sims = the move's cap);
* fast moves get no root noise, and every move keeps its root value;
* yk_examples_full_rows, yk_policies_take and examples_from_images(full_only=True) against their numpy
  restatements; the Coach's two paths."""
import ctypes as C

import numpy as np
import pytest

import playout_ref as PR
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
SEED, BASE, SIMS, FAST, PROB, TT = 2026, 300, 12, 4, 0.4, 15
CAP = dict(playout_fast_sims=FAST, playout_full_prob=PROB)


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import yacht_amd
    from yacht_amd import engine, nnet, replay
    return yacht_amd, engine, nnet, replay


def _run(E, n, sims, seed, base, net=None, image=False, priors=False, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, TT, net=net, prior="hash" if net is None else "net", max_moves=48, **kw)
    eng.run(seed, base)
    st, rec = eng.stats(), eng.records()
    out = [rec, st]
    if image:
        out.append(eng.pack_records())
    if priors:
        out.append(eng.root_priors())
    eng.close()
    assert st["errors"] == 0, st
    return out


def _same(r1, r0):
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k


def _dense_counts(rec, e, m):
    M = rec["states"].shape[1]
    a0, a1 = rec["visits_off"][e * M + m], rec["visits_off"][e * M + m + 1]
    c = np.zeros(3226, dtype=np.int32)
    v = rec["visits"][a0:a1]
    c[v[:, 0]] = v[:, 1]
    return c


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("prior,n,groups", [("hash", 48, 1), ("hash", 48, 2), ("net", 6, 1), ("net", 6, 2)])
def test_off_is_off(Y, prior, n, groups):
    _, E, N, _ = Y
    net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6) if prior == "net" else None
    r0, s0 = _run(E, n, SIMS, 707, 900, net=net, groups=groups)
    assert "fast" not in r0
    for kw in (dict(playout_fast_sims=0), dict(playout_fast_sims=0, playout_full_prob=0.3),
               dict(playout_fast_sims=FAST, playout_full_prob=1.0)):
        r1, s1 = _run(E, n, SIMS, 707, 900, net=net, groups=groups, **kw)
        _same(r1, r0)
        assert s1 == s0 and s1["fast_moves"] == 0
        assert not (r1["info"][:, :, 6] & 0x100).any()
        if kw["playout_fast_sims"]:
            assert r1["fast"].shape == (n, 48) and not r1["fast"].any()


def test_engine_rejects_bad_knobs(Y):
    _, E, _, _ = Y
    from yacht_amd._lib import YK_ERR_ARG, YkError, call
    for kw in (dict(playout_fast_sims=1), dict(playout_fast_sims=-2), dict(playout_fast_sims=SIMS + 1),
               dict(playout_fast_sims=FAST, playout_full_prob=-0.1), dict(playout_fast_sims=FAST, playout_full_prob=1.1),
               dict(playout_fast_sims=FAST, playout_full_prob=float("nan"))):
        with pytest.raises(YkError) as ei:
            E.SelfPlayEngine(2, SIMS, 1.5, TT, prior="hash", max_moves=48, **kw)
        assert ei.value.code == YK_ERR_ARG, kw
    # a rejected setting leaves the engine as it was: still uncapped
    eng = E.SelfPlayEngine(2, SIMS, 1.5, TT, prior="hash", max_moves=48)
    with pytest.raises(YkError):
        call("yk_engine_set_playout_cap", eng.handle, 1, 0.5)
    eng.run(5, 0)
    assert eng.stats()["fast_moves"] == 0 and eng.stats()["sims"] == 48 * SIMS
    # the bounds themselves are legal: 2 and sims, 0 and 1
    call("yk_engine_set_playout_cap", eng.handle, 2, 0.0)
    call("yk_engine_set_playout_cap", eng.handle, SIMS, 1.0)
    eng.close()


# ------------------------------------------------------------------ 2. the capped search is the plugin's
@pytest.fixture(scope="module")
def capped(Y):
    """3 games under the fixed schedule, the engine's records and the plugin-class reference of each game."""
    _, E, N, _ = Y
    from yacht_amd.game import YachtGame
    from yacht_amd.mcts import MCTS
    from yacht_amd.utils import dotdict
    full = PR.schedule(SEED, BASE, PROB, 48)
    caps = np.where(full, SIMS, FAST)
    eng = E.SelfPlayEngine(3, SIMS, 1.5, TT, prior="hash", max_moves=48, **CAP)
    eng.run(SEED, BASE)
    rec, st = eng.records(), eng.stats()
    lib_full = E.playout_schedule(SEED, BASE, PROB, 48)  # yk_playout_schedule: the bits the engine uses
    eng.close()
    refs = []
    for e in range(3):
        game = YachtGame(seed=SEED, env_id=BASE + e)
        mcts = MCTS(game, N.HashPriorNet(game), dotdict(numMCTSSims=SIMS, cpuct=1.5, tempThreshold=TT))
        refs.append(PR.episode(game, mcts, caps, TT))
    return dict(full=full, caps=caps, rec=rec, st=st, lib_full=lib_full, refs=refs)


def test_capped_games_are_the_per_move_plugin_searches(capped):
    full, caps, rec, st = capped["full"], capped["caps"], capped["rec"], capped["st"]
    # the precondition: full and fast moves on both sides of the temperature threshold (moves 0..13 are temp 1)
    t1 = np.arange(48) + 1 < TT
    assert full[t1].any() and (~full[t1]).any() and full[~t1].any() and (~full[~t1]).any()
    assert st["errors"] == 0
    for e, ref in enumerate(capped["refs"]):
        M = ref["n_moves"]
        assert int(rec["n_moves"][e]) == M == 48
        assert np.array_equal(rec["info"][e, :M, 2], ref["actions"]), e
        assert np.array_equal(rec["info"][e, :M, 1], ref["players"]), e
        assert np.array_equal(rec["info"][e, :M, 0], t1[:M].astype(np.int32))
        assert np.array_equal(rec["ctr"][e, :M], ref["ctr"]), e
        for m in range(M):
            assert np.array_equal(_dense_counts(rec, e, m), ref["counts"][m]), (e, m)
        assert np.array_equal(rec["states"][e, :M], ref["canon"]), e
        assert np.array_equal(rec["values"][e, :M], ref["values"]), e
        assert np.array_equal(rec["final"][e], ref["final"]), e
        assert np.array_equal(rec["info"][e, :M, 6], np.where(full, 0, 0x100)), e  # status OK | the kind
    assert np.array_equal(rec["fast"], np.broadcast_to(~full, (3, 48)))
    assert np.array_equal(capped["lib_full"], full)
    assert st["sims"] == int(caps.sum())
    assert st["fast_moves"] == int((~full).sum())


@pytest.mark.parametrize("n", [8, 40])  # (8 games are one forward row tile: the engine keeps one group; 40 are two)
def test_capped_groups_do_not_change_results(Y, n):
    _, E, _, _ = Y
    r1, s1 = _run(E, n, SIMS, SEED, BASE, groups=1, **CAP)
    r2, s2 = _run(E, n, SIMS, SEED, BASE, groups=2, **CAP)
    assert s2["groups"] == (2 if n == 40 else 1)
    _same(r2, r1)
    assert np.array_equal(r2["fast"], r1["fast"]) and r1["fast"].any() and not r1["fast"].all()
    assert (s2["sims"], s2["fast_moves"], s2["expansions"]) == (s1["sims"], s1["fast_moves"], s1["expansions"])


def test_arena_is_never_capped(Y):
    """yk_arena on a capped engine plays the uncapped engine's games, also right after a capped self-play batch."""
    _, E, _, _ = Y
    seat = np.array([1, -1, 1, -1, 1, -1], dtype=np.int32)
    out = []
    for kw in ({}, CAP):
        eng = E.SelfPlayEngine(6, SIMS, 1.5, TT, prior="hash", max_moves=48, **kw)
        if kw:
            eng.run(SEED, BASE)
            assert eng.stats()["fast_moves"] > 0
        eng.arena(seat, SEED, BASE, agent="mcts", opponent="random")
        st = eng.stats()
        assert st["errors"] == 0 and st["fast_moves"] == 0
        out.append((eng.arena_results(), st["sims"], st["expansions"]))
        eng.close()
    assert out[1][1:] == out[0][1:]
    for k in ("result", "totals", "n_moves", "actions", "final", "ctr"):
        assert np.array_equal(out[1][0][k], out[0][0][k]), k


# ------------------------------------------------------------------ 3. noise and root values
def test_fast_moves_get_no_noise_and_every_move_a_root_value(Y):
    _, E, _, _ = Y
    noise = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25, record_predictions=True, record_root_values=True)
    rec, st, (before, after) = _run(E, 4, SIMS, SEED, BASE, priors=True, **noise, **CAP)
    full = PR.schedule(SEED, BASE, PROB, 48)
    assert (rec["n_moves"] == 48).all() and np.array_equal(rec["fast"], np.broadcast_to(~full, (4, 48)))
    for e in range(4):
        for m in range(48):
            if full[m]:  # (a root with one valid action has P = eta = [1]: the mix is the identity there)
                assert before[e, m].any(), (e, m)
                assert np.count_nonzero(before[e, m]) == 1 or not np.array_equal(after[e, m], before[e, m]), (e, m)
            else:
                assert not before[e, m].any() and not after[e, m].any(), (e, m)
    assert (rec["info"][:, :, 7] != 0).all()  # fast or full: TD(lambda) targets of earlier full moves read it
    assert not np.isnan(rec["root_values"]).any()
    # full_prob = 1: the uncapped noisy engine
    r1, s1, (b1, a1) = _run(E, 4, SIMS, SEED, BASE, priors=True, **noise, playout_fast_sims=FAST, playout_full_prob=1.0)
    r0, s0, (b0, a0) = _run(E, 4, SIMS, SEED, BASE, priors=True, **noise)
    _same(r1, r0)
    assert s1 == s0 and np.array_equal(b1, b0) and np.array_equal(a1, a0)


# ------------------------------------------------------------------ 4. yk_examples_full_rows
@pytest.fixture(scope="module")
def images(Y):
    """Two capped engines' images, 5 games each, with different env_base: concatenated as after an all-gather."""
    _, E, _, _ = Y
    parts = [_run(E, 5, SIMS, SEED, base, image=True, record_root_values=True, **CAP) for base in (BASE, BASE + 5)]
    imgs = torch.stack([p[2] for p in parts])
    host = [E.unpack_record_image(p[2].cpu().numpy(), 5, 48, SIMS) for p in parts]
    plain = torch.stack([_run(E, 5, SIMS, SEED, base, image=True)[2] for base in (BASE, BASE + 5)])
    return imgs, host, plain


def test_full_rows(Y, images):
    from yacht_amd import kernels as K
    from yacht_amd._lib import YK_ERR_CAPACITY, lib
    imgs, host, plain = images
    infos, nms = [h["info"] for h in host], [h["n_moves"] for h in host]
    s0, s1 = PR.schedule(SEED, BASE, PROB, 48), PR.schedule(SEED, BASE + 5, PROB, 48)
    assert not np.array_equal(s0, s1)  # the two ranks' schedules differ
    assert np.array_equal(infos[0][:, :, 6] != 0, np.broadcast_to(~s0, (5, 48)))
    assert np.array_equal(infos[1][:, :, 6] != 0, np.broadcast_to(~s1, (5, 48)))
    for n_games in (-1, 7, 0):
        want, total = PR.full_rows(infos, nms, n_games)
        got = K.examples_full_rows(imgs, 5, 48, SIMS, n_games=n_games)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), n_games
        assert K.examples_full_rows(imgs, 5, 48, SIMS, n_games=n_games, count_only=True) == len(want)
        assert total == (10 if n_games < 0 else n_games) * 48
    want, _ = PR.full_rows(infos, nms, -1)
    assert len(want) == 5 * int(s0.sum()) + 5 * int(s1.sum())
    # a capacity one short: YK_ERR_CAPACITY, nothing written past it
    buf = torch.full((len(want) + 4,), -9, dtype=torch.int32, device="cuda")
    n = C.c_int64()
    rc = lib().yk_examples_full_rows(imgs.data_ptr(), 2, 5, 48, SIMS, -1, buf.data_ptr(), len(want) - 1, C.byref(n), None)
    torch.cuda.synchronize()
    assert rc == YK_ERR_CAPACITY and n.value == len(want)
    b = buf.cpu().numpy()
    assert np.array_equal(b[:len(want) - 1], want[:-1]) and (b[len(want) - 1:] == -9).all()
    # images of engines without the cap: every example
    got = K.examples_full_rows(plain, 5, 48, SIMS)
    assert np.array_equal(got.cpu().numpy(), np.arange(10 * 48, dtype=np.int32))


# ------------------------------------------------------------------ 5. yk_policies_take
def _random_csr(rng, n, max_len):
    lens = rng.integers(0, max_len + 1, size=n)
    lens[rng.random(n) < 0.2] = 0  # empty rows
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(3226, size=l, replace=False)) for l in lens] + [np.zeros(0, dtype=np.int64)])
    return ip, cols.astype(np.int32), rng.random(int(ip[-1]))


def _indices(rng, n, m):
    """m indices within [0, n): random with repeats, a descending run, both ends."""
    idx = rng.integers(0, n, size=m).astype(np.int32)
    if m >= 3:
        k = min(m // 3, n)
        idx[:k] = np.arange(n - 1, n - 1 - k, -1)  # a descending run from the last row
        idx[-1], idx[-2] = 0, idx[0]               # the first row, and a repeat
    return idx


@pytest.mark.parametrize("n", [1, 256, 257, 513])
def test_policies_take(Y, n):
    from yacht_amd import kernels as K
    rng = np.random.default_rng(100 + n)
    ip, cols, vals = _random_csr(rng, n, 70)  # (70 > 64: rows longer than a wavefront)
    dev = tuple(torch.from_numpy(a).to("cuda") for a in (ip, cols, vals))
    for m in (0, 1, 256, 257, 700):
        idx = _indices(rng, n, m)
        want = PR.take(ip, cols, vals, idx)
        got = K.policies_take(dev, torch.from_numpy(idx).to("cuda"))
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float64
        assert np.array_equal(got[0].cpu().numpy(), want[0]), (n, m)
        assert np.array_equal(got[1].cpu().numpy(), want[1]), (n, m)
        assert np.array_equal(got[2].cpu().numpy().view(np.uint64), want[2].view(np.uint64)), (n, m)
    # the inputs are untouched
    assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev, (ip, cols, vals)))


def test_policies_take_phases_and_errors(Y):
    from yacht_amd import kernels as K
    from yacht_amd._lib import YK_ERR_ARG, YK_ERR_CAPACITY, YK_ERR_RANGE, YK_OK, lib
    rng = np.random.default_rng(9)
    n, m = 300, 400
    ip, cols, vals = _random_csr(rng, n, 12)
    idx = _indices(rng, n, m)
    want = PR.take(ip, cols, vals, idx)
    d_ip, d_cols, d_vals, d_idx = (torch.from_numpy(a).to("cuda") for a in (ip, cols, vals, idx))
    o_ip = torch.full((m + 2,), -9, dtype=torch.int64, device="cuda")
    k = len(want[1])
    o_cols = torch.full((k + 4,), -9, dtype=torch.int32, device="cuda")
    o_vals = torch.full((k + 4,), -9.0, dtype=torch.float64, device="cuda")
    nnz = C.c_int64(-1)
    tk = lib().yk_policies_take
    src = (d_ip.data_ptr(), d_cols.data_ptr(), d_vals.data_ptr(), n, d_idx.data_ptr(), m)
    # count only: out_indptr and nnz, nothing else
    assert tk(*src, o_ip.data_ptr(), None, None, 0, C.byref(nnz), None) == YK_OK
    assert nnz.value == k and np.array_equal(o_ip.cpu().numpy()[:m + 1], want[0]) and int(o_ip[m + 1]) == -9
    # a capacity one short
    assert tk(*src, o_ip.data_ptr(), o_cols.data_ptr(), o_vals.data_ptr(), k - 1, C.byref(nnz), None) == YK_ERR_CAPACITY
    torch.cuda.synchronize()
    assert nnz.value == k and (o_cols == -9).all() and (o_vals == -9.0).all()
    # the fill: exactly k entries
    assert tk(*src, o_ip.data_ptr(), o_cols.data_ptr(), o_vals.data_ptr(), k, C.byref(nnz), None) == YK_OK
    torch.cuda.synchronize()
    assert np.array_equal(o_cols.cpu().numpy()[:k], want[1]) and (o_cols[k:] == -9).all()
    assert np.array_equal(o_vals.cpu().numpy()[:k], want[2]) and (o_vals[k:] == -9.0).all()
    # an index outside [0, n): YK_ERR_RANGE in either phase, and nothing outside the outputs is written
    for badv in (n, -1):
        bad = idx.copy()
        bad[m // 2] = badv
        d_bad = torch.from_numpy(bad).to("cuda")
        o_cols.fill_(-9)
        a = (d_ip.data_ptr(), d_cols.data_ptr(), d_vals.data_ptr(), n, d_bad.data_ptr(), m)
        assert tk(*a, o_ip.data_ptr(), None, None, 0, C.byref(nnz), None) == YK_ERR_RANGE
        assert tk(*a, o_ip.data_ptr(), o_cols.data_ptr(), o_vals.data_ptr(), k, C.byref(nnz), None) == YK_ERR_RANGE
        torch.cuda.synchronize()
        assert int(o_ip[m + 1]) == -9 and (o_cols[k:] == -9).all()
        with pytest.raises(ValueError, match="idx"):
            K.policies_take((d_ip, d_cols, d_vals), d_bad)
    # m == 0
    o_ip.fill_(-9)
    assert tk(d_ip.data_ptr(), d_cols.data_ptr(), d_vals.data_ptr(), n, None, 0, o_ip.data_ptr(), None, None, 0,
              C.byref(nnz), None) == YK_OK
    assert nnz.value == 0 and int(o_ip[0]) == 0 and int(o_ip[1]) == -9
    # YK_ERR_ARG, with real device pointers: nothing is launched, the outputs stay as they are
    o_ip.fill_(-9)
    ok = [*src, o_ip.data_ptr(), None, None, 0, C.byref(nnz), None]

    def bad(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[int(key[1:])] = v
        return tk(*a) == YK_ERR_ARG
    oc, ov = o_cols.data_ptr(), o_vals.data_ptr()
    assert bad(a0=None) and bad(a6=None) and bad(a10=None)
    assert bad(a3=-1) and bad(a3=2**31) and bad(a5=-1) and bad(a5=2**31) and bad(a4=None)
    assert bad(a6=d_ip.data_ptr())
    assert bad(a7=oc) and bad(a7=oc, a8=ov, a1=None) and bad(a7=oc, a8=ov, a2=None) and bad(a7=oc, a8=ov, a9=-1)
    assert bad(a7=d_cols.data_ptr(), a8=ov, a9=k) and bad(a7=oc, a8=d_vals.data_ptr(), a9=k)
    assert bad(a7=d_idx.data_ptr(), a8=ov, a9=k)
    torch.cuda.synchronize()
    assert (o_ip == -9).all()


# ------------------------------------------------------------------ 6. examples_from_images(full_only=True)
def test_full_only_shard_is_the_host_filter(Y):
    _, E, _, R = Y
    knobs = dict(value_mix=0.3, value_lambda=0.7)
    _, _, img = _run(E, 6, SIMS, SEED, BASE, image=True, record_root_values=True, **CAP)
    every = R.examples_from_images(img, 6, 48, SIMS, **knobs)
    assert len(every) == 6 * 48 and every.n_searched == 6 * 48
    h = E.unpack_record_image(img.cpu().numpy(), 6, 48, SIMS)
    idx, total = PR.full_rows([h["info"]], [h["n_moves"]])
    per_game = int(PR.schedule(SEED, BASE, PROB, 48).sum())
    assert total == 6 * 48 and len(idx) == 6 * per_game
    P = every.policies
    csr = tuple(P[k].cpu().numpy() for k in ("pi_indptr", "pi_cols", "pi_vals"))
    cut = 2 * per_game + 3  # the last maxlen full examples: a cut inside a game
    assert cut % per_game != 0 and cut < len(idx)
    for maxlen in (None, cut, 10**6, 0):
        keep = idx if maxlen is None else idx[max(len(idx) - maxlen, 0):]
        got = R.examples_from_images(img, 6, 48, SIMS, maxlen=maxlen, full_only=True, **knobs)
        assert len(got) == len(keep) and got.n_searched == 6 * 48
        for name in ("states", "targets", "values", "outcomes", "root_values"):
            a, b = getattr(got, name).cpu().numpy(), getattr(every, name).cpu().numpy()[keep]
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (maxlen, name)
        assert np.array_equal(got.policies["values64"].cpu().numpy(), P["values64"].cpu().numpy()[keep])
        want = PR.take(*csr, keep)
        for a, b in zip((got.policies[k].cpu().numpy() for k in ("pi_indptr", "pi_cols", "pi_vals")), want):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), maxlen
    # the value targets saw whole games: a full move's target differs from its outcome where lambda < 1 reads on
    assert not torch.equal(every.values, every.outcomes)
    # without the knobs the shard has one values array, and so has its filter
    plain = R.examples_from_images(img, 6, 48, SIMS, full_only=True)
    assert plain.outcomes is plain.values and plain.root_values is None and len(plain) == len(idx)
    # uncapped images: full_only keeps every example
    _, _, img0 = _run(E, 6, SIMS, SEED, BASE, image=True)
    a, b = R.examples_from_images(img0, 6, 48, SIMS, full_only=True), R.examples_from_images(img0, 6, 48, SIMS)
    assert torch.equal(a.states, b.states) and torch.equal(a.targets, b.targets) and torch.equal(a.values, b.values)
    assert all(torch.equal(a.policies[k], b.policies[k]) for k in b.policies)


# ------------------------------------------------------------------ 7. the Coach
def test_coach_keeps_the_full_moves(Y):
    Ymod, E, N, _ = Y
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    args = dotdict(numMCTSSims=SIMS, cpuct=1.5, tempThreshold=TT, playoutFastSims=FAST, playoutFullProb=PROB)
    coach = Coach(YachtGame(seed=SEED, env_id=BASE), N.HashPriorNet(), args)
    games = coach.executeEpisodes(3)  # streams BASE .. BASE + 2: the batch (SEED, BASE)
    full = PR.schedule(SEED, BASE, PROB, 48)
    rec, _ = _run(E, 3, SIMS, SEED, BASE, **CAP)
    moves = np.nonzero(full)[0]
    for e, ex in enumerate(games):
        assert len(ex) == len(moves)
        for (board, pi, v), m in zip(ex, moves):
            assert [int(x) for x in Ymod.pack(board)] == [int(x) for x in rec["states"][e, m]]
            assert v == float(rec["values"][e, m])
            c = _dense_counts(rec, e, m)
            assert [a for a, p in enumerate(pi) if p] == (list(np.nonzero(c)[0]) if rec["info"][e, m, 0] else
                                                          [int(rec["info"][e, m, 2])])
    # the device path: the next batch starts at stream BASE + 3
    shard = coach.selfPlayExamples(4)
    n_full = int(PR.schedule(SEED, BASE + 3, PROB, 48).sum())
    assert len(shard) == 4 * n_full and shard.n_searched == 4 * 48
    caps = np.where(PR.schedule(SEED, BASE + 3, PROB, 48), SIMS, FAST)
    assert coach.last_selfplay == dict(searched=4 * 48, kept=4 * n_full, sims=int(caps.sum()))
    rec2, _ = _run(E, 4, SIMS, SEED, BASE + 3, **CAP)
    keep = ~rec2["fast"]
    assert np.array_equal(shard.states.cpu().numpy().view(np.uint64), rec2["states"][keep])
