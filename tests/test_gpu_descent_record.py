"""The descent's single fetch of a node record per level: a level whose node is
known before any lookup - the move's cached root, a cached child - takes the record's fields and key
from one batch of loads and makes no Es test (no node record holds a terminal state); a looked-up
level takes the fields from the probe that matched the key; the fused kernel hands its tree and
generation to the descent.  There is no switch for any of it, so the yardsticks are the independent
oracle and the existing switches, at shapes with deep descents: 200 simulations give chains of four
and more cached children, many revisits, and late-game trees that reach terminal states through
cached edges."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")


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


def _run(E, n, sims, prior, net, seed, base, max_moves=48, **kw):
    eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net if prior == "net" else None, prior=prior,
                           max_moves=max_moves, **kw)
    eng.run(seed, base)
    st = eng.stats()
    rec = eng.records()
    eng.close()
    assert st["errors"] == 0, st
    return rec, st


def _dense_counts(rec, e, m):
    M = rec["states"].shape[1]
    a0, a1 = rec["visits_off"][e * M + m], rec["visits_off"][e * M + m + 1]
    c = np.zeros(3226, dtype=np.int32)
    v = rec["visits"][a0:a1]
    c[v[:, 0]] = v[:, 1]
    return c


@pytest.mark.parametrize("sims,max_moves", [(200, 48), (25, 64)])
def test_deep_cached_child_chains_vs_oracle(Y, sims, max_moves):
    """Hash prior, 32 games of full 48-move episodes: every record field, every move's visit counts and
    the expansion count are the oracle's (an independent CPU search that knows no cached child)."""
    _, E, _ = Y
    n, seed, base = 32, 4242, 1000
    rec, st = _run(E, n, sims, "hash", None, seed, base, max_moves=max_moves)
    orc = O.selfplay(np.arange(base, base + n), seed, sims, 1.5, 15, O.MODE_HASH, max_moves=max_moves, threads=16)
    assert orc["nerr"] == 0
    print(f"sims {sims}: path edges per simulation {st['path_edges'] / max(st['sims'], 1):.2f}, "
          f"expansions {st['expansions']}")
    for e in range(n):
        M = int(orc["stats"][e, 0])
        assert rec["n_moves"][e] == M == 48
        assert np.array_equal(rec["states"][e, :M], orc["canon"][e, :M])
        assert np.array_equal(rec["info"][e, :M, :7], orc["mv"][e, :M, :7]), e
        assert np.array_equal(rec["ctr"][e, :M], orc["ctr"][e, :M])
        for m in range(M):
            assert np.array_equal(_dense_counts(rec, e, m), orc["counts"][e, m]), (e, m)
        assert np.array_equal(rec["values"][e, :M], orc["values"][e, :M])
        assert np.array_equal(rec["final"][e], orc["final"][e])
    assert st["expansions"] == int(orc["stats"][:, 1].sum())


# (YK_SPLIT_DESCENT, YK_NODE_SUMMARY, YK_ROOT_SCAN); the first is the default
SETTINGS = [("0", "1", "1"), ("1", "1", "1"), ("0", "0", "0"), ("0", "0", "1"), ("0", "1", "0")]


@pytest.mark.parametrize("prior,sims", [("hash", 200), ("net", 40)])
def test_standalone_descent_and_fused_join_agree_when_deep(Y, net, prior, sims, monkeypatch):
    """k_select as its own launch (it loads the game's tree and generation itself) against the fused
    kernel's join (they are handed over), and the node summary and the root's incremental scan off and
    on: the same records, expansions, path edges and edge gathers.  The entries scanned differ only as
    the summary and the root scan make them: fewer with either on, the same with the split launch."""
    _, E, _ = Y
    out = {}
    for split, summary, rscan in SETTINGS:
        monkeypatch.setenv("YK_SPLIT_DESCENT", split)
        monkeypatch.setenv("YK_NODE_SUMMARY", summary)
        monkeypatch.setenv("YK_ROOT_SCAN", rscan)
        out[(split, summary, rscan)] = _run(E, 64, sims, prior, net, 808, 4200)
    r0, s0 = out[SETTINGS[0]]
    print({k: s["scanned"] for k, (_, s) in out.items()}, "path edges per simulation",
          s0["path_edges"] / max(s0["sims"], 1))
    for key in SETTINGS[1:]:
        r, s = out[key]
        for k in ("expansions", "path_edges", "scan_edges"):
            assert s[k] == s0[k], (key, k)
        for k in FIELDS:
            assert np.array_equal(r[k], r0[k]), (key, k)
    assert out[("1", "1", "1")][1]["scanned"] == s0["scanned"]
    sc = {key[1:]: out[key][1]["scanned"] for key in SETTINGS if key[0] == "0"}
    assert sc[("1", "0")] < sc[("0", "0")] and sc[("1", "1")] < sc[("0", "1")]  # the summary reads fewer
    assert sc[("0", "1")] < sc[("0", "0")] and sc[("1", "1")] < sc[("1", "0")]  # so does the root scan


def test_two_game_groups_equal_one(Y, net):
    """groups=2 (each group's launches on its own stream) against groups=1, net prior."""
    _, E, _ = Y
    (r1, s1), (r2, s2) = (_run(E, 32, 25, "net", net, 515, 300, groups=g) for g in (1, 2))
    assert s1["groups"] == 1 and s2["groups"] == 2
    for k in ("expansions", "path_edges", "scan_edges", "scanned"):
        assert s2[k] == s1[k], k
    for k in FIELDS:
        assert np.array_equal(r2[k], r1[k]), k


def test_gating_arena_dual_trees_replayed_by_oracle(Y):
    """A small gating arena, the previous net against the new one, each seat with its own tree: the
    tree a game searches (t >= E for the opponent's seat) and its generation reach the descent through
    the fused kernel's join.  The oracle (dual trees) replays the recorded predictions and ends every
    game with the same result, totals, actions and stream counters."""
    _, E, N = Y
    n, sims, seed, base = 16, 25, 515, 7000
    sd_a = spec.closed_form_weights(256, 6)
    sd_b = {k: (np.asarray(v, dtype=np.float32) * np.float32(0.9) if k.endswith("weight") else v)
            for k, v in sd_a.items()}
    seats = np.where(np.arange(n) < n // 2, 1, -1).astype(np.int32)
    eng = E.SelfPlayEngine(n, sims, 1.5, 0, net=N.YkNet(sd_a, 256, 6), opponent_net=N.YkNet(sd_b, 256, 6),
                           max_moves=48, record_predictions=True, max_expansions=48 * sims + 16, dual_trees=True)
    eng.arena(seats, seed, base, agent="mcts", opponent="mcts")
    assert eng.stats()["errors"] == 0
    r = eng.arena_results()
    pi, v, cnt = eng.predictions()
    o = O.arena_dual(np.arange(base, base + n), seats, seed, sims, 1.5, O.MODE_REPLAY,
                     replay=[(pi[e, :cnt[e]], v[e, :cnt[e]]) for e in range(n)], max_moves=48, threads=16)
    eng.close()
    assert o["nerr"] == 0
    assert np.array_equal(o["stats"][:, 1], cnt)
    assert np.array_equal(r["result"], o["result"])
    assert np.array_equal(r["totals"], o["totals"])
    assert np.array_equal(r["final"], o["final"])
    assert np.array_equal(r["n_moves"], o["stats"][:, 0].astype(np.int32))
    assert np.array_equal(r["ctr"], o["stats"][:, 4].astype(np.uint64))
    for i in range(n):
        m = int(r["n_moves"][i])
        assert np.array_equal(r["actions"][i, :m], o["actions"][i, :m]), i
