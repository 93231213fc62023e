"""The search past its fixed capacities ("limits"), bit for bit against the plain-Python
reference (tests/limits_ref.py over fpu_ref) - the cases test_search_limits_host.py proves to reach them:

a. a root whose visited-edge list fills mid-move (RV_CAP: k_expand_backup hands the rest of the move to full
   scans) after its kept P order is used up (RO_K: every walk ends without an unvisited entry), searched a second
   time on the same tree (k_root_sort finds more visited edges than the list holds);
b. the same searches with every root pick a full scan and with no node summary;
c. a self-play game through such roots with forced playouts, pruning and first-play urgency - everything that
   takes its sums from the visited list;
d. the arena bound: an arena of exactly the entries a batch uses plays the same games, four entries fewer is a
   clean YK_ERR_CAPACITY that writes outside nothing.
Hash prior throughout: the net adds nothing here."""
import numpy as np
import pytest

import limits_ref as L
import noise_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
SCAN_VARS = ("YK_ROOT_SCAN", "YK_ROOT_K", "YK_NODE_SUMMARY")
FPU_COUNTERS = ("fpu_picks", "fpu_unvisited_picks")
ERR_ARENA, ERR_STEP, ERR_MOVES, ERR_ZERO_COUNTS, ERR_ROOT = 4, 16, 128, 256, 512


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import engine
    assert [engine.SelfPlayEngine.ERROR_BITS[b] for b in (ERR_ARENA, ERR_STEP, ERR_MOVES, ERR_ZERO_COUNTS, ERR_ROOT)] == [
        "arena", "transition status", "move cap", "zero visit counts", "root not in tree"]
    return engine


def _within_capacity(st):
    assert st["max_nodes"] <= st["node_cap"] and st["max_edges"] <= st["edge_cap"] and st["max_arena"] <= st["arena_cap"], st


# ------------------------------------------------------------------ a / b. external roots
def _search_twice(E, r):
    """yk_mcts_reset, then yk_mcts_search twice on the four roots -> [(counts, ctr, stats)] after each call."""
    from yacht_amd import kernels as Kn
    from yacht_amd._lib import call, stream_ptr
    n = len(L.SEARCH_ROOTS)
    roots = np.stack([L.root_of_width(w) for _, w in L.SEARCH_ROOTS])
    eng = E.SelfPlayEngine(n, L.SIMS, L.CPUCT, prior="hash", max_moves=1, fpu_reduction=r,
                           fpu_root_reduction=None if r is None else L.ROOT_RED)
    call("yk_mcts_reset", eng.handle)
    dev = Kn.states_to_device(np.ascontiguousarray(roots))
    env = torch.tensor([e for e, _ in L.SEARCH_ROOTS], dtype=torch.int32, device="cuda")
    ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros((n, Kn.ACTION_SIZE), dtype=torch.int32, device="cuda")
    out = []
    for _ in range(2):
        call("yk_mcts_search", eng.handle, dev.data_ptr(), L.SEARCH_SEED, env.data_ptr(), ctr.data_ptr(), L.SIMS,
             counts.data_ptr(), stream_ptr())
        out.append((counts.cpu().numpy().copy(), ctr.cpu().numpy().copy(), eng.stats()))
    eng.close()
    return out


@pytest.mark.parametrize("r", [None, L.RED])
def test_visited_list_fills_mid_move_on_external_roots(E, r, monkeypatch):
    for k in SCAN_VARS:
        monkeypatch.delenv(k, raising=False)
    want = L.search_case(r)
    got = _search_twice(E, r)
    for c, (counts, ctr, st) in enumerate(got):
        for i, w in enumerate(want):
            bad = np.flatnonzero(counts[i] != w["counts"][c])
            assert len(bad) == 0, (c, i, len(bad), [(int(a), int(counts[i][a]), int(w["counts"][c][a])) for a in bad[:6]])
            assert int(ctr[i]) == w["ctr"][c], (c, i)
        assert st["errors"] == 0, (c, st)
        _within_capacity(st)
        for k in FPU_COUNTERS:  # (the searches of one tree accumulate: k_reset alone clears the counters)
            assert st[k] == (0 if r is None else sum(w[k][c] for w in want)), (c, k)


def test_every_scan_path_agrees_past_the_limits(E, monkeypatch):
    """The r = 0.25 searches under the default (root_scan until the list is full, node summaries), YK_ROOT_SCAN=0
    (every root pick a full scan: the code the default falls back to, from the move's start) and
    YK_NODE_SUMMARY=0.  The variables are read when an engine is made."""
    runs = {}
    for tag, env in (("default", {}), ("full", {"YK_ROOT_SCAN": "0"}), ("nosum", {"YK_NODE_SUMMARY": "0"})):
        for k in SCAN_VARS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        runs[tag] = _search_twice(E, L.RED)
    for tag in ("full", "nosum"):
        for c in range(2):
            (c0, t0, s0), (c1, t1, s1) = runs["default"][c], runs[tag][c]
            assert np.array_equal(c1, c0) and np.array_equal(t1, t0), (tag, c)
            for k in FPU_COUNTERS + ("expansions", "path_edges", "errors"):
                assert s1[k] == s0[k], (tag, c, k)
    for c in range(2):  # the incremental path did run before it gave way: it read fewer entries
        print(f"call {c + 1}: scanned", {tag: runs[tag][c][2]["scanned"] for tag in runs})
        assert runs["default"][c][2]["scanned"] < runs["full"][c][2]["scanned"]


# ------------------------------------------------------------------ c. self-play through a wide root
def _play(E, n, groups):
    """n games from env GAME_ENV on.  A game of GAME_MOVES moves does not end: the engine's defined answer is
    the move cap's error bit alone, YK_ERR_STATE from run() - and complete records."""
    from yacht_amd._lib import YK_ERR_STATE, YkError
    eng = E.SelfPlayEngine(n, L.GAME_SIMS, L.CPUCT, 15, prior="hash", max_moves=L.GAME_MOVES, groups=groups,
                           forced_playouts_k=L.FORCED_K, fpu_reduction=L.RED)
    with pytest.raises(YkError) as ei:
        eng.run(L.GAME_SEED, L.GAME_ENV)
    st, rec = eng.stats(), eng.records()
    eng.close()
    assert ei.value.code == YK_ERR_STATE and st["errors"] == ERR_MOVES, st
    assert st["groups"] == groups
    _within_capacity(st)
    return rec, st


@pytest.fixture(scope="module")
def one_game(E):
    return _play(E, 1, 1)


def test_self_play_through_a_wide_root(one_game):
    rec, st = one_game
    g = L.game_case()
    R.assert_game_equals_records(g, rec, 0, max_moves=L.GAME_MOVES)
    for k in ("forced_picks", "pruned_visits") + FPU_COUNTERS:
        assert st[k] == g[k] > 0, k


def test_self_play_through_a_wide_root_in_two_groups(E, one_game):
    rec, st = _play(E, 32, 2)
    for e in (0, 31):  # one game of either group
        R.assert_game_equals_records(L.game_case(L.GAME_ENV + e), rec, e, max_moves=L.GAME_MOVES)
    M = L.GAME_MOVES  # game 0 is the single game's, visits included
    for k in ("states", "info", "ctr", "values"):
        assert np.array_equal(rec[k][0], one_game[0][k][0]), k
    assert np.array_equal(rec["visits"][:int(rec["visits_off"][M])], one_game[0]["visits"])


# ------------------------------------------------------------------ d. the arena boundary
# test_gpu_feature_dispatch.py's fixed small case
SEED, BASE, NGAMES, SIMS, CPUCT, MOVES = 2026, 300, 3, 30, 1.0, 48


def _batch(E, arena_entries=0):
    return E.SelfPlayEngine(NGAMES, SIMS, CPUCT, 15, prior="hash", max_moves=MOVES, arena_entries=arena_entries)


def _records(eng):
    eng.run(SEED, BASE)
    st, rec = eng.stats(), eng.records()
    assert st["errors"] == 0, st
    return rec, st


def test_arena_boundary(E):
    from yacht_amd._lib import YK_ERR_CAPACITY, YkError
    games = L.arena_games(SEED, range(BASE, BASE + NGAMES), SIMS, CPUCT, MOVES)
    # 1. the default engine: the reference's games, and the reference's arena books
    eng = _batch(E)
    R0, s0 = _records(eng)
    eng.close()
    for e, (g, _) in enumerate(games):
        R.assert_game_equals_records(g, R0, e)
    M = s0["max_arena"]
    assert M % 4 == 0 and 0 < M < s0["arena_cap"]
    assert M == max(max(tops) for _, tops in games)
    # 2. exactly M entries: nothing is rounded away, nothing overflows, the same games
    eng = _batch(E, arena_entries=M)
    R1, s1 = _records(eng)
    eng.close()
    assert s1["arena_cap"] == M == s1["max_arena"]
    for k in FIELDS:
        assert np.array_equal(R1[k], R0[k]), k
    # 3. one allocation unit fewer.  Every expansion takes a multiple of 4 entries, so only an expansion that would
    #    bring a tree to exactly M entries fails - in the one game that peaks there, in the move the books name.
    eng = _batch(E, arena_entries=M - 4)
    with pytest.raises(YkError) as ei:
        eng.run(SEED, BASE)
    assert ei.value.code == YK_ERR_CAPACITY
    s3, R3 = eng.stats(), eng.records()
    eng.close()  # (succeeds)
    assert s3["arena_cap"] == M - 4 and s3["max_arena"] <= s3["arena_cap"]
    # The error word: ERR_ARENA, and what the records themselves show to have followed.  A leaf that could not be
    # expanded stays out of the tree (its value is backed up, the next visit tries again).  If that leaf is later a
    # move's root, k_move_end finds no root (ERR_ROOT, root Ns recorded as -1) and no counts: a temp-1 move has
    # nothing to draw from (ERR_ZERO_COUNTS) and plays action 0, a temp-0 move draws among all 3226 - either can be
    # illegal (ERR_STEP, the status in info[6], the game stops there) or leave a game that is not over after its
    # last move (ERR_MOVES: final result 0).  No other bit: the node, edge, hash and visit pools are sized for
    # one new node and one new edge per simulation, and a failed expansion makes fewer.
    want = ERR_ARENA
    for e in range(NGAMES):
        n = int(R3["n_moves"][e])
        info = R3["info"][e, :n]
        rootless = info[:, 4] == -1
        want |= ERR_ROOT if rootless.any() else 0
        want |= ERR_ZERO_COUNTS if (rootless & (info[:, 0] == 1)).any() else 0
        want |= ERR_STEP if ((info[:, 6] & 0xFF) != 0).any() else 0
        want |= ERR_MOVES if n == MOVES and not (info[:, 6] & 0xFF)[-1] and not R3["values"][e, :n].any() else 0
        assert ((info[:, 5] == 0) == rootless).all(), e  # (a root in the tree has visited edges)
    print("errors", s3["errors"], "expected", want)
    assert s3["errors"] == want
    # the games that stay below M - 4 entries are the default engine's, every field; the one that peaks is up
    # to the move that needs the M entries
    peak = [max(tops) for _, tops in games]
    assert sorted(p > M - 4 for p in peak) == [False, False, True]
    for e, (g, tops) in enumerate(games):
        m = next((i for i, t in enumerate(tops) if t > M - 4), g["n_moves"])
        assert int(R3["n_moves"][e]) >= m
        for k in ("states", "info", "ctr"):
            assert np.array_equal(R3[k][e, :m], R0[k][e, :m]), (e, k)
        if peak[e] <= M - 4:
            assert m == g["n_moves"] and np.array_equal(R3["values"][e], R0["values"][e])
            assert np.array_equal(R3["final"][e], R0["final"][e])
    # 4. a fresh default engine afterwards: engine 3 wrote outside nothing
    eng = _batch(E)
    R4, s4 = _records(eng)
    eng.close()
    for k in FIELDS:
        assert np.array_equal(R4[k], R0[k]), k
    assert s4 == s0
