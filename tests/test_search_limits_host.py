"""The cases of test_gpu_search_limits.py do reach the limits they are there for - shown on the plain-Python
reference alone (tests/limits_ref.py over fpu_ref), so that a failure of the GPU module cannot be excused by its
inputs, and a changed capacity in csrc/yk_engine_dev.h fails here rather than emptying the GPU test.

The search kernels change paths at two fixed capacities: the root's visited-edge list holds
RV_CAP entries - one more and the rest of the move runs on full scans - and the root's kept P order holds RO_K."""
import numpy as np
import pytest

import limits_ref as L

RV_CAP, RO_K = L.dev_constant("RV_CAP"), L.dev_constant("RO_K")
LEFT = 100  # simulations that must still run after the visited list overflows: the fallback carries real picks


def test_the_capacities_are_the_ones_the_cases_were_chosen_for():
    assert (RV_CAP, RO_K) == (1024, 512)
    assert L.wide_root().shape == (8,) and len(L.SEARCH_ROOTS) == 4
    from oracle import oracle as O
    for _, w in L.SEARCH_ROOTS:
        assert int(O.valid(L.root_of_width(w), 1)[0][0].sum()) == w
    # a root of at most 256 entries never leaves full-scan mode (k_root_sort): the bid root is that tree
    assert [w for _, w in L.SEARCH_ROOTS if w <= 256] == [202]


@pytest.mark.parametrize("r", [None, L.RED])
def test_external_roots_cross_the_visited_list_mid_move(r):
    for (env, width), w in zip(L.SEARCH_ROOTS, L.search_case(r)):
        e, n = w["edges"], L.SIMS
        assert len(e) == 2 * n and all(b - a in (0, 1) for a, b in zip(e, e[1:]))
        if width <= 256:
            assert e[-1] <= width
            continue
        over, half = L.first_above(e, RV_CAP), L.first_above(e, RO_K)
        print(f"r={r} env {env} ({width} wide): {e[n - 1]} edges after call 1, {e[-1]} after call 2; past RO_K after "
              f"simulation {half}, past RV_CAP after simulation {over} with {n - 1 - over} left; largest N {w['max_n']}")
        # past RV_CAP within call 1, with simulations left: the hand-over is mid-move
        assert over is not None and n - 1 - over >= LEFT
        # past RO_K long before (a simulation adds one edge at most), and the kept order itself is used up:
        # every one of the RO_K largest priors is visited, so every walk ends without an unvisited entry
        assert half is not None and over - half >= RV_CAP - RO_K
        p = w["root_p"]
        top = np.lexsort((np.arange(len(p)), -p.astype(np.float64)))[:RO_K]  # P descending, the lower action first
        assert (w["counts"][0][top] > 0).all()
        # revisits interleave with new edges
        assert w["max_n"][0] >= 4
        # call 2 starts above the capacity: k_root_sort's own exit
        assert e[n - 1] > RV_CAP and e[-1] > e[n - 1]
        assert int((w["counts"][0] > 0).sum()) == e[n - 1] and int((w["counts"][1] > 0).sum()) == e[-1]
        assert int(w["counts"][0].sum()) == n - 1 and int(w["counts"][1].sum()) == 2 * n - 1  # (the first expands the root)
        if r is not None:
            assert w["fpu_picks"][1] > w["fpu_picks"][0] > w["fpu_unvisited_picks"][0] > 0


def test_the_game_passes_a_wide_root_with_every_reader_of_the_list():
    g = L.game_case()
    assert g["n_moves"] == L.GAME_MOVES
    for m, pm in enumerate(g["per_move"]):
        print(f"move {m}: {pm}")
    wide = [pm for pm in g["per_move"][4:6] if pm["raw_edges"] > RV_CAP]
    assert wide, [pm["raw_edges"] for pm in g["per_move"]]
    assert any(all(pm[k] > 0 for k in ("forced_picks", "pruned_visits", "fpu_picks", "fpu_unvisited_picks")) for pm in wide)
    assert [pm["raw_edges"] <= 256 for pm in g["per_move"][:4]] == [True] * 4  # (the bid roots: full scans only)


def test_the_arena_books_of_the_boundary_case():
    """test (d)'s games: the reference's arena peak is a multiple of 4 reached by one game's move, and the games
    below it exist too - the overflow of one tree must leave them alone."""
    games = L.arena_games(2026, (300, 301, 302), 30, 1.0)
    peaks = [max(t) for _, t in games]
    print("arena entries in use, the peak per game:", peaks)
    assert max(peaks) % 4 == 0 and max(peaks) > 0
    assert sum(p == max(peaks) for p in peaks) == 1 and min(peaks) <= max(peaks) - 4
