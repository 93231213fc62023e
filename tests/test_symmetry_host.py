"""Symmetry augmentation, the parts that need no GPU: the restatement in
tests/symmetry_ref.py - the definition tests/test_gpu_symmetry.py holds the device to - is a symmetry of the
game as the oracle's own functions play it; the C ABI validates its arguments before any device call; and
NNetWrapper.train rejects an unknown symmetry name."""
import ctypes as C
import math

import numpy as np
import pytest

import symmetry_ref as R
from oracle import oracle as O

SEED, KEY = 0x1234_5678_9ABC_DEF0, 77
ALL = R.CARRY | R.ROLLS | R.GROUPS


@pytest.fixture(scope="module")
def pool(golden):
    """Every 23rd golden state and the hand-made ones, taken as canonical boards (the mover is p1)."""
    S = np.concatenate([golden("states.npz")["states"][::23], R.hand_states()])
    return np.ascontiguousarray(S, dtype=np.uint64)


def _plans(S, flags, seed=SEED, key=KEY):
    return [R.plan(S[k], k, key, seed, flags) for k in range(len(S))]


def _apply(S, plans):
    return np.array([R.transform_state(s, p) for s, p in zip(S, plans)], dtype=np.uint64)


def test_hand_states_cover_what_they_claim():
    H = R.hand_states()
    n1, n2 = (H[:, 1] >> np.uint64(40)) & np.uint64(0xF), (H[:, 4] >> np.uint64(40)) & np.uint64(0xF)
    assert {0, 5, 10} <= set(n1.tolist()) and {0, 5, 10} <= set(n2.tolist())
    w0 = H[:, 0]
    assert {1, 2, 13} <= set((w0 & np.uint64(0xF)).tolist())
    assert set(((w0 >> np.uint64(4)) & np.uint64(1)).tolist()) == {0, 1}
    pend = [int(((w >> 8) & 0xFF) != 0xFF) + int(((w >> 16) & 0xFF) != 0xFF) for w in w0.tolist()]
    assert set(pend) == {0, 1, 2}
    assert any(not (w >> 5) & 1 for w in w0.tolist()) and any(not (w >> 6) & 1 for w in w0.tolist())


def test_flags_do_not_move_the_draws_and_zero_is_the_identity(pool):
    for k in range(0, len(pool), 7):
        full = R.plan(pool[k], k, KEY, SEED, ALL)
        assert np.array_equal(R.transform_state(pool[k], R.plan(pool[k], k, KEY, SEED, 0)), pool[k])
        for f, names in ((R.CARRY, ("perm1", "perm2")), (R.ROLLS, ("permA", "permB")), (R.GROUPS, ("swap",))):
            one = R.plan(pool[k], k, KEY, SEED, f)
            assert all(one[x] == full[x] for x in names)
    hot = [p for p in _plans(pool, ALL)]
    assert any(p["swap"] for p in hot) and not all(p["swap"] for p in hot)
    assert any(p["perm1"] != sorted(p["perm1"]) for p in hot) and any(p["permB"] != sorted(p["permB"]) for p in hot)


def test_action_map_is_a_bijection_and_the_table_is_the_scalar_map(pool):
    for flags in (R.CARRY, R.GROUPS, ALL):
        for k, p in enumerate(_plans(pool, flags)):
            t = R.action_table(pool[k], p)
            assert np.array_equal(np.sort(t), np.arange(R.ASIZE)), (flags, k)
    H = R.hand_states()
    for k, p in enumerate(_plans(H, ALL, key=3)):
        t = R.action_table(H[k], p)
        assert t.tolist() == [R.map_action(a, H[k], p) for a in range(R.ASIZE)], k
        assert R.map_action(-1, H[k], p) == -1 and R.map_action(R.ASIZE, H[k], p) == R.ASIZE


@pytest.mark.parametrize("flags", [R.CARRY, R.ROLLS, R.GROUPS, ALL])
def test_valid_features_and_ended_follow_the_symmetry(pool, flags):
    """valid(T s) == A(valid(s)) as sets; featurize(T s) is featurize(s) with its carry and roll slots
    permuted (bit for bit); getGameEnded and the totals are invariant."""
    plans = _plans(pool, flags)
    T = _apply(pool, plans)
    ok, cnt = O.valid(pool, 1)
    okT, cntT = O.valid(T, 1)
    f, fT = O.featurize(pool), O.featurize(T)
    assert np.array_equal(cnt, cntT)
    for k, p in enumerate(plans):
        t = R.action_table(pool[k], p)
        assert np.array_equal(okT[k][t], ok[k]), k
        g = f[k].copy()
        for base, perm in ((3, p["perm1"]), (13, p["perm2"])):
            g[base:base + len(perm)] = f[k][base + np.array(perm, dtype=np.int64)]
        a = f[k][23 + np.array(p["permA"])]
        b = f[k][28 + np.array(p["permB"])]
        g[23:28], g[28:33] = (b, a) if p["swap"] else (a, b)
        assert g.tobytes() == fT[k].tobytes(), k
    (e, tot), (eT, totT) = O.ended(pool, 1), O.ended(T, 1)
    assert np.array_equal(e, eT) and np.array_equal(tot, totT)
    assert (e != 0).any()


def _sorted_form(words):
    """Carries and rolls sorted: the fields of a state up to the dice's order."""
    w = [int(x) for x in words]
    for base in (1, 4):
        n = (w[base] >> 40) & 0xF
        d = sorted((w[base] >> (4 * i)) & 0xF for i in range(n))
        w[base] = (w[base] & ~((1 << (4 * n)) - 1)) | sum(x << (4 * i) for i, x in enumerate(d))
    for sh in (24, 44):
        d = sorted((w[0] >> (sh + 4 * i)) & 0xF for i in range(5))
        w[0] = (w[0] & ~(0xFFFFF << sh)) | (sum(x << (4 * i) for i, x in enumerate(d)) << sh)
    return w


def test_score_steps_commute_with_carry_and_roll_permutations(pool):
    """Phase-1 states under CARRY | ROLLS: step(T s, A a) and step(s, a) agree on status, next player and
    stream counter, and on every field once carries and rolls are sorted - for valid actions, reused
    categories and combos past the carry (the reference's silent no-ops) alike."""
    idx = [k for k in range(len(pool)) if (int(pool[k, 0]) >> 4) & 1]
    rng = np.random.RandomState(5)
    plans = _plans(pool, R.CARRY | R.ROLLS)
    moved = 0
    for k in idx:
        p = plans[k]
        t = R.action_table(pool[k], p)
        ok, _ = O.valid(pool[k], 1)
        va = np.flatnonzero(ok[0])
        acts = np.concatenate([va[rng.permutation(len(va))[:12]], rng.randint(R.NBID, R.ASIZE, 4)]).astype(np.int32)
        Ts = R.transform_state(pool[k], p)
        o, npl, st, c = O.step(np.tile(pool[k], (len(acts), 1)), 1, acts, 9, k, 100)
        oT, nplT, stT, cT = O.step(np.tile(Ts, (len(acts), 1)), 1, t[acts], 9, k, 100)
        assert np.array_equal(st, stT) and np.array_equal(npl, nplT) and np.array_equal(c, cT), k
        for j in range(len(acts)):
            if st[j] == 0:
                assert _sorted_form(o[j]) == _sorted_form(oT[j]), (k, int(acts[j]))
        moved += int((t[acts] != acts).sum())
    assert len(idx) > 100 and moved > 100


def test_bid_steps_commute_with_the_group_swap(pool):
    """Bid states of rounds 2-12 under GROUPS, all 202 bids: step(T s, A a) is the group swap of step(s, a) -
    state, status, next player and stream counter (ties draw from the same stream)."""
    idx = [k for k in range(len(pool)) if not (int(pool[k, 0]) >> 4) & 1 and 2 <= int(pool[k, 0]) & 0xF <= 12]
    plans = _plans(pool, R.GROUPS)
    acts = np.arange(R.NBID, dtype=np.int32)
    swapped = resolved = 0
    for k in idx:
        p = plans[k]
        t = R.action_table(pool[k], p)
        Ts = R.transform_state(pool[k], p)
        o, npl, st, c = O.step(np.tile(pool[k], (R.NBID, 1)), 1, acts, 9, k, 100)
        oT, nplT, stT, cT = O.step(np.tile(Ts, (R.NBID, 1)), 1, t[acts], 9, k, 100)
        assert np.array_equal(st, stT) and np.array_equal(npl, nplT) and np.array_equal(c, cT), k
        good = st == 0
        want = np.array([R.transform_state(x, p) for x in o], dtype=np.uint64)
        assert np.array_equal(want[good], oT[good]), k
        swapped += p["swap"]
        resolved += int(((o[good, 0] >> np.uint64(4)) & np.uint64(1)).sum())
    assert len(idx) > 50 and 10 < swapped < len(idx) and resolved > 1000


def test_fisher_yates_is_uniform_on_three():
    """The six orders of a list of three over 6,000 example indices: each count within 5 sigma of 1,000."""
    counts = {}
    for k in range(6000):
        key = tuple(R.fisher_yates(3, R.BASE_P1, k, KEY, SEED))
        counts[key] = counts.get(key, 0) + 1
    sigma = math.sqrt(6000 * (1 / 6) * (5 / 6))
    print(sorted(counts.items()), f"sigma {sigma:.1f}")
    assert len(counts) == 6
    assert all(abs(c - 1000) <= 5 * sigma for c in counts.values())


def test_draws_are_off_the_game_and_noise_streams():
    from oracle import spec
    x = spec.philox4x32_10(5, 9, KEY, 0x40000000, SEED & R.M32, SEED >> 32)
    assert R.x1(5, 9, KEY, SEED) == x[1] and R.below(5, 7, 9, KEY, SEED) == (x[1] * 7) >> 32
    assert x[:2] != spec.philox4x32_10(5, 9, KEY, 0, SEED & R.M32, SEED >> 32)[:2]
    assert R.x1(5, 9 + 2 ** 32, KEY, SEED) == R.x1(5, 9, KEY, SEED)  # k & 0xffffffff


def test_restatement_orders_rows_and_keeps_values():
    H = R.hand_states()[[6, 2]]  # 10 dice in the score phase; a bid state
    cols = np.array([202 + 251, 202 + 252 * 3 + 7, 202, 5, 0, 150, 201], dtype=np.int32)
    order = np.argsort(cols[:3])
    cols[:3] = cols[:3][order]
    indptr = np.array([0, 3, 7], dtype=np.int64)
    vals = np.arange(1, 8, dtype=np.float64) / 8
    for key in range(6):
        s, t, c, v = R.augment(H, np.array([202 + 17, 150], dtype=np.int32), indptr, cols, vals, SEED, key, ALL, 40)
        for k in range(2):
            p = R.plan(H[k], 40 + k, key, SEED, ALL)
            a0, a1 = indptr[k], indptr[k + 1]
            assert (np.diff(c[a0:a1]) > 0).all()
            assert {(R.map_action(a, H[k], p), x) for a, x in zip(cols[a0:a1], vals[a0:a1])} == set(zip(c[a0:a1], v[a0:a1]))
            assert np.array_equal(s[k], R.transform_state(H[k], p))
        assert t[0] == R.map_action(202 + 17, H[0], R.plan(H[0], 40, key, SEED, ALL))


# ---------------------------------------------------------------- ABI and knob
def test_augment_is_exported_and_bound():
    import yacht_amd
    from yacht_amd import _lib, kernels, replay
    assert hasattr(yacht_amd.lib(), "yk_examples_augment")
    P = C.c_void_p
    assert _lib.SIGNATURES["yk_examples_augment"] == [P, P, P, P, P, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32,
                                                      C.c_int, P, P, P, P, P]
    assert replay.augment_examples is kernels.augment_examples
    assert kernels.symmetry_flags(()) == 0 and kernels.symmetry_flags(["groups", "carry"]) == 5
    assert kernels.symmetry_flags(("carry", "rolls", "groups")) == ALL == 7
    assert {k: kernels.SYMMETRIES[k] for k in R.FLAG_OF} == R.FLAG_OF


def test_augment_rejects_bad_arguments_without_a_gpu():
    """n < 0, flags outside 0..7, half-given pairs, NULL states / out_states with n > 0: YK_ERR_ARG, decided
    before anything touches the device (the pointers here point nowhere)."""
    import yacht_amd
    f = yacht_amd.lib().yk_examples_augment
    s, t, ip, co, va, os_, ot, oc, ov = (0x1000 * (i + 1) for i in range(9))

    def call(states=s, targets=t, indptr=ip, cols=co, vals=va, n=4, flags=7, out_states=os_, out_targets=ot,
             out_cols=oc, out_vals=ov):
        return f(states, targets, indptr, cols, vals, n, 0, 1, 0, flags, out_states, out_targets, out_cols, out_vals, None)

    assert call(n=-1) == -1
    for flags in (-1, 8, 1 << 30):
        assert call(flags=flags) == -1
    assert call(targets=None) == -1 and call(out_targets=None) == -1
    for name in ("indptr", "cols", "vals", "out_cols", "out_vals"):
        assert call(**{name: None}) == -1, name
    assert call(indptr=None, cols=None, vals=None) == -1 and call(out_cols=None, out_vals=None) == -1
    assert call(states=None) == -1 and call(out_states=None) == -1
    assert call(out_states=s) == -1  # out must not alias in
    assert call(n=0) == 0 and call(n=0, states=None, out_states=None, targets=None, out_targets=None) == 0


def test_train_rejects_an_unknown_symmetry_before_any_device_work():
    from yacht_amd import kernels, nnet
    from yacht_amd.utils import dotdict
    for bad in (("carry", "mirror"), "mirror", ["Carry"]):
        with pytest.raises(ValueError, match="unknown symmetry"):
            kernels.symmetry_flags(bad)
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=32, vloss_weight=1.5, cuda=True, hidden=64,
                   nblocks=1, dropout=0.0, seed=6, symmetries=("carry", "mirror"))
    game = type("Game", (), {"getActionSize": lambda self: R.ASIZE})()
    w = nnet.NNetWrapper(game, args)
    with pytest.raises(ValueError, match="unknown symmetry 'mirror'"):
        w.train([], verbose=False)
    assert getattr(w, "_tr", None) is None  # no trainer (no device buffer) was made
