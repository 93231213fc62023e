"""A general leaf's priors at 10 dice, compact-first and four entries per lane: its
q / qt are filled through the per-wave window in the two pieces of the staged P write - zeros, then one
category's four consecutive actions per lane (two 8-byte loads of the logits row, two 8-byte window writes),
then each lane's leaf of numpy's pairwise tree read back - so the leaf pays an exp per valid action where the
dense pass evaluates 52 per lane.  Each prior is the same expression on the same operands and the window is
zero where the dense pass writes 0, so everything must be bit for bit what YK_PRIOR_FAST=0 (every leaf
through the dense pass and the gather write) and YK_PRIOR_FAST=2 (the previous default: the dense pass for
general leaves, then the staged write) give.  The window class at 10 dice keeps its one-entry loops (four per
lane there measured no gain); its cases stay here against level 0, next to the general ones."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
PATHS = ("prior_window", "prior_sparse", "prior_general")
NBID, NCOMB, NCAT, ASIZE = 202, 252, 12, 3226
WCAP = 2048   # PF_WCAP (yk_engine_dev.h): floats of the per-wave window
SPLIT = 1608  # where numpy's pairwise tree for 3226 splits at its root: category 5's combination 146
LEVELS = ("0", "2", None)


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


class _Env:
    """YK_PRIOR_FAST as the engine reads it at creation; restored on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get("YK_PRIOR_FAST")
        if self.mode is None:
            os.environ.pop("YK_PRIOR_FAST", None)
        else:
            os.environ["YK_PRIOR_FAST"] = self.mode

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("YK_PRIOR_FAST", None)
        else:
            os.environ["YK_PRIOR_FAST"] = self.old


def _run(E, n, sims, prior, net, seed, base, mode, **kw):
    with _Env(mode):
        eng = E.SelfPlayEngine(n, sims, 1.5, 15, net=net if prior == "net" else None, prior=prior, max_moves=48, **kw)
    eng.run(seed, base)
    st = eng.stats()
    rec = eng.records()
    pred = eng.predictions() if kw.get("record_predictions") else None
    eng.close()
    assert st["errors"] == 0, st
    return rec, st, pred


def _check_levels(runs):
    """runs: (records, stats, predictions) of YK_PRIOR_FAST = 0, 2 and unset, in that order."""
    (r0, s0, _), (r2, s2, _), (r3, s3, _) = runs
    print({k: s3[k] for k in PATHS}, "expansions", s3["expansions"])
    for r, s in ((r2, s2), (r3, s3)):
        for k in ("expansions", "path_edges", "scanned", "scan_edges"):
            assert s[k] == s0[k], k
        for k in FIELDS:
            assert np.array_equal(r[k], r0[k]), k
        assert sum(s[k] for k in PATHS) == s["expansions"]
    assert s3["prior_window"] > 0 and s3["prior_general"] > 0, s3
    assert {k: s3[k] for k in PATHS} == {k: s2[k] for k in PATHS}  # a leaf's class counter does not move


def test_quad_priors_equal_dense_pass_hash_recorded(Y):
    """Full 48-move episodes of 192 games, hash prior, 40 simulations, record_predictions on (every 48th game):
    identical records, counters and recorded Ps * valids rows and v at the three levels of the switch (equal
    records prove first_j too: the later descents take it)."""
    _, E, _ = Y
    runs = [_run(E, 192, 40, "hash", None, 707, 900, mode, record_predictions=True, record_stride=48)
            for mode in LEVELS]
    _check_levels(runs)
    pi0, v0, c0 = runs[0][2]
    assert (c0 > 0).all() and (c0 <= pi0.shape[1]).all()
    for _, _, (pi, v, c) in runs[1:]:
        assert np.array_equal(c, c0)
        for r, n in enumerate(c0):  # (the slots past a game's count were never written)
            assert np.array_equal(pi[r, :n], pi0[r, :n]) and np.array_equal(v[r, :n], v0[r, :n]), r


def test_quad_priors_equal_dense_pass_net(Y, net):
    """The same episodes with the net prior, 25 simulations."""
    _, E, _ = Y
    _check_levels([_run(E, 192, 25, "net", net, 707, 900, mode) for mode in LEVELS])


@pytest.mark.parametrize("kw", [dict(fpu_reduction=0.25), dict(forced_playouts_k=2.0)], ids=["fpu", "forced"])
def test_quad_priors_in_the_other_instantiations(Y, net, kw):
    """First-play urgency and forced playouts run their own instantiations of the expansion kernel around the
    one shared expansion (other registers around it): 64 games x 10 simulations, the default against level 0,
    records identical."""
    _, E, _ = Y
    (r0, s0, _), (r3, s3, _) = (_run(E, 64, 10, "net", net, 515, 300, mode, **kw) for mode in ("0", None))
    assert s3["expansions"] == s0["expansions"] and s3["prior_window"] > 0 and s3["prior_general"] > 0, s3
    for k in FIELDS:
        assert np.array_equal(r3[k], r0[k]), k


# ---------------------------------------------------------------- crafted roots: both classes, around the split
ALL = tuple(range(NCAT))
# (carry of the player to move, its unused categories, the class of the root by the rule of 6b)
WINDOW_CASES = [
    (10, tuple(range(0, 8))),   # eight adjacent categories from the first: the widest window (2024)
    (10, tuple(range(4, 12))),  # and up to the last action of the row
    (10, (2, 5, 9)),            # zeros between the categories
    (10, (5,)),                 # one category, the one the tree's split at 1608 cuts
    (10, (0, 7)),
    (10, (11,)),
]
WINDOW_WLEN = [2024, 2024, 2024, 264, 2024, 264]
GENERAL_CASES = [
    (10, ALL),
    (10, tuple(range(0, 9))),
    (10, tuple(range(3, 12))),
    (10, (0, 8)),
    (10, (0, 5, 9)),           # category 5 unused: 252 + 146 entries below the split, the cut group in both pieces
    (10, (0, 1, 2, 3, 4, 9)),  # category 5 used: the entries below the split end on a category's edge
    (10, (2, 5, 11)),
    (7, ALL),                  # the table class (21 of a category's 252 combinations valid): the dense pass stays
    (10, (0, 11)),             # the two ends of the row, ten categories of zeros between them
    (10, (0, 5, 11)),
]


def _root(ndice, cats):
    """A canonical score-phase root whose player to move holds `ndice` dice and the unused categories `cats`.
    The other player holds 10 dice and all 12 categories, so the root's child (the second simulation's
    expansion) is a full-width leaf on the general path."""
    from yacht_amd.state import PHASE_SCORE, PlayerState, YachtState, pack
    used = 0xFFF & ~sum(1 << c for c in cats)
    other = PlayerState(carry=[6, 5, 4, 3, 2, 1, 6, 5, 4, 3], used_mask=0)
    carry = [1, 2, 3, 4, 5, 6, 1, 2, 3, 4][:ndice]
    return pack(YachtState(round_no=5, phase=PHASE_SCORE, p1=PlayerState(carry=carry, used_mask=used), p2=other))


def _valid(root, ndice, cats):
    """The root's valid actions by the CPU oracle (getValidMoves); for 10 dice also by the closed form."""
    m, cnt = O.valid(np.asarray(root).reshape(1, -1), [1])
    a = np.flatnonzero(m[0])
    assert len(a) == int(cnt[0])
    if ndice == 10:
        assert np.array_equal(a, np.concatenate([NBID + NCOMB * c + np.arange(NCOMB) for c in cats]))
    else:
        assert 0 < len(a) < NCOMB * len(cats) and len(a) % len(cats) == 0
        assert set((a - NBID) // NCOMB) == set(cats)
    return a


def _wlen(valid):
    """The window a leaf's valid actions span, by the rule of 6b."""
    base = int(valid[0]) & ~7
    return (int(valid[-1]) + 1 - base + 7) & ~7


@pytest.fixture(scope="module")
def searchers(Y, net):
    """One-game engines (2 simulations, predictions recorded) per prior, at level 0 and at the default."""
    _, E, _ = Y
    out = {}
    for prior in ("hash", "net"):
        for mode in ("0", None):
            with _Env(mode):
                out[prior, mode] = E.SelfPlayEngine(1, 2, 1.5, net=net if prior == "net" else None, prior=prior,
                                                    max_moves=1, record_predictions=True)
    yield out
    for e in out.values():
        e.close()


def _search(Y, eng, root):
    """Two simulations from `root` on a fresh tree: the first expands the root, the second its child."""
    from yacht_amd import kernels as K
    from yacht_amd._lib import call
    call("yk_mcts_reset", eng.handle)
    roots = K.states_to_device(root)
    env = torch.tensor([5], dtype=torch.int32, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = torch.zeros((1, ASIZE), dtype=torch.int32, device="cuda")
    call("yk_mcts_search", eng.handle, roots.data_ptr(), 99, env.data_ptr(), ctr.data_ptr(), 2, counts.data_ptr(), None)
    torch.cuda.synchronize()
    P = np.zeros(ASIZE, dtype=np.float32)
    call("yk_engine_root_prior", eng.handle, 0, P.ctypes.data_as(C.c_void_p))
    pi, v, cnt = eng.predictions()
    st = eng.stats()
    assert st["errors"] == 0, st
    return dict(counts=counts.cpu().numpy(), ctr=int(ctr.item()), P=P, pi=pi[0, :2].copy(), v=v[0, :2].copy(),
                cnt=int(cnt[0]), st=st)


def _check_root(Y, searchers, prior, root, valid, want):
    """Outputs equal at level 0 and at the default; the stored P is the recorded row over numpy's own pairwise
    sum of it, an IEEE float32 division per entry; the row is zero off the valid set; the path counters are
    `want` at the default."""
    off = _search(Y, searchers[prior, "0"], root)
    on = _search(Y, searchers[prior, None], root)
    for k in ("counts", "ctr", "P", "pi", "v", "cnt"):
        assert np.array_equal(on[k], off[k]), k
    assert on["cnt"] == 2 and on["st"]["expansions"] == 2
    row = on["pi"][0]  # the recorded row: Ps * valids of the root
    mask = np.zeros(ASIZE, dtype=bool)
    mask[valid] = True
    assert row.dtype == np.float32 and (row[~mask] == 0).all() and np.sum(row) > 0
    if prior == "hash":  # (the hash prior is positive everywhere; a softmax may round to 0)
        assert (row[mask] > 0).all()
    assert np.array_equal(on["P"], row / np.sum(row))  # float32 throughout; np.sum is the pairwise sum
    assert {k: on["st"][k] for k in PATHS} == want
    assert {k: off["st"][k] for k in PATHS} == {"prior_window": 0, "prior_sparse": 0, "prior_general": 2}


@pytest.mark.parametrize("prior", ["hash", "net"])
@pytest.mark.parametrize("case", range(len(WINDOW_CASES)))
def test_window_leaves_at_ten_dice(Y, searchers, prior, case):
    """The root is a window-class score node at 10 dice (its own window, one entry per lane: undisturbed by the
    general leaves' use of the same window); its child is a full-width general leaf, compact-first."""
    ndice, cats = WINDOW_CASES[case]
    root = _root(ndice, cats)
    valid = _valid(root, ndice, cats)
    assert _wlen(valid) == WINDOW_WLEN[case] <= WCAP
    _check_root(Y, searchers, prior, root, valid, {"prior_window": 1, "prior_sparse": 0, "prior_general": 1})


@pytest.mark.parametrize("prior", ["hash", "net"])
@pytest.mark.parametrize("ndice,cats", GENERAL_CASES)
def test_general_leaves_compact_first(Y, searchers, prior, ndice, cats):
    """The root is a general leaf with valid actions on both sides of the split (at 10 dice the code under test:
    q / qt through the window in two pieces; at 7 dice the dense pass, kept); its child is a second, full-width
    general leaf."""
    root = _root(ndice, cats)
    valid = _valid(root, ndice, cats)
    assert _wlen(valid) > WCAP
    assert valid[0] < SPLIT <= valid[-1]
    _check_root(Y, searchers, prior, root, valid, {"prior_window": 0, "prior_sparse": 0, "prior_general": 2})
