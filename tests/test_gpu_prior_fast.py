"""The expansion's compact-first prior: a leaf whose valid actions span a small
window of the action row (every bid node, a 10-dice node whose unused categories lie close together), or a
5-dice node (one action per unused category), computes each unnormalised prior once, in compact order,
stages it in LDS and feeds numpy's pairwise sum and the P write from there.  The sum adds the same
operands in the same order, so everything must be what the dense pass gives, bit for bit:
YK_PRIOR_FAST=0 sends every leaf through the dense pass."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")
PATHS = ("prior_window", "prior_sparse", "prior_general")
NBID, NCOMB, NCAT, ASIZE = 202, 252, 12, 3226
WCAP = 2048  # PF_WCAP (yk_engine_dev.h): floats of the per-wave window


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


def _check_switch(off, on):
    (r0, s0, _), (r1, s1, _) = off, on
    print({k: s1[k] for k in PATHS}, "expansions", s1["expansions"])
    for k in ("expansions", "path_edges", "scanned", "scan_edges"):
        assert s1[k] == s0[k], k
    for k in FIELDS:
        assert np.array_equal(r1[k], r0[k]), k
    assert all(s1[k] > 0 for k in PATHS), s1
    assert sum(s1[k] for k in PATHS) == s1["expansions"]
    assert s0["prior_window"] == 0 and s0["prior_sparse"] == 0 and s0["prior_general"] == s0["expansions"], s0


@pytest.mark.parametrize("prior,sims", [("hash", 40), ("hash", 200), ("net", 25)])
def test_prior_fast_equals_dense_pass(Y, net, prior, sims):
    """Full 48-move episodes of 192 games: identical records and counters with the switch off and on, every
    path taken with it on, only the general one with it off."""
    _, E, _ = Y
    _check_switch(*(_run(E, 192, sims, prior, net, 707, 900, mode) for mode in ("0", None)))


def test_prior_fast_recorded_predictions_equal(Y):
    """record_predictions on (every 48th game): the recorded Ps * valids rows and v are the dense pass's."""
    _, E, _ = Y
    off, on = (_run(E, 192, 40, "hash", None, 707, 900, mode, record_predictions=True, record_stride=48)
               for mode in ("0", None))
    _check_switch(off, on)
    (pi0, v0, c0), (pi1, v1, c1) = off[2], on[2]
    assert np.array_equal(c1, c0) and (c0 > 0).all() and (c0 <= pi0.shape[1]).all()
    for r, n in enumerate(c0):  # (the slots past a game's count were never written)
        assert np.array_equal(pi1[r, :n], pi0[r, :n]) and np.array_equal(v1[r, :n], v0[r, :n]), r


def test_prior_fast_two_groups_equal_one(Y, net):
    """Two game groups on their own streams, the path on: the records of one group."""
    _, E, _ = Y
    (r1, s1, _), (r2, s2, _) = (_run(E, 32, 25, "net", net, 515, 300, None, groups=g) for g in (1, 2))
    assert s1["groups"] == 1 and s2["groups"] == 2
    assert s2["expansions"] == s1["expansions"]
    assert s2["prior_window"] > 0 and s2["prior_sparse"] > 0
    for k in FIELDS:
        assert np.array_equal(r2[k], r1[k]), k


# ---------------------------------------------------------------- window edges, from crafted roots
def _root(kind, cats):
    """A canonical root whose player to move has the unused categories `cats`: a 10-dice or a 5-dice score
    node, or a bid node.  The other player holds 10 dice and all 12 categories, so the root's child (the
    second simulation's expansion) is a full-width leaf on the general path - a bid root's child is the
    other player's bid node."""
    from yacht_amd.state import PHASE_BID, PHASE_SCORE, PlayerState, YachtState, pack
    used = 0xFFF & ~sum(1 << c for c in cats)
    other = PlayerState(carry=[6, 5, 4, 3, 2, 1, 6, 5, 4, 3], used_mask=0)
    if kind == "bid":
        s = YachtState(round_no=3, phase=PHASE_BID, rollA=[1, 2, 3, 4, 5], rollB=[2, 2, 3, 3, 6],
                       p1=PlayerState(carry=[1, 1, 2, 3, 4], used_mask=1), p2=PlayerState(carry=[6, 6, 5, 4, 3], used_mask=2))
    elif kind == "ten":
        s = YachtState(round_no=5, phase=PHASE_SCORE, p1=PlayerState(carry=[1, 2, 3, 4, 5, 6, 1, 2, 3, 4], used_mask=used),
                       p2=other)
    else:
        s = YachtState(round_no=13, phase=PHASE_SCORE, p1=PlayerState(carry=[1, 3, 3, 4, 6], used_mask=used), p2=other)
    return pack(s)


def _valid(kind, cats):
    if kind == "bid":
        return np.arange(NBID)
    if kind == "ten":
        return np.concatenate([NBID + NCOMB * c + np.arange(NCOMB) for c in cats])
    return np.array([NBID + NCOMB * c for c in cats])


def _path(kind, cats):
    """The path the root's expansion takes by the rule of DESIGN.md 6b."""
    if kind == "five":
        return "prior_sparse"
    a = _valid(kind, cats)
    base = int(a[0]) & ~7
    return "prior_window" if ((int(a[-1]) + 1 - base + 7) & ~7) <= WCAP else "prior_general"


ALL = tuple(range(NCAT))
# The largest span a state can have inside the window is eight adjacent categories: 2016 actions, 2024
# floats from the 8-aligned base (category starts are 2 or 6 mod 8) - no state spans exactly WCAP.  One
# category more, 2276 floats, must fall to the general path.
CASES = [("ten", (c,), "prior_window") for c in range(NCAT)] + [  # category 11 ends at the row's end, action 3225
    ("ten", (4, 5), "prior_window"),                  # an adjacent pair
    ("ten", (3, 5), "prior_window"),                  # a non-adjacent pair: a used category of zeros between
    ("ten", tuple(range(0, 8)), "prior_window"),      # the largest span that fits, from the first category
    ("ten", tuple(range(4, 12)), "prior_window"),     # the same up to the row's end
    ("ten", (1, 8), "prior_window"),                  # the same span with six used categories inside
    ("ten", tuple(range(0, 9)), "prior_general"),     # that span plus one category
    ("ten", tuple(range(3, 12)), "prior_general"),
    ("ten", (0, 8), "prior_general"),
    ("ten", ALL, "prior_general"),
    ("five", (7,), "prior_sparse"),
    ("five", (0,), "prior_sparse"),
    ("five", (11,), "prior_sparse"),
    ("five", ALL, "prior_sparse"),
    ("bid", (), "prior_window"),
]


@pytest.fixture(scope="module")
def searchers(Y, net):
    """One-game engines (2 simulations, predictions recorded) per prior, with the switch off and on."""
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
    yk, _, _ = Y
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


@pytest.mark.parametrize("prior", ["hash", "net"])
@pytest.mark.parametrize("kind,cats,path", CASES)
def test_window_edges(Y, searchers, prior, kind, cats, path):
    """The root's expansion is the code under test.  Outputs equal with the switch off and on; the stored P is
    the recorded row over numpy's own pairwise sum of it; the expansion takes the path named for the case."""
    assert _path(kind, cats) == path
    root = _root(kind, cats)
    off = _search(Y, searchers[prior, "0"], root)
    on = _search(Y, searchers[prior, None], root)
    for k in ("counts", "ctr", "P", "pi", "v", "cnt"):
        assert np.array_equal(on[k], off[k]), k
    assert on["cnt"] == 2 and on["st"]["expansions"] == 2
    # the recorded row: Ps * valids of the root
    row = on["pi"][0]
    valid = _valid(kind, cats)
    mask = np.zeros(ASIZE, dtype=bool)
    mask[valid] = True
    assert row.dtype == np.float32 and (row[~mask] == 0).all() and np.sum(row) > 0
    if prior == "hash":  # (the hash prior is positive everywhere; a softmax may round to 0)
        assert (row[mask] > 0).all()
    assert np.array_equal(on["P"], row / np.sum(row))  # float32 throughout; np.sum is the pairwise sum
    # the paths: the root's, then its child's (a bid root's child is a bid node, any other's a full-width leaf)
    child = "prior_window" if kind == "bid" else "prior_general"
    want = {k: (k == path) + (k == child) for k in PATHS}
    assert {k: on["st"][k] for k in PATHS} == want
    assert {k: off["st"][k] for k in PATHS} == {"prior_window": 0, "prior_sparse": 0, "prior_general": 2}
