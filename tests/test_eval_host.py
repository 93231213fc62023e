"""Held-out evaluation, host side: the numpy restatement tests/eval_ref.py on rows
whose numbers are known in closed form, its summation order against math.fsum, and every argument check
that needs no device - the C entry points' YK_ERR_ARG paths, YkNet.evaluate's shapes, the policy target's
name, Coach's holdoutEps."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import eval_ref as R
from conftest import GOLDEN
from oracle import oracle as O

A = R.ASIZE


@pytest.fixture(scope="module")
def boards():
    """Three boards of tests/golden/states.npz - a bid phase, a score phase with a 5-dice and one with a
    10-dice carry - and their valid masks for player 1."""
    S = np.load(os.path.join(GOLDEN, "states.npz"))["states"]
    phase = (S[:, 0] >> np.uint64(4)) & np.uint64(1)
    carry = (S[:, 1] >> np.uint64(40)) & np.uint64(0xF)
    pick = [int(np.nonzero(phase == 0)[0][0]), int(np.nonzero((phase == 1) & (carry == 5))[0][0]),
            int(np.nonzero((phase == 1) & (carry == 10))[0][0])]
    W = S[pick]
    ok = O.valid(W, 1)[0].astype(bool)
    assert ok[0, :202].all() and not ok[0, 202:].any() and ok[1:, 202:].any(1).all()
    return W, ok


def test_all_logits_equal(boards):
    _, ok = boards
    for t in (0, 7, 3225):
        x = np.full((3, 3264), 2.5, dtype=np.float32)
        r = R.rows(x, np.zeros(3, np.float32), ok, [t] * 3, np.zeros(3, np.float32))
        assert np.allclose(r[:, 0], 2.5 + math.log(A), rtol=0, atol=1e-12)
        assert np.allclose(r[:, 1], math.log(A), rtol=0, atol=1e-12)
        assert np.allclose(r[:, 3], math.log(A), rtol=0, atol=1e-12)
        assert (r[:, 2] == t).all()  # every lower index ties and comes first
        assert np.allclose(r[:, 4], ok.sum(1) / A, rtol=1e-12, atol=0)
        assert (r[:, 12] == (t == 0)).all() and (r[:, 13] == (t < 5)).all()
        assert not r[:, 5:8].any() and (r[:, 14] == 0).all() and (r[:, 15] == 1).all()


def test_tie_at_the_maximum(boards):
    _, ok = boards
    x = np.zeros((2, 3226), dtype=np.float32)
    x[:, [100, 2000]] = 9.0
    r = R.rows(x, np.array([0.5, -0.5], np.float32), ok, [100, 2000], np.array([1.0, 1.0], np.float32))
    assert list(r[:, 2]) == [0.0, 1.0] and list(r[:, 12]) == [1.0, 0.0] and list(r[:, 13]) == [1.0, 1.0]
    lse = 9.0 + math.log(2.0 + (A - 2) * math.exp(-9.0))
    assert np.allclose(r[:, 0], lse, rtol=0, atol=1e-12) and np.allclose(r[:, 1], lse - 9.0, rtol=0, atol=1e-12)
    assert list(r[:, 8]) == [0.5, -0.5] and list(r[:, 9]) == [-0.5, -1.5] and list(r[:, 10]) == [0.25, 2.25]
    assert list(r[:, 11]) == [1.0, 0.0]


def test_csr_rows_and_targets_outside(boards):
    _, ok = boards
    rng = np.random.default_rng(5)
    x = rng.normal(size=(3, 3226)).astype(np.float32)
    indptr = np.array([0, 0, 2, 5], dtype=np.int64)  # row 0 empty
    cols = np.array([3, 3225, 0, 9, 4000], dtype=np.int32)  # (a column outside: skipped by the soft CE only)
    vals = np.array([0.25, 0.75, 0.5, 0.0, 0.25])
    r = R.rows(x, np.zeros(3, np.float32), ok, [-1, 3226, 5], np.zeros(3, np.float32), csr=(indptr, cols, vals))
    assert not r[0, 5:8].any()
    assert list(r[:, 14]) == [1.0, 1.0, 0.0] and list(r[:2, 1]) == [0.0, 0.0] and list(r[:2, 2]) == [A, A]
    assert not r[:2, 12:14].any()
    xd = x.astype(np.float64)
    assert r[1, 5] == 1.0 and r[2, 5] == 0.75
    assert math.isclose(r[1, 6], 0.25 * (r[1, 0] - xd[1, 3]) + 0.75 * (r[1, 0] - xd[1, 3225]), rel_tol=1e-14)
    assert math.isclose(r[2, 6], 0.5 * (r[2, 0] - xd[2, 0]), rel_tol=1e-14)
    assert math.isclose(r[1, 7], -(0.25 * math.log(0.25) + 0.75 * math.log(0.75)), rel_tol=1e-14)
    assert math.isclose(r[2, 7], -(0.5 * math.log(0.5) + 0.25 * math.log(0.25)), rel_tol=1e-14)
    # the gather: row i of the logits belongs to example batch_idx[i]
    idx = np.array([2, 0, 2], dtype=np.int32)
    g = R.rows(x[idx], np.zeros(3, np.float32), ok, [-1, 3226, 5], np.zeros(3, np.float32), csr=(indptr, cols, vals),
               batch_idx=idx)
    assert np.array_equal(g, r[idx])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_sums_order_stays_within_the_worst_case_bound(n):
    """Any order of n additions is within n 2^-53 sum|terms| of the exact sum (math.fsum)."""
    rng = np.random.default_rng(n)
    rows = rng.normal(size=(n, 16)) * np.exp(rng.uniform(-20, 20, size=(n, 16)))
    got = R.sums(rows)
    for c in range(16):
        exact = math.fsum(rows[:, c])
        assert abs(got[c] - exact) <= n * 2.0 ** -53 * math.fsum(np.abs(rows[:, c])), c
    # the order itself, on a column where it shows: 2^53 then ones - row by row every 1 would be lost
    col = np.zeros((600, 16))
    col[0, 0], col[1:, 0] = 2.0 ** 53, 1.0
    seq = 0.0
    for p in [sum(col[j::256, 0].tolist(), 0.0) for j in range(256)]:  # (sum of a list: left to right)
        seq = seq + p
    assert R.sums(col)[0] == seq and seq > 2.0 ** 53 + 500


# ------------------------------------------------------------------ the binding and the C argument checks
def test_binding_and_exports():
    import yacht_amd
    from yacht_amd import _lib
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["yk_net_logits"] == [P, P, P, P, I, P]
    assert _lib.SIGNATURES["yk_examples_metrics"] == [P, L, P, P, P, P, P, P, P, P, L, P, P, P]
    assert _lib.SIGNATURES["yk_net_evaluate"] == [P, P, P, P, P, P, P, P, L, I, P, P, P]
    lib = C.CDLL(yacht_amd.LIB_PATH)
    assert all(hasattr(lib, f) for f in ("yk_net_logits", "yk_examples_metrics", "yk_net_evaluate"))


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    import yacht_amd
    lib = yacht_amd.lib()
    buf = (C.c_char * 256)()  # (never read: the arguments are checked first)
    b = C.addressof(buf)
    sums = (C.c_double * 16)(*([7.0] * 16))
    m, e, lg = lib.yk_examples_metrics, lib.yk_net_evaluate, lib.yk_net_logits
    ok_m = [b, 3264, b, b, b, b, None, None, None, None, 4, None, sums, None]
    ok_e = [b, b, b, b, None, None, None, None, 4, 0, None, sums, None]

    def bad(f, good, pos, value):
        a = list(good)
        a[pos] = value
        return f(*a)
    for pos in (0, 2, 3, 4, 5, 12):  # a NULL required pointer
        assert bad(m, ok_m, pos, None) == -1, pos
    assert bad(m, ok_m, 1, 3225) == -1 and bad(m, ok_m, 10, -1) == -1  # ld < 3226, n < 0
    for pos in (0, 1, 2, 3, 11):
        assert bad(e, ok_e, pos, None) == -1, pos
    assert bad(e, ok_e, 8, -1) == -1
    for given in ((6,), (7,), (8,), (6, 7), (7, 8), (6, 8)):  # a half-given CSR
        a = list(ok_m)
        for pos in given:
            a[pos] = b
        assert m(*a) == -1, given
        a = list(ok_e)
        for pos in given:
            a[pos - 2] = b
        assert e(*a) == -1, given
    assert lg(None, b, b, b, 4, None) == -1 and lg(b, None, b, b, 4, None) == -1
    assert lg(b, b, None, b, 4, None) == -1 and lg(b, b, b, None, 4, None) == -1 and lg(b, b, b, b, -1, None) == -1
    assert list(sums) == [7.0] * 16  # nothing was written
    # n == 0: YK_OK, sums all zero, no device call
    assert bad(m, ok_m, 10, 0) == 0 and list(sums) == [0.0] * 16
    sums[:] = [7.0] * 16
    assert bad(e, ok_e, 8, 0) == 0 and list(sums) == [0.0] * 16
    assert lg(b, b, b, b, 0, None) == 0


# ------------------------------------------------------------------ the Python layers
def test_eval_summary():
    from yacht_amd.nnet import eval_summary
    s = [0.0] * 16
    s[1], s[3], s[4], s[5], s[6], s[7], s[9], s[10], s[11], s[12], s[13], s[14], s[15] = \
        8.0, 6.0, 3.0, 2.0, 10.0, 4.0, -2.0, 1.0, 3.0, 1.0, 2.0, 1.0, 4.0
    d = eval_summary(s, soft=True)
    assert d == dict(n=4, bad_targets=1, policy_ce=2.0, top1=0.25, top5=0.5, policy_entropy=1.5, valid_mass=0.75,
                     policy_ce_soft=2.5, target_entropy=1.0, policy_kl=3.0, value_mse=0.25, value_bias=-0.5,
                     value_sign_acc=0.75)
    h = eval_summary(s, soft=False)
    assert h["policy_ce_soft"] is None and h["target_entropy"] is None and h["policy_kl"] is None
    assert {k: v for k, v in h.items() if v is not None} == {k: v for k, v in d.items() if k in h and h[k] is not None}
    z = eval_summary([0.0] * 16, soft=True)  # no rows: NaN means, no exception
    assert z["n"] == 0 and z["bad_targets"] == 0
    assert all(math.isnan(z[k]) for k in z if k not in ("n", "bad_targets"))


def test_evaluate_argument_checks_need_no_device():
    torch = pytest.importorskip("torch")
    from yacht_amd.nnet import check_eval_args
    st, tg, va = torch.zeros((5, 8), dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(5)
    ip, co, vl = torch.zeros(6, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float64)
    assert check_eval_args(st, tg, va, None, None, 0) is None
    assert len(check_eval_args(st, tg, va, (ip, co, vl), torch.zeros(2, dtype=torch.int32), 16)) == 3
    empty = check_eval_args(st, tg, va, (ip, co[:0], vl[:0]), None, 0)
    assert empty[1].numel() == 1 and empty[2].numel() == 1  # three real pointers even with no entry
    for bad in (dict(states=st.to(torch.int32)), dict(states=st[:, :7]), dict(targets=tg.to(torch.int64)),
                dict(targets=tg[:4]), dict(values=va.double()), dict(values=va[:4]),
                dict(idx=torch.zeros(2, dtype=torch.int64)), dict(chunk=1.5), dict(policies=(ip, co)),
                dict(policies=(ip[:5], co, vl)), dict(policies=(ip, co, vl.float())),
                dict(policies=(ip, co, vl[:2])), dict(policies=(ip, co.to(torch.int64), vl))):
        kw = dict(states=st, targets=tg, values=va, policies=None, idx=None, chunk=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_eval_args(**kw)


def test_policy_target_name_and_holdout_eps_are_checked_first():
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict

    class Game:
        def getActionSize(self):
            return A
    net = NNetWrapper(Game(), dotdict(hidden=64, nblocks=1, dropout=0.0, policy_target="visits"))
    assert net.eval_target() == "visits" and net.eval_target("argmax") == "argmax"
    with pytest.raises(ValueError, match="policy_target"):
        net.evaluate([], target="soft")  # (before the examples are looked at)
    base = dict(numMCTSSims=4, cpuct=1.5, tempThreshold=15)
    with pytest.raises(ValueError, match="holdoutEps"):
        Coach(None, None, dotdict(base, holdoutEps=-1))
    from yacht_amd.game import YachtGame
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(base))
    assert c.holdout_eps == 0 and c.holdoutHistory == [] and c.eval_history == [] and c.last_eval is None
    assert Coach(YachtGame(seed=1, env_id=0), object(), dotdict(base, holdoutEps=3)).holdout_eps == 3
