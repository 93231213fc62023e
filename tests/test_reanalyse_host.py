"""Reanalysis, the parts that need no GPU: the knobs are checked before anything
touches the device, the C entry points exist and reject bad arguments without a device call, and the numpy
restatement tests/reanalyse_ref.py - which the device only has to equal - is itself checked: the splice's
identities, from-counts on rows known by hand, and the selection's statistics."""
import ctypes as C
import math

import numpy as np
import pytest

import reanalyse_ref as RR

A = RR.A
BASE = dict(numMCTSSims=4, cpuct=1.5, tempThreshold=15)


# ------------------------------------------------------------------ 1. knobs
@pytest.mark.parametrize("extra", [dict(reanalyseFraction=-0.1), dict(reanalyseFraction=1.5),
                                   dict(reanalyseFraction=float("nan")), dict(reanalyseFraction=0.5, reanalyseSims=1),
                                   dict(reanalyseSims=1), dict(reanalyseSims=0), dict(reanalyseSims=2.5),
                                   dict(reanalyseFraction=0.5, numMCTSSims=1)])
def test_bad_knobs_raise_before_any_device_call(extra):
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.replay import check_reanalyse_knobs
    from yacht_amd.utils import dotdict
    args = dotdict(BASE, **extra)
    with pytest.raises(ValueError, match="reanalyseFraction|reanalyseSims"):
        check_reanalyse_knobs(args.get("reanalyseFraction", 0.0), args.get("reanalyseSims"), args.numMCTSSims)
    with pytest.raises(ValueError, match="reanalyseFraction|reanalyseSims"):
        Coach(None, None, args)  # (nothing of the game or the net is touched before the check)


def test_knob_defaults_are_off():
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.replay import check_reanalyse_knobs
    from yacht_amd.utils import dotdict
    assert check_reanalyse_knobs() == (0.0, 0)
    assert check_reanalyse_knobs(0.0, None, 1) == (0.0, 1)  # off: numMCTSSims = 1 stays a legal configuration
    assert check_reanalyse_knobs(0.25, None, 100) == (0.25, 100)
    assert check_reanalyse_knobs(1, 7, 100) == (1.0, 7)
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE))
    assert c.reanalyse_fraction == 0.0 and c.reanalyse_sims == 4 and c.last_reanalysis is None
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE, reanalyseFraction=0.5, reanalyseSims=9))
    assert (c.reanalyse_fraction, c.reanalyse_sims) == (0.5, 9)


def test_reanalyse_checks_its_arguments_first():
    torch = pytest.importorskip("torch")
    from yacht_amd import replay
    bare = replay.ExampleShard(torch.zeros((3, 8), dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                               torch.zeros(3))
    idx = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="policies"):
        replay.reanalyse(bare, idx, prior="hash", sims=4, cpuct=1.5, seed=1, env_base=0)
    pol = dict(pi_indptr=torch.zeros(4, dtype=torch.int64), pi_cols=torch.zeros(0, dtype=torch.int32),
               pi_vals=torch.zeros(0, dtype=torch.float64), values64=torch.zeros(3, dtype=torch.float64))
    full = replay.ExampleShard(bare.states, bare.targets, bare.values, policies=pol)
    for sims in (1, 0, -3):
        with pytest.raises(ValueError, match="sims"):
            replay.reanalyse(full, idx, prior="hash", sims=sims, cpuct=1.5, seed=1, env_base=0)
    with pytest.raises(TypeError, match="idx"):
        replay.reanalyse(full, idx.long(), prior="hash", sims=4, cpuct=1.5, seed=1, env_base=0)


# ------------------------------------------------------------------ 2. the C ABI
def test_entry_points_exist_and_reject_bad_arguments_without_a_device_call():
    import yacht_amd
    from yacht_amd._lib import SIGNATURES, YK_ERR_ARG, YK_OK
    lib = yacht_amd.lib()
    for name in ("yk_reanalyse_select", "yk_policies_from_counts", "yk_policies_splice"):
        assert hasattr(lib, name) and name in SIGNATURES
    m = C.c_int64(-7)
    sel = lib.yk_reanalyse_select
    assert sel(4, 0, 1, 2, 0.5, None, 0, None, None) == YK_ERR_ARG  # no m
    for n in (-1, 2**31):
        assert sel(n, 0, 1, 2, 0.5, None, 0, C.byref(m), None) == YK_ERR_ARG
    for f in (-0.01, 1.01, float("nan"), float("inf")):
        assert sel(4, 0, 1, 2, f, None, 0, C.byref(m), None) == YK_ERR_ARG
    assert m.value == -7
    assert sel(0, 0, 1, 2, 0.5, None, 0, C.byref(m), None) == YK_OK and m.value == 0  # empty: nothing launched
    nnz = C.c_int64()
    ip = (C.c_int64 * 8)()
    p = C.cast(ip, C.c_void_p)  # (a non-null pointer; never dereferenced: the calls fail before)
    fc = lib.yk_policies_from_counts
    assert fc(None, 0, None, None, None, 0, None, C.byref(nnz), None, None) == YK_ERR_ARG  # no pi_indptr
    assert fc(None, 0, p, None, None, 0, None, None, None, None) == YK_ERR_ARG  # no nnz
    assert fc(None, 2, p, None, None, 0, None, C.byref(nnz), None, None) == YK_ERR_ARG  # no counts
    assert fc(p, -1, p, None, None, 0, None, C.byref(nnz), None, None) == YK_ERR_ARG
    assert fc(p, 2**31, p, None, None, 0, None, C.byref(nnz), None, None) == YK_ERR_ARG
    assert fc(p, 2, p, p, None, 4, None, C.byref(nnz), None, None) == YK_ERR_ARG  # pi_cols without pi_vals
    q = C.cast((C.c_int64 * 8)(), C.c_void_p)
    r = C.cast((C.c_int64 * 8)(), C.c_void_p)
    sp = lib.yk_policies_splice
    ok = [p, p, p, 2, p, 1, p, p, p, q, None, None, 0, C.byref(nnz), None]

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return sp(*a) == YK_ERR_ARG
    assert bad(a0=None) and bad(a9=None) and bad(a13=None)       # indptr, out_indptr, nnz
    assert bad(a3=-1) and bad(a3=2**31) and bad(a5=-1)           # n, m
    assert bad(a4=None) and bad(a6=None)                         # idx / new_indptr with m > 0
    assert bad(a9=p)                                             # out_indptr is an input
    assert bad(a10=r)                                            # out_cols without out_vals
    assert bad(a10=r, a11=r, a1=None) and bad(a10=r, a11=r, a7=None)  # nothing to copy from
    assert bad(a10=p, a11=r) and bad(a10=r, a11=p)               # out_cols / out_vals is an input


# ------------------------------------------------------------------ 3. the restatement
def _random_csr(rng, n, max_len):
    lens = rng.integers(0, max_len + 1, size=n)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(A, size=l, replace=False)) for l in lens] + [np.zeros(0, dtype=np.int64)])
    return ip, cols.astype(np.int32), rng.random(int(ip[-1]))


def test_splice_identities():
    rng = np.random.default_rng(3)
    old = _random_csr(rng, 37, 9)
    # no rows: the identity
    none = RR.splice(*old, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), old[1][:0], old[2][:0])
    assert all(np.array_equal(a, b) for a, b in zip(none, old))
    # all rows, every new row non-empty: the new CSR
    lens = rng.integers(1, 9, size=37)
    nip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ncols = np.concatenate([np.sort(rng.choice(A, size=l, replace=False)) for l in lens]).astype(np.int32)
    nvals = rng.random(int(nip[-1]))
    every = RR.splice(*old, np.arange(37, dtype=np.int32), nip, ncols, nvals)
    assert np.array_equal(every[0], nip) and np.array_equal(every[1], ncols) and np.array_equal(every[2], nvals)
    # some rows: those are the new ones (an empty new row keeps the old), the others the old ones
    idx = np.asarray([0, 5, 6, 36], dtype=np.int32)
    sub = tuple(x.copy() for x in _random_csr(rng, 4, 6))
    got = RR.splice(*old, idx, *sub)
    for i in range(37):
        a, b = int(got[0][i]), int(got[0][i + 1])
        j = list(idx).index(i) if i in idx else -1
        if j >= 0 and sub[0][j + 1] > sub[0][j]:
            want_c, want_v = sub[1][sub[0][j]:sub[0][j + 1]], sub[2][sub[0][j]:sub[0][j + 1]]
        else:
            want_c, want_v = old[1][old[0][i]:old[0][i + 1]], old[2][old[0][i]:old[0][i + 1]]
        assert np.array_equal(got[1][a:b], want_c) and np.array_equal(got[2][a:b], want_v)
    with pytest.raises(AssertionError):
        RR.splice(*old, np.asarray([5, 5], dtype=np.int32), *_random_csr(rng, 2, 3))


def test_from_counts_on_rows_known_by_hand():
    c = np.zeros((5, A), dtype=np.int32)
    c[0, 17] = 9                      # one entry
    c[1, [0, 3225]] = [1, 3]          # the two ends
    c[2, [4, 9, 11]] = [5, 7, 7]      # a tie at the maximum: the lowest wins
    c[4, [2, 8]] = [-3, 6]            # a negative count is not an entry
    ip, cols, vals, tg, n_empty = RR.from_counts(c)
    assert ip.tolist() == [0, 1, 3, 6, 6, 7] and cols.tolist() == [17, 0, 3225, 4, 9, 11, 8]
    assert vals.tolist() == [1.0, 0.25, 0.75, 5 / 19, 7 / 19, 7 / 19, 1.0]
    assert tg.tolist() == [17, 3225, 9, -1, 8] and n_empty == 1
    # the arithmetic of a temp-1 move as the Coach's tuples state it (coach.examples_from_records)
    row = np.zeros(A, dtype=np.int32)
    row[[3, 40, 41, 3000]] = [2, 1, 8, 1]
    counts = [float(x) ** 1.0 for x in row]
    s = float(sum(counts))
    _, cols, vals, tg, _ = RR.from_counts(row[None])
    assert [x / s for x in counts if x] == vals.tolist() and tg.tolist() == [41]


def test_selection_statistics():
    n, f = 4096, 0.25
    a = RR.select(n, 0, 21, 2, f)
    assert abs(len(a) - n * f) <= 6 * math.sqrt(n * f * (1 - f))  # 1024 +- 6 sqrt(768)
    assert np.all(np.diff(a) > 0) and a.dtype == np.int32
    b = RR.select(n, 0, 21, 3, f)
    assert abs(len(b) - n * f) <= 6 * math.sqrt(n * f * (1 - f))
    assert not np.array_equal(a, b)  # two keys differ
    both = len(np.intersect1d(a, b))  # ... and are independent: about n f^2 = 256 in common (sd < 14)
    assert abs(both - n * f * f) <= 6 * math.sqrt(n * f * f * (1 - f * f))
    assert len(RR.select(257, 5, 21, 2, 0.0)) == 0 and np.array_equal(RR.select(257, 5, 21, 2, 1.0), np.arange(257))
    # a selection is a function of the global index: a window shifted by its base picks the same examples
    assert np.array_equal(RR.select(1000, 96, 21, 2, f), a[(a >= 96) & (a < 1096)] - 96)
    # the counter's word 1 carries the index's high half, and the domain word keeps the draws off the game streams'
    base = 2**32 - 3
    u = [RR.uniform(21, 2, base + i) for i in range(6)]
    from oracle import spec
    x0, x1, _, _ = spec.philox4x32_10(1, 1, 2, 0x10000000, 21, 0)
    assert u[4] == float((x0 | (x1 << 32)) >> 11) * 2.0 ** -53
    assert len(set(u)) == 6 and u[4] != float(spec.draw64(21, 2, base + 4) >> 11) * 2.0 ** -53
