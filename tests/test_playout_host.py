"""Playout cap randomization, the parts that need no GPU: the reference schedule of
tests/playout_ref.py and the library's own (a host function), the knobs checked before anything touches the
device, the C entry points and their argument checks, and the numpy restatements of the full-row selection and
the CSR take on cases known by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import playout_ref as PR
from conftest import REPO
from helpers import philox_draw64_np

BASE = dict(numMCTSSims=12, cpuct=1.5, tempThreshold=15)
FIXED = ".FF.FF.F.F.F.F.F....F.FFF..F..F.FF..F...F...F..."  # (seed 2026, env_base 300, p 0.4), F = full


# ------------------------------------------------------------------ 1. the schedule
def test_reference_philox_is_the_game_streams_philox():
    """playout_ref's draw under domain 0 with counter (ctr, 0, env) is the game stream's draw64."""
    from oracle import spec
    for seed, env, ctr in ((2026, 300, 0), (2**63 + 5, 7, 41), (1, 2**32 - 1, 2**31)):
        x0, x1, _, _ = spec.philox4x32_10(ctr & PR.M32, 0, env, 0, seed & PR.M32, seed >> 32)
        assert (x0 | (x1 << 32)) == int(philox_draw64_np(seed, env, np.array([ctr], dtype=np.uint64))[0])


def test_schedule_extremes_and_fixed_case():
    assert not PR.schedule(2026, 300, 0.0, 48).any()
    assert PR.schedule(2026, 300, 1.0, 48).all()
    full = PR.schedule(2026, 300, 0.4, 48)
    assert PR.show(full) == FIXED
    assert int(full.sum()) == 20 and int(full[:14].sum()) == 8  # moves 0..13 are the temp-1 moves at threshold 15
    # env_base and seed both matter (ranks and iterations get their own schedules)
    assert PR.show(PR.schedule(2026, 301, 0.4, 48)) != FIXED
    assert PR.show(PR.schedule(2027, 300, 0.4, 48)) != FIXED


def test_schedule_domain_is_its_own():
    """The draws differ from the same counters under every other registered domain."""
    mine = [PR.uniform(2026, 300, m) for m in range(48)]
    for dom in (0, 0x10000000, 0x20000000, 0x40000000, 0x80000000):
        other = [PR.uniform(2026, 300, m, domain=dom) for m in range(48)]
        assert all(a != b for a, b in zip(mine, other)), hex(dom)
    src = open(os.path.join(REPO, "nypc-yacht-auction_amd", "csrc", "yk_philox.h")).read()
    assert re.search(r"constexpr uint32_t PHILOX_PLAYOUT = 0x30000000u;", src)
    assert re.search(r"//\s+PHILOX_PLAYOUT\s+\(move, env base, 0, \.\)", src)


def test_library_schedule_is_the_reference():
    """yk_playout_schedule runs on the host: the bits the engine uses, without a GPU."""
    from yacht_amd.engine import playout_schedule
    assert PR.show(playout_schedule(2026, 300, 0.4, 48)) == FIXED
    rng = np.random.default_rng(11)
    for _ in range(20):
        seed, base = int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**32))
        p = float(rng.random())
        assert np.array_equal(playout_schedule(seed, base, p, 64), PR.schedule(seed, base, p, 64)), (seed, base, p)
    assert playout_schedule(5, 6, 0.5, 0).shape == (0,)
    assert not playout_schedule(5, 6, 0.0, 48).any() and playout_schedule(5, 6, 1.0, 48).all()


# ------------------------------------------------------------------ 2. knobs
def test_check_playout_knobs_accepts():
    pytest.importorskip("torch")
    from yacht_amd.replay import check_playout_knobs as ck
    assert ck() == (0, 1.0) and ck(None, None, 100) == (0, 1.0) and ck(0, 1.0, 100) == (0, 1.0)
    assert ck(0, None, 1) == (0, 1.0)  # off: numMCTSSims = 1 stays a legal configuration
    assert ck(20, 0.25, 100) == (20, 0.25)
    assert ck(2, 1, 2) == (2, 1.0) and ck(100, 1e-9, 100) == (100, 1e-9)
    assert ck(np.int64(5), None, 10) == (5, 1.0)


BAD = [dict(playoutFastSims=1), dict(playoutFastSims=-4), dict(playoutFastSims=13), dict(playoutFastSims=2.5),
       dict(playoutFastSims=True), dict(playoutFastSims=4, playoutFullProb=-0.1),
       dict(playoutFastSims=4, playoutFullProb=1.5), dict(playoutFastSims=4, playoutFullProb=float("nan")),
       dict(playoutFastSims=4, playoutFullProb=0.0),  # no examples
       dict(playoutFullProb=0.5), dict(playoutFastSims=0, playoutFullProb=0.5),  # would silently do nothing
       dict(playoutFullProb=float("nan")), dict(playoutFastSims=4, numMCTSSims=None)]


@pytest.mark.parametrize("extra", BAD)
def test_bad_knobs_raise_before_any_device_call(extra):
    pytest.importorskip("torch")
    from yacht_amd.coach import Coach
    from yacht_amd.replay import check_playout_knobs
    from yacht_amd.utils import dotdict
    args = dotdict(BASE, **extra)
    with pytest.raises(ValueError, match="playoutFastSims|playoutFullProb"):
        check_playout_knobs(args.get("playoutFastSims"), args.get("playoutFullProb"), args.get("numMCTSSims"))
    with pytest.raises(ValueError, match="playoutFastSims|playoutFullProb"):
        Coach(None, None, args)  # (nothing of the game or the net is touched before the check)


def test_coach_defaults_are_off_and_knobs_are_kept():
    pytest.importorskip("torch")
    import inspect

    from yacht_amd import engine, replay
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.utils import dotdict
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE))
    assert (c.playout_fast_sims, c.playout_full_prob) == (0, 1.0)
    c = Coach(YachtGame(seed=1, env_id=0), object(), dotdict(BASE, playoutFastSims=4, playoutFullProb=0.4))
    assert (c.playout_fast_sims, c.playout_full_prob) == (4, 0.4)
    sig = inspect.signature(engine.SelfPlayEngine.__init__).parameters
    assert sig["playout_fast_sims"].default == 0 and sig["playout_full_prob"].default == 1.0
    assert inspect.signature(replay.examples_from_images).parameters["full_only"].default is False
    assert engine.SelfPlayEngine.COUNTER_NAMES[4] == "fast_moves"


def test_host_tuple_path_skips_fast_moves():
    """coach.examples_from_records on hand-made records: a move whose info[6] carries 0x100 is not an example."""
    pytest.importorskip("torch")
    from yacht_amd.coach import examples_from_records
    E, M = 2, 4
    info = np.zeros((E, M, 8), dtype=np.int32)
    info[:, :, 2] = np.arange(M) + 5  # temp 0: pi is one-hot at the action
    info[0, 1, 6] = PR.REC_FAST
    info[1, 0, 6] = PR.REC_FAST
    info[1, 3, 6] = PR.REC_FAST  # (past game 1's end: never looked at)
    rec = dict(states=np.zeros((E, M, 8), dtype=np.uint64), info=info, n_moves=np.array([4, 3], dtype=np.int32),
               visits_off=np.zeros(E * M + 1, dtype=np.int64), visits=np.zeros((0, 2), dtype=np.int32),
               values=np.arange(E * M, dtype=np.float64).reshape(E, M))
    ex = examples_from_records(rec, E)
    assert [[t[2] for t in g] for g in ex] == [[0.0, 2.0, 3.0], [5.0, 6.0]]
    assert [[t[1].index(1) for t in g] for g in ex] == [[5, 7, 8], [6, 7]]
    info[:, :, 6] = 0
    assert [len(g) for g in examples_from_records(rec, E)] == [4, 3]


# ------------------------------------------------------------------ 3. the C ABI
def _header():
    src = open(os.path.join(REPO, "include", "yacht_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_and_binding_declare_the_feature():
    import yacht_amd
    from yacht_amd import _lib
    src = _header()
    lib = yacht_amd.lib()
    for name in ("yk_engine_set_playout_cap", "yk_playout_schedule", "yk_examples_full_rows", "yk_policies_take"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
    assert re.search(r"#define YK_REC_FAST 0x100\b", src) and _lib.YK_REC_FAST == 0x100 == PR.REC_FAST
    P, L, I = C.c_void_p, C.c_int64, C.c_int
    assert _lib.SIGNATURES["yk_engine_set_playout_cap"] == [P, I, C.c_double]
    assert _lib.SIGNATURES["yk_playout_schedule"] == [C.c_uint64, C.c_uint32, C.c_double, I, P]
    assert _lib.SIGNATURES["yk_examples_full_rows"] == [P, I, I, I, I, L, P, L, P, P]
    assert _lib.SIGNATURES["yk_policies_take"] == [P, P, P, L, P, L, P, P, P, L, P, P]


def test_entry_points_reject_bad_arguments_without_a_device_call():
    import yacht_amd
    from yacht_amd._lib import YK_ERR_ARG, YK_OK
    lib = yacht_amd.lib()
    buf = (C.c_uint8 * 64)()
    sch = lib.yk_playout_schedule
    assert sch(1, 2, 0.5, 48, None) == YK_ERR_ARG and sch(1, 2, 0.5, -1, buf) == YK_ERR_ARG
    for p in (-0.01, 1.01, float("nan"), float("inf")):
        assert sch(1, 2, p, 48, buf) == YK_ERR_ARG
    assert sch(1, 2, 0.5, 0, buf) == YK_OK
    assert lib.yk_engine_set_playout_cap(None, 4, 0.5) == YK_ERR_ARG
    n = C.c_int64(-7)
    p = C.cast((C.c_int64 * 8)(), C.c_void_p)  # (a non-null pointer; never dereferenced: the calls fail before)
    q = C.cast((C.c_int64 * 8)(), C.c_void_p)
    r = C.cast((C.c_int64 * 8)(), C.c_void_p)
    fr = lib.yk_examples_full_rows
    assert fr(None, 1, 4, 48, 8, -1, None, 0, C.byref(n), None) == YK_ERR_ARG   # no images
    assert fr(p, 1, 4, 48, 8, -1, None, 0, None, None) == YK_ERR_ARG           # no n_full
    for dims in ((0, 4, 48, 8), (1, 0, 48, 8), (1, 4, 0, 8), (1, 4, 48, -1)):
        assert fr(p, *dims, -1, None, 0, C.byref(n), None) == YK_ERR_ARG
    assert fr(p, 1, 4, 48, 8, -1, p, -1, C.byref(n), None) == YK_ERR_ARG       # idx with a negative capacity
    assert n.value == -7
    tk = lib.yk_policies_take
    nnz = C.c_int64()
    ok = [p, p, p, 2, p, 1, q, None, None, 0, C.byref(nnz), None]

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return tk(*a) == YK_ERR_ARG
    assert bad(a0=None) and bad(a6=None) and bad(a10=None)   # indptr, out_indptr, nnz
    assert bad(a3=-1) and bad(a3=2**31) and bad(a5=-1) and bad(a5=2**31)  # n, m
    assert bad(a4=None)                                      # idx with m > 0
    assert bad(a6=p)                                         # out_indptr is the input's
    assert bad(a7=r)                                         # out_cols without out_vals
    assert bad(a7=r, a8=r, a1=None) and bad(a7=r, a8=r, a2=None)  # nothing to copy from
    assert bad(a7=r, a8=q, a9=-1)                            # a negative capacity
    assert bad(a7=p, a8=r) and bad(a7=r, a8=p)               # out_cols / out_vals is an input


# ------------------------------------------------------------------ 4. the restatements
def test_take_on_hand_made_rows():
    ip = np.array([0, 2, 2, 5], dtype=np.int64)  # rows: [10, 11], [], [20, 21, 22]
    cols = np.array([10, 11, 20, 21, 22], dtype=np.int32)
    vals = np.array([0.5, 0.5, 0.25, 0.25, 0.5])
    o = PR.take(ip, cols, vals, [2, 0, 1, 2])
    assert o[0].tolist() == [0, 3, 5, 5, 8] and o[1].tolist() == [20, 21, 22, 10, 11, 20, 21, 22]
    assert o[2].tolist() == [0.25, 0.25, 0.5, 0.5, 0.5, 0.25, 0.25, 0.5]
    assert o[0].dtype == np.int64 and o[1].dtype == np.int32 and o[2].dtype == np.float64
    e = PR.take(ip, cols, vals, [])
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0
    same = PR.take(ip, cols, vals, [0, 1, 2])
    assert all(np.array_equal(a, b) for a, b in zip(same, (ip, cols, vals)))
    with pytest.raises(AssertionError):
        PR.take(ip, cols, vals, [3])


def test_full_rows_on_hand_made_records():
    a = np.zeros((2, 3, 8), dtype=np.int32)
    b = np.zeros((2, 3, 8), dtype=np.int32)
    a[:, 1, 6] = PR.REC_FAST       # image 0: move 1 fast
    b[:, 0, 6] = PR.REC_FAST | 3   # image 1: move 0 fast (a status beside the bit)
    b[:, 2, 6] = 5                 # a status alone is not the bit
    nm = [np.array([3, 2]), np.array([3, 3])]
    idx, total = PR.full_rows([a, b], nm)
    # examples: img0 g0 m0..2 = 0,1,2 ; g1 m0..1 = 3,4 ; img1 g0 = 5,6,7 ; g1 = 8,9,10
    assert total == 11 and idx.tolist() == [0, 2, 3, 6, 7, 9, 10] and idx.dtype == np.int32
    idx, total = PR.full_rows([a, b], nm, n_games=3)
    assert total == 8 and idx.tolist() == [0, 2, 3, 6, 7]
    idx, total = PR.full_rows([a, b], nm, n_games=0)
    assert total == 0 and idx.size == 0
    a[:, :, 6] = 0
    b[:, :, 6] = 0
    idx, total = PR.full_rows([a, b], nm)
    assert idx.tolist() == list(range(11))
