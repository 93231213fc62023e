"""The self-play temperatures on the host: the knobs' validation, the schedule the host
builds against its formula bit for bit, the plain-Python restatement (tests/temper_ref.py) against noise_ref's
when both schedules are off, and the draw margins of the games the GPU tests replay.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_ref as R
import temper_ref as T

import yacht_amd
from yacht_amd import replay
from yacht_amd._lib import YK_ERR_ARG

FIELDS = ("states", "info", "ctr", "values", "final", "n_moves", "visits_off", "visits")


# ------------------------------------------------------------------ 1. the knobs
def test_unset_is_off_and_early_defaults_to_final():
    off = replay.check_temperature_knobs()
    assert off == dict(move_temperature=None, move_temperature_early=None, root_policy_temperature=None,
                       root_policy_temperature_early=None, temperature_halflife=None)
    k = replay.check_temperature_knobs(moveTemperature=0.15, rootPolicyTemperature=1.1)
    assert (k["move_temperature"], k["move_temperature_early"]) == (0.15, 0.15)
    assert (k["root_policy_temperature"], k["root_policy_temperature_early"]) == (1.1, 1.1)
    assert k["temperature_halflife"] is None
    k = replay.check_temperature_knobs(0.15, 0.75, 1.1, 1.25, 19)
    assert k == dict(move_temperature=0.15, move_temperature_early=0.75, root_policy_temperature=1.1,
                     root_policy_temperature_early=1.25, temperature_halflife=19.0)
    # the ends of both ranges are legal
    replay.check_temperature_knobs(0.05, 100.0, 0.25, 10.0, 1e-3)
    # an Early equal to its final value needs no halflife
    replay.check_temperature_knobs(moveTemperature=0.5, moveTemperatureEarly=0.5)


@pytest.mark.parametrize("kw", [
    dict(moveTemperature=0.04), dict(moveTemperature=100.5), dict(moveTemperature=float("nan")),
    dict(moveTemperature=0.0), dict(moveTemperature=-1.0), dict(moveTemperature=True), dict(moveTemperature="1"),
    dict(moveTemperature=0.5, moveTemperatureEarly=0.01, temperatureHalflife=8),
    dict(moveTemperature=0.5, moveTemperatureEarly=float("inf"), temperatureHalflife=8),
    dict(rootPolicyTemperature=0.2), dict(rootPolicyTemperature=10.5), dict(rootPolicyTemperature=float("nan")),
    dict(rootPolicyTemperature=False), dict(rootPolicyTemperature=[1.1]),
    dict(rootPolicyTemperature=1.1, rootPolicyTemperatureEarly=11.0, temperatureHalflife=8),
    # an Early or a halflife without its final value would silently do nothing
    dict(moveTemperatureEarly=0.75), dict(rootPolicyTemperatureEarly=1.25), dict(temperatureHalflife=8),
    dict(moveTemperatureEarly=0.75, rootPolicyTemperature=1.1),
    dict(rootPolicyTemperatureEarly=1.25, moveTemperature=0.15),
    # an Early that differs from its final value needs a halflife > 0
    dict(moveTemperature=0.15, moveTemperatureEarly=0.75),
    dict(rootPolicyTemperature=1.1, rootPolicyTemperatureEarly=1.25),
    dict(moveTemperature=0.15, moveTemperatureEarly=0.75, temperatureHalflife=0),
    dict(moveTemperature=0.15, moveTemperatureEarly=0.75, temperatureHalflife=-2.0),
    dict(moveTemperature=0.15, moveTemperatureEarly=0.75, temperatureHalflife=float("nan")),
    dict(moveTemperature=0.15, moveTemperatureEarly=0.75, temperatureHalflife=float("inf")),
    dict(moveTemperature=0.15, temperatureHalflife=True), dict(moveTemperature=0.15, temperatureHalflife="8"),
])
def test_bad_knobs_are_value_errors(kw):
    with pytest.raises(ValueError):
        replay.check_temperature_knobs(**kw)


def test_knobs_are_read_from_args():
    from yacht_amd.utils import dotdict
    args = dotdict(moveTemperature=0.15, moveTemperatureEarly=0.75, rootPolicyTemperature=1.1,
                   rootPolicyTemperatureEarly=1.25, temperatureHalflife=19)
    assert replay.temperature_knobs_of(args) == replay.check_temperature_knobs(0.15, 0.75, 1.1, 1.25, 19)
    assert replay.temperature_knobs_of(dotdict()) == replay.check_temperature_knobs()
    with pytest.raises(ValueError):
        replay.temperature_knobs_of(dotdict(moveTemperatureEarly=0.75))


# ------------------------------------------------------------------ 2. the schedule, bit for bit
@pytest.mark.parametrize("early,final,halflife", [(0.75, 0.15, 19.0), (1.25, 1.1, 19.0), (1.3, 0.3, 8.0),
                                                   (0.05, 100.0, 0.37), (10.0, 0.25, 4096.0), (1.0, 1.0, 0.0),
                                                   (0.8, 0.8, 3.0), (100.0, 0.05, 1e-3)])
def test_schedule_is_the_formula_bit_for_bit(early, final, halflife):
    from yacht_amd import kernels as K
    n = 64
    got = K.temperature_schedule(early, final, halflife, n)
    assert got.dtype == np.float64 and got.shape == (n,)
    if early == final:
        want = np.full(n, final)
    else:
        want = np.array([final + (early - final) * 2.0 ** (-m / halflife) for m in range(n)], dtype=np.float64)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(T.schedule(early, final, halflife, n).view(np.uint64), want.view(np.uint64))
    assert got[0] == final + (early - final) and (early == final or abs(got[-1] - final) < abs(got[0] - final))
    if halflife >= 1 and halflife == int(halflife) and int(halflife) < n:  # one halflife in: half way, exactly
        assert got[int(halflife)] == final + (early - final) * 0.5


def test_schedule_rejects_bad_arguments():
    lib = yacht_amd.lib()
    out = np.zeros(8, dtype=np.float64)
    ok = lib.yk_temperature_schedule(0.75, 0.15, 19.0, 8, out.ctypes.data)
    assert ok == 0 and out[0] == 0.75
    for early, final, hl, n, ptr in ((0.75, 0.15, 19.0, 8, None), (0.75, 0.15, 19.0, -1, out.ctypes.data),
                                     (0.0, 0.15, 19.0, 8, out.ctypes.data), (0.75, -1.0, 19.0, 8, out.ctypes.data),
                                     (math.nan, 0.15, 19.0, 8, out.ctypes.data),
                                     (0.75, math.inf, 19.0, 8, out.ctypes.data),
                                     (0.75, 0.15, 0.0, 8, out.ctypes.data), (0.75, 0.15, -1.0, 8, out.ctypes.data),
                                     (0.75, 0.15, math.nan, 8, out.ctypes.data),
                                     (0.75, 0.15, math.inf, 8, out.ctypes.data)):
        assert lib.yk_temperature_schedule(early, final, hl, n, C.c_void_p(ptr)) == YK_ERR_ARG


# ------------------------------------------------------------------ 3. the restatement
def test_pick_is_the_reference_draw_at_one_and_sharpens_below():
    counts = [3, 1, 7, 2, 7]
    for u in (0.0, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -53):
        i, total, _ = T.pick(counts, 1.0, u)
        cdf = np.cumsum(np.array(counts, dtype=np.float64) / 20.0)
        assert total == 20.0 and i == int(np.searchsorted(cdf / cdf[-1], u, side="right"))
    # T -> 0.05: the two largest counts share everything (7 ** 20 against 3 ** 20 is 2e7 to 1)
    assert T.pick(counts, 0.05, 0.49)[0] == 2 and T.pick(counts, 0.05, 0.51)[0] == 4
    # T = 100: close to uniform
    assert [T.pick(counts, 100.0, u)[0] for u in (0.1, 0.3, 0.5, 0.7, 0.9)] == [0, 1, 2, 3, 4]
    assert T.pick([], 0.5, 0.3)[0] == -1
    assert T.pick([1, 65535], 0.05, 0.5)[1] == 1.0 + 65535.0 ** 20 and math.isfinite(3024 * 65535.0 ** 20)


def test_root_temper_restated():
    P = np.array([0.5, 0.25, 0.0, 0.125, 0.125], dtype=np.float32)
    assert np.array_equal(T.root_temper(P, 1.0), P)
    flat, sharp = T.root_temper(P, 1.25), T.root_temper(P, 0.8)
    assert flat.dtype == np.float32 and flat[2] == 0 and sharp[2] == 0
    assert flat[0] < P[0] < sharp[0] and flat[3] > P[3] > sharp[3]
    assert abs(float(flat.sum()) - 1) < 1e-6 and abs(float(sharp.sum()) - 1) < 1e-6
    assert np.array_equal(T.root_temper(np.array([0.3], dtype=np.float32), 2.0), np.array([1.0], dtype=np.float32))
    assert np.array_equal(T.root_temper(np.zeros(3, dtype=np.float32), 2.0), np.zeros(3, dtype=np.float32))


def test_both_schedules_off_is_noise_ref():
    for thr in (15, 49):
        want = R.play_episode(T.SEED, T.ENV_BASE, T.SIMS, temp_threshold=thr)
        got = T.play_episode(T.SEED, T.ENV_BASE, T.SIMS, temp_threshold=thr)
        for k in FIELDS:
            assert np.array_equal(got[k], want[k]), k
        # and tables of exactly 1.0 are off as well
        ones = np.ones(48)
        got = T.play_episode(T.SEED, T.ENV_BASE, T.SIMS, move_t=ones, root_t=ones, temp_threshold=thr)
        for k in FIELDS:
            assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------ 4. the GPU tests' games keep off the boundaries
def test_replayed_games_have_a_draw_margin():
    """Every (seed, env) that tests/test_gpu_temper.py replays through play_episode and demands exact actions of:
    the smallest |c_i / last - u| over the game's draws is >= 1e-9 (device pow and libm pow differ by ulps, a
    relative 1e-15 or so of a c_i).  The run that consumes the device's own noised priors cannot be played here;
    the GPU test asserts its margin before it compares."""
    mt = T.schedule(n_moves=48, **T.MOVE_SCHEDULE)
    rt = T.schedule(n_moves=48, **T.ROOT_SCHEDULE)
    worst = float("inf")
    for e in range(T.N_GAMES):
        for thr in T.THRESHOLDS:
            g = T.play_episode(T.SEED, T.ENV_BASE + e, T.SIMS, move_t=mt, temp_threshold=thr)
            assert g["n_moves"] == 48 and g["info"][:thr - 1, 0].all() and not g["info"][thr - 1:, 0].any()
            worst = min(worst, g["margin"])
        for kw in (dict(root_t=rt), dict(root_t=rt, move_t=mt, k=2.0)):
            worst = min(worst, T.play_episode(T.SEED, T.ENV_BASE + e, T.SIMS, temp_threshold=49, **kw)["margin"])
    print(f"smallest draw margin {worst:.3g}")
    assert worst >= T.MARGIN
