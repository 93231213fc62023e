"""Averaged (EMA) weights, the parts that need no GPU: the host weight schedule against
tests/ema_ref.py bit for bit, the argument checks that return before anything touches a device, the knob check,
the declarations, and the float32 update formula against the same recurrence in float64."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ema_ref as ER
from conftest import REPO

ENTRY_POINTS = ("yk_ema_weight", "yk_ema_update", "yk_trainer_set_ema", "yk_trainer_ema_buffer",
                "yk_trainer_ema_get", "yk_trainer_ema_set", "yk_trainer_ema_state")
YK_OK, YK_ERR_ARG = 0, -1


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _lib_weight(lib, decay, t):
    w = C.c_float(-1.0)
    rc = lib.yk_ema_weight(float(decay), int(t), C.byref(w))
    return rc, np.float32(w.value)


# ------------------------------------------------------------------ 1. the schedule
def test_reference_weight_by_hand():
    assert ER.weight(0.999, 0) == np.float32(0.9)       # 1 - 1/10
    assert ER.weight(0.999, 1) == np.float32(1.0 - 2.0 / 11.0)
    assert ER.weight(0.0, 12345) == np.float32(1.0)      # decay 0: the shadow is the parameters
    assert ER.weight(0.5, 8) == np.float32(0.5) and ER.weight(0.5, 7) == np.float32(1.0 - 8.0 / 17.0)
    # 0.999 takes over from the warm-up term at t = 8990 / 8991: (1 + t) / (10 + t) is 8991 / 9000 = 0.999 at
    # 8990 (the two terms meet, up to the quotient's rounding), below it before and above it from 8991 on
    assert (1.0 + 8989) / (10.0 + 8989) < 0.999 < (1.0 + 8991) / (10.0 + 8991)
    assert abs((1.0 + 8990) / (10.0 + 8990) - 0.999) < 1e-15
    assert ER.weight(0.999, 8989) == np.float32(1.0 - 8990.0 / 8999.0) > ER.weight(0.999, 8991)
    assert ER.weight(0.999, 8990) == np.float32(1.0 - min(0.999, 8991.0 / 9000.0))
    assert ER.weight(0.999, 8991) == np.float32(1.0 - 0.999) == ER.weight(0.999, 10**6)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.999])
def test_library_weight_is_the_reference_bit_for_bit(decay):
    from yacht_amd._lib import lib
    for t in (0, 1, 8, 9, 10, 8990, 8991, 10**6):
        rc, w = _lib_weight(lib(), decay, t)
        assert rc == YK_OK
        assert _bits(w) == _bits(ER.weight(decay, t)), (decay, t, w)
        assert 0.0 <= w <= 1.0


# ------------------------------------------------------------------ 2. argument checks (no device)
def test_weight_argument_errors():
    from yacht_amd._lib import lib
    L = lib()
    for decay, t in ((-0.1, 0), (1.0, 0), (1.5, 3), (math.nan, 0), (math.inf, 0), (0.5, -1)):
        rc, w = _lib_weight(L, decay, t)
        assert rc == YK_ERR_ARG and w == np.float32(-1.0), (decay, t)
    assert L.yk_ema_weight(0.5, 0, None) == YK_ERR_ARG


def test_update_argument_errors_without_a_device():
    """Refused before any launch: the pointers here are host arrays no kernel may see."""
    from yacht_amd._lib import lib
    L = lib()
    e = np.ones(8, dtype=np.float32)
    p = np.zeros(8, dtype=np.float32)
    ep, pp = e.ctypes.data, p.ctypes.data
    assert L.yk_ema_update(None, pp, 8, 0.5, None) == YK_ERR_ARG
    assert L.yk_ema_update(ep, None, 8, 0.5, None) == YK_ERR_ARG
    assert L.yk_ema_update(ep, pp, -1, 0.5, None) == YK_ERR_ARG
    for w in (-0.1, 1.5, math.nan):
        assert L.yk_ema_update(ep, pp, 8, w, None) == YK_ERR_ARG, w
    assert L.yk_ema_update(ep, pp, 0, 0.5, None) == YK_OK  # n == 0: nothing to do, no launch
    assert (e == 1).all() and (p == 0).all()


def test_trainer_entry_points_refuse_null():
    from yacht_amd._lib import lib
    L = lib()
    out = (C.c_double * 4)()
    ptr = C.c_void_p()
    assert L.yk_trainer_set_ema(None, 0.9, 1) == YK_ERR_ARG
    assert L.yk_trainer_ema_buffer(None, C.byref(ptr)) == YK_ERR_ARG
    assert L.yk_trainer_ema_get(None, None) == YK_ERR_ARG
    assert L.yk_trainer_ema_set(None, None, 0) == YK_ERR_ARG
    assert L.yk_trainer_ema_state(None, out) == YK_ERR_ARG


# ------------------------------------------------------------------ 3. knobs
def test_check_ema_knobs():
    from yacht_amd.replay import check_ema_knobs as ck
    assert ck() == (0.0, 1) and ck(None, None) == (0.0, 1) and ck(0, 1) == (0.0, 1)
    assert ck(0.9) == (0.9, 1) and ck(0.999, 4) == (0.999, 4) and ck(0.5, np.int64(2)) == (0.5, 2)
    d, e = ck(0.9, 3)
    assert isinstance(d, float) and isinstance(e, int)
    for bad in ((-0.1, 1), (1.0, 1), (1.5, 1), (math.nan, 1), (0.9, 0), (0.9, -2), (0.9, 1.5), (0.9, True),
                (0.9, "2"), (0.0, 2), (None, 4)):
        with pytest.raises(ValueError):
            ck(*bad)


def test_coach_and_wrapper_check_the_knobs_before_any_device_work():
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import HashPriorNet, NNetWrapper
    from yacht_amd.utils import dotdict
    game = YachtGame(seed=1, env_id=0)
    base = dict(numMCTSSims=4, cpuct=1.5, tempThreshold=15)
    for bad in (dict(emaDecay=1.0), dict(emaDecay=-0.5), dict(emaEvery=3), dict(emaDecay=0.9, emaEvery=0)):
        with pytest.raises(ValueError):
            Coach(game, HashPriorNet(game), dotdict(base, **bad))
    c = Coach(game, HashPriorNet(game), dotdict(base, emaDecay=0.99, emaEvery=2))
    assert (c.ema_decay, c.ema_every) == (0.99, 2)
    assert (Coach(game, HashPriorNet(game), dotdict(base)).ema_decay) == 0.0
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=16, hidden=64, nblocks=1, dropout=0.0)
    w = NNetWrapper(game, dotdict(args, emaDecay=0.9, emaEvery=0))
    with pytest.raises(ValueError):
        w.train([])  # the knob check comes first: no trainer is built
    assert not NNetWrapper(game, args).ema_on() and NNetWrapper(game, dotdict(args, emaDecay=0.5)).ema_on()


# ------------------------------------------------------------------ 4. declarations
def test_header_and_binding_declare_the_entry_points():
    from yacht_amd import _lib
    hdr = open(os.path.join(REPO, "include", "yacht_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and name in _lib._NEWER, name
        assert hasattr(_lib.lib(), name), name
    mk = open(os.path.join(REPO, "nypc-yacht-auction_amd", "Makefile")).read()
    assert re.search(r"\byk_ema\b", mk)
    # yk_trainer_get / _set keep their 0..3 range
    assert "which < 0 || which > 3" in open(os.path.join(REPO, "nypc-yacht-auction_amd", "csrc", "yk_train.hip")).read()


# ------------------------------------------------------------------ 5. the formula against float64
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
def test_float32_formula_stays_within_the_derived_bound_of_float64(decay):
    """400 updates of a 4099-element random walk.  Each update makes three roundings of at most 2**-24 relative:
    two act on w (p - e), of magnitude at most 2 M, one on the result, at most M - 5 * 2**-24 * M per update -
    and the carried error contracts by d_t <= decay, so the total stays below 5 * 2**-24 * M / (1 - decay).
    Used of the bound when this was written: 0.11 (decay 0.5), 0.06 (0.9), 0.001 (0.999)."""
    rng = np.random.default_rng(20261020)
    n, steps = 4099, 400
    p = rng.standard_normal(n).astype(np.float32)
    e32, e64 = p.copy(), p.astype(np.float64)
    M, worst = float(np.abs(p).max()), 0.0
    for t in range(steps):
        p = (p + rng.normal(0.0, 1e-2, n).astype(np.float32)).astype(np.float32)
        M = max(M, float(np.abs(p).max()))
        w = ER.weight(decay, t)
        e32 = ER.update(e32, p, w)
        e64 = ER.update64(e64, p, w)
        assert e32.dtype == np.float32
        worst = max(worst, float(np.abs(e32.astype(np.float64) - e64).max()))
    bound = 5.0 * 2.0 ** -24 * M / (1.0 - decay)
    print(f"decay {decay}: worst {worst:.3e}, bound {bound:.3e}, used {worst / bound:.4f}")
    assert worst <= bound
