"""The four handle constructors of the C ABI, end to end on whatever machine runs the suite: with a device
each returns YK_OK and a handle that is destroyed again; without one the first device allocation fails, the
call returns YK_ERR_NOMEM, frees what it made and leaves the caller's handle null."""
import ctypes as C

import numpy as np
import pytest
import torch

H, NB, FEAT, ASIZE = 64, 0, 59, 3226
SIZES = [H * FEAT, H, H, H, H, H, ASIZE * H, ASIZE, H, H, 128 * H, 128, 128, 1]  # state_dict order, no blocks


@pytest.fixture(scope="module")
def params():
    rng = np.random.default_rng(3)
    arrs = [np.ascontiguousarray(rng.standard_normal(n).astype(np.float32) * 0.05) for n in SIZES]
    return arrs, (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _check(lib, rc, h, destroy):
    if torch.cuda.is_available():
        assert rc == 0 and h.value is not None
        assert getattr(lib, destroy)(h) == 0
    else:
        assert rc == -3  # YK_ERR_NOMEM
        assert h.value is None


@pytest.mark.parametrize("amp", [0, 1])
def test_trainer_create(params, amp):
    import yacht_amd
    from yacht_amd.train import YkTrainConfig
    lib = yacht_amd.lib()
    cfg = YkTrainConfig(1, 2e-3, 1e-4, 0.9, 0.999, 1e-8, 5.0, 1.5, 0.3, 0, amp, 65536.0, 2000)
    h = C.c_void_p()
    rc = lib.yk_trainer_create(C.byref(h), H, NB, params[1], len(SIZES), C.byref(cfg))
    _check(lib, rc, h, "yk_trainer_destroy")


def test_net_create(params):
    import yacht_amd
    lib = yacht_amd.lib()
    h = C.c_void_p()
    rc = lib.yk_net_create(C.byref(h), H, NB, params[1], len(SIZES))
    _check(lib, rc, h, "yk_net_destroy")


def test_engine_create():
    import yacht_amd
    from yacht_amd._lib import YkEngineConfigFull
    lib = yacht_amd.lib()
    cfg = YkEngineConfigFull(n_envs=1, sims=2, cpuct=1.5, temp_threshold=15, max_moves=48, prior=1,
                             record_predictions=0, max_expansions=0, arena_entries=64, record_stride=1, groups=0,
                             dual_trees=0, dirichlet_alpha=0.0, dirichlet_eps=0.0, record_root_values=0)
    h = C.c_void_p()
    rc = lib.yk_engine_create(C.byref(h), C.byref(cfg), None)
    _check(lib, rc, h, "yk_engine_destroy")
