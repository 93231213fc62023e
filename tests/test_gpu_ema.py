"""Averaged (EMA) weights on the MI355X: the streaming kernel alone, bit for bit against
tests/ema_ref.py at every size / alignment path; the kernel inside both trainers (the shadow follows the
reference recurrence fed with each step's parameters, and everything else stays what a trainer without it
computes); the skipped AMP step; the on / off / state errors; NNetWrapper (what plays is the shadow, the
checkpoint carries both sets); the evaluate CLI; and one Coach iteration with a forced rejection."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ema_ref as ER
from conftest import PKG
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

YK_ERR_STATE, YK_ERR_ARG = -5, -1
# one pass of the kernel's full grid on the vector path: 2048 workgroups x 256 threads x 4 floats (yk_ema.hip)
ONE_PASS = 2048 * 256 * 4
SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099, ONE_PASS + 3)
GUARD = 8  # floats on either side of each buffer (a multiple of 4: offset 0 stays 16-byte aligned)
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import kernels as K
    from yacht_amd import train
    from yacht_amd._lib import call, lib, ptr, stream_ptr
    return K, train, call, lib, ptr, stream_ptr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """Equal bit for bit; where the reference is NaN (0 x inf: its sign and payload are the host FPU's, not the
    rule's) the result must be a NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _sd(hidden, nblocks):
    return {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in spec.closed_form_weights(hidden, nblocks).items()}


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.fixture(scope="module")
def kernel_data():
    """(e, p) of the largest size, made once: N(0, 1) with elements where p == e exactly, zeros in either, both,
    and one inf in p.  Every smaller size takes a prefix (the special elements sit at the front)."""
    rng = np.random.default_rng(7)
    n = max(SIZES)
    e = rng.standard_normal(n).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    p[::7] = e[::7]          # p == e: the result must be e
    p[2::11] = 0.0           # zeros in p,
    e[3::13] = 0.0           # in e,
    e[5::143] = 0.0          # and in both
    p[5::143] = 0.0
    p[0] = e[0]              # (n = 1: the p == e case)
    p[1] = np.inf            # n >= 3: one inf
    return e, p


@pytest.mark.parametrize("off_e,off_p", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_kernel_matches_reference_bit_for_bit(Y, kernel_data, off_e, off_p):
    """off_e / off_p: floats into the allocation - 0 is 16-byte aligned (the float4 path needs both), 1 takes
    the scalar path.  The floats around each range are untouched."""
    K, TR, call, lib, ptr, stream_ptr = Y
    E, P = kernel_data
    weights = (np.float32(0.0), np.float32(0.5), ER.weight(0.999, 10**6), np.float32(1.0))
    for n in SIZES:
        e0, p0 = E[:n], P[:n]
        ebuf = np.full(n + 2 * GUARD + 1, SENTINEL, dtype=np.float32)
        pbuf = np.full(n + 2 * GUARD + 1, SENTINEL, dtype=np.float32)
        pbuf[GUARD + off_p:GUARD + off_p + n] = p0
        dp = torch.from_numpy(pbuf).cuda()
        assert dp.data_ptr() % 16 == 0
        for w in weights:
            ebuf[GUARD + off_e:GUARD + off_e + n] = e0
            de = torch.from_numpy(ebuf).cuda()
            assert de.data_ptr() % 16 == 0
            ev, pv = de[GUARD + off_e:GUARD + off_e + n], dp[GUARD + off_p:GUARD + off_p + n]
            assert (ev.data_ptr() % 16 == 0) == (off_e == 0) and (pv.data_ptr() % 16 == 0) == (off_p == 0)
            call("yk_ema_update", ptr(ev), ptr(pv), n, float(w), stream_ptr())
            got_e, got_p = de.cpu().numpy(), dp.cpu().numpy()
            want = ER.update(e0, p0, w)
            tag = (n, off_e, off_p, float(w))
            assert _same_bits(got_e[GUARD + off_e:GUARD + off_e + n], want), tag
            assert (got_e[:GUARD + off_e] == SENTINEL).all() and (got_e[GUARD + off_e + n:] == SENTINEL).all(), tag
            assert np.array_equal(_bits(got_p), _bits(pbuf)), tag  # params and their guards: read only
            fin = np.isfinite(p0)
            same = p0 == e0
            assert np.array_equal(_bits(want[same]), _bits(e0[same]))  # (the reference itself: p == e gives e)
            if w == 0.0:  # e as it was (beside the inf: 0 x inf is NaN under the rule)
                assert np.array_equal(_bits(got_e[GUARD + off_e:GUARD + off_e + n][fin]), _bits(e0[fin])), tag
            if w == 1.0:
                # p - as far as the rule's own roundings allow: e + fl(p - e) is p exactly where p - e is exact
                # (p == e, a zero on either side, the inf), and otherwise within the two roundings' reach,
                # 2**-24 |p - e| from the difference and 2**-24 |p| from the sum
                got = got_e[GUARD + off_e:GUARD + off_e + n]
                exact = same | (p0 == 0) | (e0 == 0) | ~fin
                assert np.array_equal(got[exact], p0[exact]), tag
                p64, e64 = p0[fin].astype(np.float64), e0[fin].astype(np.float64)
                reach = 2.0 ** -24 * (np.abs(p64 - e64) + np.abs(p64)) * (1 + 2.0 ** -23)
                assert (np.abs(got[fin].astype(np.float64) - p64) <= reach).all(), tag


def test_kernel_n_zero_and_bad_arguments_on_device_buffers(Y):
    K, TR, call, lib, ptr, stream_ptr = Y
    e = torch.ones(8, device="cuda")
    p = torch.zeros(8, device="cuda")
    L = lib()
    assert L.yk_ema_update(ptr(e), ptr(p), 0, 0.5, stream_ptr()) == 0
    for w in (-0.1, 1.5, float("nan")):
        assert L.yk_ema_update(ptr(e), ptr(p), 8, w, stream_ptr()) == YK_ERR_ARG
    assert L.yk_ema_update(ptr(e), ptr(p), -1, 0.5, stream_ptr()) == YK_ERR_ARG
    assert (e == 1).all().item() and (p == 0).all().item()


# ------------------------------------------------------------------ 2. inside both trainers
@pytest.fixture(scope="module")
def batches(Y, golden):
    """train_h64_b1.npz's states as device examples and the six steps' row sets: 16, 16, a ragged 5, 16, 16, 16;
    step 3 (0-based) goes through backward + apply."""
    K = Y[0]
    g = golden("train_h64_b1.npz")
    n = len(g["values"])
    rng = np.random.RandomState(3)
    S = K.states_to_device(g["states"])
    tg = torch.tensor(rng.randint(0, 3226, n), dtype=torch.int32, device="cuda")
    vv = torch.tensor(np.asarray(g["values"], dtype=np.float32), device="cuda")
    rows = [np.arange(0, 16), np.arange(16, 32), np.arange(32, 37), np.arange(37, 53), np.arange(48, 64),
            np.arange(5, 21)]
    idx = [torch.tensor(r, dtype=torch.int32, device="cuda") for r in rows]
    return S, tg, vv, idx


def _trainer(TR, amp, **kw):
    return TR.Trainer(_sd(64, 1), 64, 1, lr=2e-3, weight_decay=1e-4, max_batch=16, vloss_weight=1.5, dropout=0.0,
                      seed=9, amp=amp, **kw)


def _do_step(tr, batches, k):
    S, tg, vv, idx = batches
    if k == 3:
        tr.backward(S, tg, vv, idx=idx[k])
        tr.apply()
    else:
        tr.step(S, tg, vv, idx=idx[k])


def _everything(tr):
    m, v = tr.moments()
    out = dict(params=tr.params().cpu().numpy().copy(), grads=tr.grads().cpu().numpy().copy(),
               losses=tr.losses().copy(), steps=tr.step_count)
    for k in m:
        out["m/" + k], out["v/" + k] = m[k].numpy().copy(), v[k].numpy().copy()
    if tr.amp:
        out["amp"] = tr.amp_state()
    return out


def _assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag} {k}")  # (NaN == NaN: a skipped step's grads)
            assert a[k].dtype != np.float32 or np.array_equal(_bits(a[k])[~np.isnan(a[k])], _bits(b[k])[~np.isnan(b[k])])
        else:
            assert a[k] == b[k], (tag, k, a[k], b[k])


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("amp", [False, True])
def test_trainer_shadow_follows_the_reference_recurrence(Y, batches, amp, every):
    K, TR, call, lib, ptr, stream_ptr = Y
    on = _trainer(TR, amp, ema_decay=0.9, ema_every=every)
    off = _trainer(TR, amp)
    assert on.ema_state() == {"decay": 0.9, "every": every, "updates": 0, "since": 0}
    e = on.params().cpu().numpy().copy()
    assert np.array_equal(_bits(on.ema().cpu().numpy()), _bits(e))  # the shadow starts as the parameters
    assert on.ema().data_ptr() != on.params().data_ptr() and on.ema().numel() == on.nparams
    updates = since = 0
    for k in range(6):
        _do_step(on, batches, k)
        _do_step(off, batches, k)
        p = on.params().cpu().numpy()
        since += 1
        if since == every:
            e = ER.update(e, p, ER.weight(0.9, updates))
            updates, since = updates + 1, 0
        assert np.array_equal(_bits(on.ema().cpu().numpy()), _bits(e)), (k, amp, every)
        assert on.ema_state() == {"decay": 0.9, "every": every, "updates": updates, "since": since}
        _assert_same(_everything(on), _everything(off), f"step {k}")
    assert updates == 6 // every and not np.array_equal(e, p)
    # the host copy in state_dict order is the flat view, tensor by tensor
    flat = np.concatenate([t.numpy().ravel() for t in on.ema_state_dict().values()])
    assert np.array_equal(_bits(flat), _bits(e))
    assert list(on.ema_state_dict().keys()) == list(on.state_dict().keys())


def test_skipped_amp_step_counts(Y, golden):
    """The recipe of test_amp_skipped_step_gradients_as_torch_leaves_them: at init_scale 2 ** 40 the scaled fp16
    gradients overflow and GradScaler skips the step.  The apply is counted, the shadow moves once more toward
    the unchanged parameters, the optimiser's step count stays."""
    K, TR, call, lib, ptr, stream_ptr = Y
    H, NB, B = 64, 1, 32
    W = golden("states.npz")["states"][:B]
    rng = np.random.RandomState(6)
    S = K.states_to_device(W)
    tg = torch.tensor(rng.randint(0, 3226, B), dtype=torch.int32, device="cuda")
    vv = torch.tensor(rng.rand(B) * 2 - 1, dtype=torch.float32, device="cuda")
    tr = TR.Trainer(_sd(H, NB), H, NB, max_batch=B, dropout=0.0, amp=True, init_scale=2.0 ** 40, ema_decay=0.9)
    p0 = tr.params().cpu().numpy().copy()
    # a shadow away from the parameters, so that a move toward them shows
    e0 = (p0 + np.float32(0.25)).astype(np.float32)
    names = list(tr.state_dict().keys())
    sizes = [int(np.prod(s)) for s in tr.shapes]
    cuts = np.cumsum([0] + sizes)
    tr.load_ema({k: torch.from_numpy(e0[cuts[i]:cuts[i + 1]].reshape(tr.shapes[i]).copy())
                 for i, k in enumerate(names)}, 4)
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(e0))
    assert tr.ema_state()["updates"] == 4
    tr.step(S, tg, vv)
    st = tr.amp_state()
    assert st["found_inf"] and st["steps"] == 0 and tr.step_count == 0
    assert np.array_equal(tr.params().cpu().numpy(), p0)
    assert tr.ema_state() == {"decay": 0.9, "every": 1, "updates": 5, "since": 0}
    want = ER.update(e0, p0, ER.weight(0.9, 4))
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(want)) and not np.array_equal(want, e0)


def test_on_off_and_state_errors(Y, batches):
    K, TR, call, lib, ptr, stream_ptr = Y
    L = lib()
    tr = _trainer(TR, False)
    zeros = {"decay": 0.0, "every": 0, "updates": 0, "since": 0}
    assert tr.ema_state() == zeros
    p = C.c_void_p()
    outs = [np.zeros(s, dtype=np.float32) for s in tr.shapes]
    arr = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    assert L.yk_trainer_ema_buffer(tr.handle, C.byref(p)) == YK_ERR_STATE
    assert L.yk_trainer_ema_get(tr.handle, arr) == YK_ERR_STATE
    assert L.yk_trainer_ema_set(tr.handle, arr, 0) == YK_ERR_STATE
    assert L.yk_trainer_ema_set(tr.handle, None, 0) == YK_ERR_STATE
    with pytest.raises(TR.YkError):
        tr.ema()
    for k in range(3):
        _do_step(tr, batches, k)
    assert tr.ema_state() == zeros
    p3 = tr.params().cpu().numpy().copy()
    tr.set_ema(0.9, 1)  # on at step 3: the shadow starts from the step-3 parameters with count 0
    assert tr.ema_state() == {"decay": 0.9, "every": 1, "updates": 0, "since": 0}
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(p3))
    _do_step(tr, batches, 3)
    e = ER.update(p3, tr.params().cpu().numpy(), ER.weight(0.9, 0))
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(e))
    # a bad set_ema leaves the knobs (and the shadow) as they were
    for decay, every in ((1.0, 1), (-0.5, 1), (float("nan"), 1), (0.5, 0), (0.5, -3)):
        assert L.yk_trainer_set_ema(tr.handle, decay, every) == YK_ERR_ARG
    assert tr.ema_state() == {"decay": 0.9, "every": 1, "updates": 1, "since": 0}
    # new values while on change only the two knobs
    tr.set_ema(0.5, 3)
    assert tr.ema_state() == {"decay": 0.5, "every": 3, "updates": 1, "since": 0}
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(e))
    # load_params leaves the shadow alone
    tr.load_params(_sd(64, 1))
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(e))
    p0 = tr.params().cpu().numpy().copy()
    assert not np.array_equal(p0, e)
    # load_ema(None, 0): the shadow is the parameters again
    tr.load_ema(None, 0)
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(p0)) and tr.ema_state()["updates"] == 0
    # off: the state errors are back; on again starts afresh
    tr.set_ema(0.0)
    assert tr.ema_state() == zeros and L.yk_trainer_ema_buffer(tr.handle, C.byref(p)) == YK_ERR_STATE
    _do_step(tr, batches, 4)
    tr.set_ema(0.9, 2)
    assert tr.ema_state() == {"decay": 0.9, "every": 2, "updates": 0, "since": 0}
    assert np.array_equal(_bits(tr.ema().cpu().numpy()), _bits(tr.params().cpu().numpy()))
    with pytest.raises(ValueError):
        _trainer(TR, False, ema_decay=0.0, ema_every=2)


# ------------------------------------------------------------------ 3. the wrapper
ARGS = dict(lr=2e-3, weight_decay=1e-4, epochs=2, batch_size=64, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1,
            dropout=0.3)


@pytest.fixture(scope="module")
def examples(Y):
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import HashPriorNet
    from yacht_amd.utils import dotdict
    game = YachtGame(seed=1, env_id=0)
    coach = Coach(game, HashPriorNet(game), dotdict(numMCTSSims=4, cpuct=1.5, tempThreshold=15))
    return game, [ex for ep in coach.executeEpisodes(4) for ex in ep]


def _sd_equal(a, b):
    return list(a.keys()) == list(b.keys()) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def test_wrapper_plays_the_shadow_and_checkpoints_both(Y, examples, tmp_path):
    from yacht_amd.nnet import NNetWrapper, YkNet
    from yacht_amd.state import pack
    from yacht_amd.utils import dotdict
    K = Y[0]
    game, ex = examples
    args = dotdict(ARGS, emaDecay=0.9)
    w = NNetWrapper(game, args)
    board = ex[0][0]
    assert w._ema_sd is None and w.yk_net(raw=True) is w.yk_net()  # no shadow yet: the raw weights are the average
    w.train(ex, verbose=False)
    steps = -(-len(ex) // 64) * 2
    assert w.ema_updates == steps and w._trainer().ema_state()["updates"] == steps
    # after train: predict is the shadow's net, the torch copy the raw iterate
    shadow = w.ema_state_dict()
    assert _sd_equal(shadow, w._trainer().ema_state_dict()) and _sd_equal(w.nnet.state_dict(), w._trainer().state_dict())
    assert not _sd_equal(shadow, w.nnet.state_dict())
    pi1, v1 = w.predict(board)
    S = K.states_to_device(pack(board))
    pe, ve = YkNet(shadow, 64, 1).predict_states(S)
    assert np.array_equal(_bits(pi1), _bits(pe[0].cpu().numpy())) and v1 == np.float32(ve[0].item())
    pr, vr = w.yk_net(raw=True).predict_states(S)
    assert not np.array_equal(pi1, pr[0].cpu().numpy())
    assert w.yk_net(raw=True) is not w.yk_net() and w.yk_net(raw=True) is w.yk_net(raw=True)
    # evaluate: the default is what plays
    ev_raw, ev_ema, ev = w.evaluate(ex, weights="raw"), w.evaluate(ex, weights="ema"), w.evaluate(ex)
    assert ev == ev_ema and ev_raw["loss"] != ev_ema["loss"] and ev_raw["n"] == ev_ema["n"] == len(ex)
    with pytest.raises(ValueError):
        w.evaluate(ex, weights="mean")
    # the checkpoint: the old three keys and the two new ones; "state_dict" is the raw iterate
    w.save_checkpoint(str(tmp_path), "both.pth.tar")
    ck = torch.load(os.path.join(tmp_path, "both.pth.tar"), map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "optimizer", "args", "ema_state_dict", "ema_updates"}
    assert _sd_equal(ck["state_dict"], w.nnet.state_dict()) and _sd_equal(ck["ema_state_dict"], shadow)
    assert ck["ema_updates"] == steps
    w2 = NNetWrapper(game, args)
    w2.load_checkpoint(str(tmp_path), "both.pth.tar", load_optimizer=True)
    pi2, v2 = w2.predict(board)
    assert np.array_equal(_bits(pi1), _bits(pi2)) and v1 == v2
    assert _sd_equal(w2.ema_state_dict(), shadow) and w2.ema_updates == steps
    assert _sd_equal(w2._trainer().ema_state_dict(), shadow) and w2._trainer().ema_state()["updates"] == steps
    m1, s1 = w._trainer().moments()
    m2, s2 = w2._trainer().moments()
    assert all(torch.equal(m1[k], m2[k]) and torch.equal(s1[k], s2[k]) for k in m1)
    assert w2._trainer().step_count == w._trainer().step_count
    # one more identical train call: the shadows still agree bit for bit.  (The GradScaler's scale is not part of
    # the reference checkpoint: the reloaded trainer starts at 65536 again, which is where the first one still
    # is - no step of this toy run overflows.)
    assert w.uses_amp() and w._trainer().amp_state()["scale"] == 65536.0 and w._trainer().step_count == steps
    w.train(ex, verbose=False)
    w2.train(ex, verbose=False)
    assert _sd_equal(w.ema_state_dict(), w2.ema_state_dict()) and w.ema_updates == w2.ema_updates == 2 * steps
    assert _sd_equal(w.nnet.state_dict(), w2.nnet.state_dict())


def test_wrapper_f32_retrain_after_reload_matches(Y, examples, tmp_path):
    """The float32 step has no state outside the checkpoint: after a reload one more identical train call
    leaves raw weights and shadow bit-identical."""
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    game, ex = examples
    args = dotdict(ARGS, emaDecay=0.9, amp=False)
    w = NNetWrapper(game, args)
    w.train(ex, verbose=False)
    w.save_checkpoint(str(tmp_path), "f32.pth.tar")
    w2 = NNetWrapper(game, args)
    w2.load_checkpoint(str(tmp_path), "f32.pth.tar", load_optimizer=True)
    w.train(ex, verbose=False)
    w2.train(ex, verbose=False)
    assert _sd_equal(w.ema_state_dict(), w2.ema_state_dict()) and w.ema_updates == w2.ema_updates
    assert _sd_equal(w.nnet.state_dict(), w2.nnet.state_dict())
    assert not _sd_equal(w.ema_state_dict(), w.nnet.state_dict())


def test_wrapper_off_keys_and_loading_across_the_knob(Y, examples, tmp_path):
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.state import pack
    from yacht_amd.utils import dotdict
    game, ex = examples
    off = NNetWrapper(game, dotdict(ARGS))
    off.train(ex, verbose=False)
    assert off._ema_sd is None and off._trainer().ema_state()["decay"] == 0.0
    off.save_checkpoint(str(tmp_path), "off.pth.tar")
    ck = torch.load(os.path.join(tmp_path, "off.pth.tar"), map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "optimizer", "args"}
    # on loads a file written with it off: the shadow is the loaded parameters, count 0
    on = NNetWrapper(game, dotdict(ARGS, emaDecay=0.9))
    on.train(ex, verbose=False)
    assert on.ema_updates > 0
    on.load_checkpoint(str(tmp_path), "off.pth.tar")
    assert on.ema_updates == 0 and _sd_equal(on.ema_state_dict(), off.nnet.state_dict())
    assert _sd_equal(on._trainer().ema_state_dict(), off.nnet.state_dict())
    assert on._trainer().ema_state()["updates"] == 0
    assert np.array_equal(on._trainer().ema().cpu().numpy(), on._trainer().params().cpu().numpy())
    pa, va = on.predict(ex[0][0])
    pb, vb = off.predict(ex[0][0])
    assert np.array_equal(_bits(pa), _bits(pb)) and va == vb
    # off loads a file written with it on: the extra keys are ignored
    on.train(ex, verbose=False)
    on.save_checkpoint(str(tmp_path), "on.pth.tar")
    off.load_checkpoint(str(tmp_path), "on.pth.tar")
    assert off._ema_sd is None and _sd_equal(off.nnet.state_dict(), on.nnet.state_dict())
    pc, _ = off.predict(ex[0][0])
    pr, _ = on.yk_net(raw=True).predict_states(Y[0].states_to_device(pack(ex[0][0])))
    assert np.array_equal(_bits(pc), _bits(pr[0].cpu().numpy()))


def test_export_and_evaluate_cli(Y, examples, tmp_path):
    from yacht_amd.evaluate import evaluate_files, load_examples_file
    from yacht_amd.examples_io import save_examples
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    game, ex = examples
    w = NNetWrapper(game, dotdict(ARGS, emaDecay=0.9))
    w.train(ex, verbose=False)
    w.save_checkpoint(str(tmp_path), "full.pth.tar")
    w.export_ema(str(tmp_path), "ema.pth.tar")
    ck = torch.load(os.path.join(tmp_path, "ema.pth.tar"), map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "args"} and _sd_equal(ck["state_dict"], w.ema_state_dict())
    plain = NNetWrapper(game, dotdict(ARGS))
    plain.load_checkpoint(str(tmp_path), "ema.pth.tar")
    pa, va = plain.predict(ex[0][0])
    pb, vb = w.predict(ex[0][0])
    assert np.array_equal(_bits(pa), _bits(pb)) and va == vb
    # the CLI: --weights ema on the full checkpoint == --weights raw on the exported file
    exfile = str(tmp_path / "ex.npz")
    save_examples(exfile, [ex])
    loaded = load_examples_file(exfile)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in [os.environ.get("PYTHONPATH")] if p]))

    def cli(model, *extra):
        r = subprocess.run([sys.executable, "-m", "yacht_amd.evaluate", "--model", str(tmp_path / model),
                            "--examples", exfile, *extra], capture_output=True, text=True, env=env, timeout=300)
        return r.returncode, [ln for ln in r.stdout.splitlines() if ln.strip()], r.stderr[-2000:]
    rc, out_ema, err = cli("full.pth.tar", "--weights", "ema")
    assert rc == 0 and len(out_ema) == 1, err
    rc, out_exp, err = cli("ema.pth.tar", "--weights", "raw")
    assert rc == 0 and len(out_exp) == 1, err
    a, b = json.loads(out_ema[0]), json.loads(out_exp[0])
    want_ema, want_raw = (json.loads(json.dumps(w.evaluate(loaded, weights=k))) for k in ("ema", "raw"))
    assert a == b == want_ema and a["n"] == len(ex) and want_raw["loss"] != a["loss"]
    # the default is today's: the checkpoint's "state_dict", the raw weights (in process: the same function)
    assert json.loads(json.dumps(evaluate_files(str(tmp_path / "full.pth.tar"), exfile))) == want_raw
    rc, out, err = cli("ema.pth.tar", "--weights", "ema")  # the exported file has no such key: refused, by name
    assert rc != 0 and not out and "ema_state_dict" in err
    with pytest.raises(KeyError, match="ema_state_dict"):
        evaluate_files(str(tmp_path / "ema.pth.tar"), exfile, weights="ema")


# ------------------------------------------------------------------ 4. the Coach
def test_coach_iteration_and_forced_rejection(Y, tmp_path):
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    d = str(tmp_path)
    args = dotdict(numIters=1, numEps=8, tempThreshold=15, updateThreshold=1.5, maxlenOfQueue=200000,
                   numMCTSSims=4, arenaCompare=4, cpuct=1.5, checkpoint=d, load_folder_file=(d, "best.pth.tar"),
                   numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=64,
                   vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.3, emaDecay=0.9, holdoutEps=2)
    game = YachtGame(seed=3, env_id=0)
    net = NNetWrapper(game, args)
    c = Coach(game, net, args)
    c.learn()
    assert sum(c.last_pit) == 4
    assert set(c.last_eval) == {"prev", "new", "new_raw"}
    assert c.last_eval["new"]["n"] == c.last_eval["new_raw"]["n"] == 2 * 48
    assert np.isfinite(c.last_eval["new_raw"]["loss"]) and c.last_eval["new_raw"] != c.last_eval["new"]
    # updateThreshold > 1: rejected - both sets are temp.pth.tar's again
    ck = torch.load(os.path.join(d, "temp.pth.tar"), map_location="cpu", weights_only=True)
    assert {"ema_state_dict", "ema_updates"} <= set(ck)
    assert _sd_equal(net.nnet.state_dict(), ck["state_dict"])
    assert _sd_equal(net.ema_state_dict(), ck["ema_state_dict"]) and net.ema_updates == ck["ema_updates"] == 0
    tr = net._trainer()
    assert _sd_equal(tr.state_dict(), ck["state_dict"]) and _sd_equal(tr.ema_state_dict(), ck["ema_state_dict"])
    assert tr.ema_state()["updates"] == 0
    assert not os.path.exists(os.path.join(d, "best.pth.tar"))
    # the previous net held the same two sets all along
    assert _sd_equal(c.pnet.ema_state_dict(), ck["ema_state_dict"])
