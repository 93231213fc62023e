"""The legal-move mask on the GPU: both trainers with yk_trainer_set_legal_mask on held to
a float64 masked step (tests/mask_ref.py), the exact properties of the mask, the masked evaluation against its
float64 restatement, the contract checker, and NNetWrapper.train with args.maskIllegal end to end.

The bounds are those of tests/test_gpu_train_edges.py, taken over unchanged.  Float32 trainer: per-tensor
gradient relative norm < 1e-4 against float64, ce / B and se / B within 1e-5 |ref| + 1e-6, the gradient
sq-norm within 2.1e-4.  Mixed-precision trainer: per tensor d(ours, float64) <= 1.5 d(torch-AMP, float64) + 2e-3
and each loss within 1.5 |torch-AMP - float64| + 1e-4 |ref| + 1e-7, torch-AMP being torch autocast('cuda') +
GradScaler on the same masked loss on the GPU.  One optimiser step: the update p - p0 per tensor no further from
the float64 step than 1.5 x torch's own distance (float32 on the CPU, floor 1e-3; AMP on the GPU, 2e-2).

tests/test_mask_host.py proves on the CPU that the inputs cannot excuse a failure: the masked and the unmasked
float64 gradients differ by a relative norm >= 0.1 (measured: >= 0.22) in every tensor outside v_head, so a kernel that ignores the
mask is four orders of magnitude outside the float32 bound and two outside the mixed-precision one.

Every comparison prints its worst tensor before it asserts."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import eval_ref as E  # noqa: E402
import mask_ref as M  # noqa: E402
import train_ref as R  # noqa: E402
from oracle import spec  # noqa: E402

_REF = {}


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import kernels as K
    from yacht_amd import train
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return K, train


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the cases' arrays are read-only)


def _setup(K, H, NB, B, soft, dropout):
    """The case's device inputs and its CPU batch: (case, S, tg, vv, idx, csr, (X, target, values, valid, masks))."""
    case = M.mask_case(H, NB, B, M.case_seed(H, NB, B))
    S = K.states_to_device(case["states"].copy())
    X = K.featurize(S).cpu().numpy()
    np.testing.assert_allclose(X, case["feat"], rtol=0, atol=1e-6)  # (the host file proved its inputs on these)
    idx64 = case["idx"].astype(np.int64)
    _, tgt, vals, ok, masks = M.batch_of(case, soft, H, NB, B, dropout)
    tg, vv, idx = _dev(case["targets"]), _dev(case["values"]), _dev(case["idx"])
    assert idx.dtype == torch.int32 and tg.dtype == torch.int32 and vv.dtype == torch.float32
    csr = tuple(_dev(a) for a in R.csr_of(case["pi"])) if soft else None
    return case, S, tg, vv, idx, csr, (X[idx64], tgt, vals, ok, masks)


def _ref(case, H, NB, B, soft, dropout, batch, dtype, update=False):
    key = (H, NB, B, soft, dropout, dtype, update)
    if key not in _REF:
        X, tgt, vals, ok, masks = batch
        _REF[key] = M.ref_step(case["sd"], H, NB, X, tgt, vals, ok, dtype, masks=masks, p=dropout, update=update)
    return _REF[key]


def _trainer(TR, case, H, NB, max_batch, dropout, amp, B=None, legal_mask=True):
    kw = dict(init_scale=R.amp_scale(B)) if amp else {}
    return TR.Trainer(case["sd"], H, NB, lr=2e-3, weight_decay=1e-4, max_batch=max_batch, vloss_weight=1.5,
                      dropout=dropout, seed=R.SEED_DROP, amp=amp, legal_mask=legal_mask, **kw)


def _backward(tr, S, tg, vv, idx, csr, dropout):
    """A full max_batch backward of other rows first (hard targets, all valid; row offset 0), as every minibatch
    before an epoch's last one is - the legal bits it leaves in the max_batch-strided buffer must not reach the
    batch under test - then that batch."""
    full = torch.arange(tr.max_batch, dtype=torch.int32, device="cuda").flip(0) % S.shape[0]
    tr.backward(S, tg, vv, idx=full)
    tr.backward(S, None if csr else tg, vv, idx=idx, row0=R.ROW0 if dropout else 0, policies=csr)


# ---------------------------------------------------------------- 1. the float32 trainer
@pytest.mark.parametrize("H,NB,max_batch,B,soft,dropout", M.F32_CASES)
def test_f32_masked_step_vs_float64(T, H, NB, max_batch, B, soft, dropout):
    K, TR = T
    case, S, tg, vv, idx, csr, batch = _setup(K, H, NB, B, soft, dropout)
    r64 = _ref(case, H, NB, B, soft, dropout, batch, torch.float64)
    r32 = _ref(case, H, NB, B, soft, dropout, batch, torch.float32)
    tr = _trainer(TR, case, H, NB, max_batch, dropout, False)
    _backward(tr, S, tg, vv, idx, csr, dropout)
    ce, se, _ = tr.losses()
    grads = {n: v.numpy() for n, v in tr.gradients().items()}  # (before the clip: backward() alone)
    tr.apply()
    sq = tr.losses()[2]
    rows = sorted((R.relnorm(grads[n], g), R.relnorm(r32["grads"][n], g), n) for n, g in r64["grads"].items())
    d, d32, name = rows[-1]
    print(f"f32 masked ({H}, {NB}, {B}) of {max_batch} soft={soft} p={dropout}: worst {name} {d:.3e} (torch float32 "
          f"{d32:.3e}, ratio {d / max(d32, 1e-12):.2f}); ce {ce / B:.7f} ref {r64['ce']:.7f}; mse {se / B:.7f} ref "
          f"{r64['mse']:.7f}; sq-norm rel {abs(sq - r64['sqnorm']) / r64['sqnorm']:.3e}")
    for dd, _, n in rows:
        assert dd < 1e-4, ("grad", n, dd)
    assert abs(ce / B - r64["ce"]) <= 1e-5 * abs(r64["ce"]) + 1e-6, (ce / B, r64["ce"])
    assert abs(se / B - r64["mse"]) <= 1e-5 * abs(r64["mse"]) + 1e-6, (se / B, r64["mse"])
    assert abs(sq - r64["sqnorm"]) <= 2.1e-4 * r64["sqnorm"], (sq, r64["sqnorm"])
    tr.close()


# ---------------------------------------------------------------- 2. the mixed-precision trainer
def _torch_amp_step(case, H, NB, batch, dropout, init_scale):
    """The reference's GPU train step (NNet.py:141-155) on the masked loss: autocast('cuda') + GradScaler('cuda'),
    clip 5.0, AdamW(2e-3, 1e-4) - losses, gradients after unscale_, parameters, scaler state."""
    X, tgt, vals, ok, masks = batch
    model = R.make_model(case["sd"], H, NB, torch.float32, masks, dropout, device="cuda")
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    x, t, v, okt = (torch.as_tensor(np.asarray(a)).cuda() for a in (X, tgt, vals, ok))
    with torch.autocast("cuda"):
        loss, lp, lv = M.masked_loss(model, x, t, v, okt)
    scaler.scale(loss).backward()
    big = max(float(q.grad.abs().max()) for q in model.parameters())  # fp16 overflow stays a factor 4 away
    assert all(bool(torch.isfinite(q.grad).all()) for q in model.parameters()) and big < 2.0 ** 14, big
    scaler.unscale_(opt)
    grads = {n: q.grad.detach().double().cpu().numpy().copy() for n, q in model.named_parameters()}
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=5.0)
    scaler.step(opt)
    scaler.update()
    params = {n: q.detach().double().cpu().numpy().copy() for n, q in model.named_parameters()}
    taken = all(int(st["step"]) == 1 for st in opt.state.values()) and len(opt.state) > 0
    return dict(ce=float(lp.detach()), mse=float(lv.detach()), grads=grads, params=params,
                scale=scaler.get_scale(), taken=taken)


def _amp_step(TR, case, H, NB, max_batch, B, S, tg, vv, idx, csr, dropout):
    tr = _trainer(TR, case, H, NB, max_batch, dropout, True, B=B)
    _backward(tr, S, tg, vv, idx, csr, dropout)
    scale = tr.amp_state()["scale"]
    assert scale == R.amp_scale(B)
    ce, se, _ = tr.losses()
    grads = {n: v.numpy().astype(np.float64) / scale for n, v in tr.gradients().items()}
    tr.apply()
    return tr, ce / B, se / B, grads


@pytest.mark.parametrize("H,NB,max_batch,B,soft,dropout", M.AMP_CASES)
def test_amp_masked_step_vs_float64(T, H, NB, max_batch, B, soft, dropout):
    K, TR = T
    case, S, tg, vv, idx, csr, batch = _setup(K, H, NB, B, soft, dropout)
    r64 = _ref(case, H, NB, B, soft, dropout, batch, torch.float64)
    ramp = _torch_amp_step(case, H, NB, batch, dropout, R.amp_scale(B))
    tr, ce, mse, grads = _amp_step(TR, case, H, NB, max_batch, B, S, tg, vv, idx, csr, dropout)
    rows = []
    for n, g in r64["grads"].items():
        d, damp = R.relnorm(grads[n], g), R.relnorm(ramp["grads"][n], g)
        rows.append((d / (1.5 * damp + 2e-3), d, damp, n))
    rows.sort()
    used, d, damp, name = rows[-1]
    print(f"amp masked ({H}, {NB}, {B}) of {max_batch} soft={soft} scale {R.amp_scale(B):g}: worst {name} {d:.3e} "
          f"(torch-AMP {damp:.3e}, ratio {d / max(damp, 1e-12):.2f}, {used:.2f} of the bound); ce {ce:.7f} torch-AMP "
          f"{ramp['ce']:.7f} ref {r64['ce']:.7f}; mse {mse:.7f} torch-AMP {ramp['mse']:.7f} ref {r64['mse']:.7f}")
    for _, dd, da, n in rows:
        assert dd <= 1.5 * da + 2e-3, ("grad", n, dd, da)
    for k, ours in (("ce", ce), ("mse", mse)):
        assert abs(ours - r64[k]) <= 1.5 * abs(ramp[k] - r64[k]) + 1e-4 * abs(r64[k]) + 1e-7, (k, ours, ramp[k], r64[k])
    st = tr.amp_state()
    assert st["scale"] == ramp["scale"] and (st["steps"] == 1) == ramp["taken"] and st["found_inf"] == (not ramp["taken"])
    tr.close()


# ---------------------------------------------------------------- 3. one optimiser step
@pytest.mark.parametrize("amp,H,NB,max_batch,B", M.UPDATE_CASES)
def test_one_masked_step_update_vs_float64(T, amp, H, NB, max_batch, B):
    K, TR = T
    case, S, tg, vv, idx, csr, batch = _setup(K, H, NB, B, False, 0.0)
    r64 = _ref(case, H, NB, B, False, 0.0, batch, torch.float64, update=True)
    assert r64["gnorm"] > 5.0  # the clip is active
    if amp:
        other = _torch_amp_step(case, H, NB, batch, 0.0, R.amp_scale(B))
        assert other["taken"]
        tr = _amp_step(TR, case, H, NB, max_batch, B, S, tg, vv, idx, csr, 0.0)[0]
        assert tr.amp_state()["steps"] == 1
        floor = 2e-2
    else:
        other = _ref(case, H, NB, B, False, 0.0, batch, torch.float32, update=True)
        tr = _trainer(TR, case, H, NB, max_batch, 0.0, False)
        _backward(tr, S, tg, vv, idx, None, 0.0)
        tr.apply()
        floor = 1e-3
    assert tr.step_count == 1
    params = tr.state_dict()
    rows = []
    for n, p in r64["params"].items():
        p0 = case["sd"][n].numpy().astype(np.float64)
        d, dref = R.relnorm(params[n].numpy() - p0, p - p0), R.relnorm(other["params"][n] - p0, p - p0)
        rows.append((d / (1.5 * dref + floor), d, dref, n))
    rows.sort()
    used, d, dref, name = rows[-1]
    print(f"{'amp' if amp else 'f32'} masked update ({H}, {NB}, {B}) of {max_batch}: worst {name} {d:.3e} "
          f"(torch {'AMP' if amp else 'float32'} {dref:.3e}, ratio {d / max(dref, 1e-12):.2f}, {used:.2f} of the bound)")
    for _, dd, dr, n in rows:
        assert dd <= 1.5 * dr + floor, ("update", n, dd, dr)
    tr.close()


# ---------------------------------------------------------------- 4. the fused step
@pytest.mark.parametrize("H,NB,B,soft", [(64, 1, 63, False), (128, 2, 100, True)])
def test_amp_masked_fused_step_equals_backward_then_apply(T, H, NB, B, soft):
    """yk_trainer_step sums the gradient norm inside the gradient launches; backward() (here at a row offset:
    dropout is 0, it must not matter) + apply() re-reads G.  With the mask on: the same losses, the same grad
    sq-norm to 1e-12, the same GradScaler state and parameters (rtol 1e-6: the clip coefficient may move by an
    ulp) over 3 steps of other rows each - test_amp_fused_norm_step_equals_backward_then_apply's assertion."""
    K, TR = T
    case, S, tg, vv, _, _, _ = _setup(K, H, NB, B, soft, 0.0)
    csr = tuple(_dev(a) for a in R.csr_of(case["pi"])) if soft else None
    fused = _trainer(TR, case, H, NB, 128, 0.0, True, B=B)
    split = _trainer(TR, case, H, NB, 128, 0.0, True, B=B)
    perm = np.random.RandomState(5).permutation(3 * B).astype(np.int32)
    for k in range(3):
        idx = _dev(perm[k * B:(k + 1) * B])
        fused.step(S, None if soft else tg, vv, idx=idx, policies=csr)
        split.backward(S, None if soft else tg, vv, idx=idx, row0=5, policies=csr)
        split.apply()
        lf, ls = fused.losses(), split.losses()
        assert lf[0] == ls[0] and lf[1] == ls[1] and np.isfinite(ls).all(), (k, lf, ls)
        assert abs(lf[2] - ls[2]) <= 1e-12 * ls[2], (k, lf[2], ls[2])
        assert fused.amp_state() == split.amp_state(), k
        np.testing.assert_allclose(fused.params().cpu().numpy(), split.params().cpu().numpy(), rtol=1e-6, atol=1e-9)
    assert fused.amp_state()["steps"] == 3
    fused.close()
    split.close()


# ---------------------------------------------------------------- 5. exact properties
def _bits(d):
    return {n: v.numpy().view(np.uint32).copy() for n, v in d.items()}


def _one_step(tr, S, tg, vv, idx, csr=None):
    """backward + apply -> (losses after backward, gradient bits before the clip, parameter bits after)."""
    tr.backward(S, None if csr else tg, vv, idx=idx, policies=csr)
    ls = tr.losses()[:2].copy()
    g = _bits(tr.gradients())
    tr.apply()
    return ls, g, _bits(tr.state_dict())


@pytest.mark.parametrize("amp", [False, True])
def test_mask_switched_on_then_off_is_a_trainer_that_never_had_it(T, amp):
    K, TR = T
    H, NB, mb, B = M.EXACT_CASE
    case, S, tg, vv, idx, _, _ = _setup(K, H, NB, B, False, 0.0)
    never = _trainer(TR, case, H, NB, mb, 0.0, amp, B=B, legal_mask=False)
    toggled = _trainer(TR, case, H, NB, mb, 0.0, amp, B=B, legal_mask=True)
    masked = _trainer(TR, case, H, NB, mb, 0.0, amp, B=B, legal_mask=True)
    assert toggled.legal_mask and not never.legal_mask
    toggled.backward(S, tg, vv, idx=idx)  # a masked backward leaves its bits and its -inf logits behind
    toggled.set_legal_mask(False)
    assert not toggled.legal_mask
    a, b, c = (_one_step(t, S, tg, vv, idx) for t in (never, toggled, masked))
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], c[0])  # (the mask itself changes the loss)
    for n in a[1]:
        assert np.array_equal(a[1][n], b[1][n]) and np.array_equal(a[2][n], b[2][n]), n
    assert any(not np.array_equal(a[1][n], c[1][n]) for n in a[1])
    for t in (never, toggled, masked):
        t.close()


@pytest.mark.parametrize("rows", ["batch", "narrow"])
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("amp", [False, True])
def test_perturbed_invalid_logits_change_nothing(T, amp, soft, rows):
    """+50.0 on pi_head.2.bias at every column invalid in all batch rows, through yk_trainer_set: the losses,
    every gradient and every updated parameter (but those bias entries themselves) keep their bits, and the bias
    and weight-row gradients at those columns are exactly 0.  "batch": the case's whole batch, whose valid sets
    cover every column (the statement is then about nothing); "narrow": its rows of one valid action and of one
    or two occupied head parts, which leave more than 100 columns never valid (tests/test_mask_host.py)."""
    K, TR = T
    H, NB, mb, B = M.EXACT_CASE
    case, S, tg, vv, idx, _, _ = _setup(K, H, NB, B, soft, 0.0)
    csr = tuple(_dev(a) for a in R.csr_of(case["pi"])) if soft else None
    if rows == "narrow":
        sub = M.idx_narrow_rows(case)
        idx = _dev(sub)
        dead = M.never_valid(case, sub)
        assert len(dead) > 100
    else:
        dead = M.never_valid(case)
    base = _trainer(TR, case, H, NB, mb, 0.0, amp, B=B)
    pert = _trainer(TR, case, H, NB, mb, 0.0, amp, B=B)
    sd = {k: v.clone() for k, v in case["sd"].items()}
    sd["pi_head.2.bias"][torch.as_tensor(dead, dtype=torch.long)] += 50.0
    pert.load_params(sd)
    a, b = _one_step(base, S, tg, vv, idx, csr), _one_step(pert, S, tg, vv, idx, csr)
    assert np.isfinite(a[0]).all() and np.array_equal(a[0], b[0]), (a[0], b[0])
    live = np.setdiff1d(np.arange(M.A), dead)
    for n in a[1]:
        assert np.array_equal(a[1][n], b[1][n]), ("grad", n)
        if n == "pi_head.2.bias":
            assert np.array_equal(a[2][n][live], b[2][n][live]), n
        else:
            assert np.array_equal(a[2][n], b[2][n]), ("param", n)
    for t in (a, b):
        assert not t[1]["pi_head.2.bias"][dead].any() and not t[1]["pi_head.2.weight"][dead].any()
    # (and at every column invalid in a row, the row's own dlogit is 0: the bias gradient of a one-row batch)
    j = int(np.flatnonzero(case["cats"][idx.cpu().numpy()] == 2)[0])  # a row of several valid actions
    one = idx[j:j + 1]
    base.backward(S, None if soft else tg, vv, idx=one, policies=csr)
    g = base.gradients()["pi_head.2.bias"].numpy()
    ok = case["valid"][int(one[0])]
    assert not g[~ok].any() and g[ok].any()
    base.close()
    pert.close()


# ---------------------------------------------------------------- 6. the masked evaluation
def _evaluate(net, name, S, tg, vv, csr, idx, n, chunk):
    import yacht_amd
    rows = torch.full((n, 16), 7.0, dtype=torch.float64, device="cuda")
    sums = (C.c_double * 16)()
    p = [t.data_ptr() for t in csr] if csr is not None else [None] * 3
    rc = getattr(yacht_amd.lib(), name)(net.handle, S.data_ptr(), tg.data_ptr(), vv.data_ptr(), *p, idx.data_ptr(), n,
                                        chunk, rows.data_ptr(), sums, None)
    assert rc == 0
    return rows.cpu().numpy(), np.array(list(sums))


@pytest.mark.parametrize("use_csr", [False, True])
def test_evaluate_legal_against_float64(T, use_csr):
    """n = 100 rows of the mask's categories through a batch_idx, chunk 37 (three chunks, the last partial) and
    chunk 0.  Columns 0, 1, 3, 5, 6, 7 within rtol 1e-11 and atol 1e-11 (1 + max|x| over the valid actions) of
    the float64 restatement - tests/test_gpu_eval.py's bound, derived there - the counting columns and 8-10
    exact, column 4 within 1e-12 of 1, the sums in the fixed order; yk_net_evaluate on the same rows still
    returns the unmasked numbers."""
    K, _ = T
    from yacht_amd import nnet as N
    n = 100
    case, S, tg, vv, idx, _, _ = _setup(K, 64, 1, n, use_csr, 0.0)
    csr_h = R.csr_of(case["pi"]) if use_csr else None
    csr = tuple(_dev(a) for a in csr_h) if use_csr else None
    net = N.YkNet(spec.closed_form_weights(64, 1), 64, 1)
    lg, v = net.logits(S[idx.long()])
    x, vh = lg.cpu().numpy()[:, :M.A], v.cpu().numpy()
    want = M.eval_rows(x, vh, case["valid"], case["targets"], case["values"], csr_h, batch_idx=case["idx"])
    plain = E.rows(x, vh, case["valid"], case["targets"], case["values"], csr_h, batch_idx=case["idx"])
    ok = case["valid"][case["idx"].astype(np.int64)]
    atol = 1e-11 * (1.0 + np.abs(np.where(ok, x, 0.0)).max(1))
    exact = [2, 11, 12, 13, 14, 15]
    first = None
    for chunk in (37, 0):
        got, sums = _evaluate(net, "yk_net_evaluate_legal", S, tg, vv, csr, idx, n, chunk)
        assert np.isfinite(got).all()
        assert np.array_equal(got[:, exact], want[:, exact])
        assert np.array_equal(got[:, 8:11].view(np.uint64), want[:, 8:11].view(np.uint64))
        for col in (0, 1, 3, 5, 6, 7):
            err = np.abs(got[:, col] - want[:, col])
            tol = 1e-11 * np.abs(want[:, col]) + atol
            print(f"masked csr {use_csr} chunk {chunk} col {col}: max err / tol {float((err / tol).max()):.3g}")
            assert (err <= tol).all(), (col, int(np.argmax(err / tol)))
        assert np.abs(got[:, 4] - 1.0).max() <= 1e-12
        assert np.array_equal(sums.view(np.uint64), E.sums(got).view(np.uint64))
        if first is None:
            first = got
        assert np.array_equal(got.view(np.uint64), first.view(np.uint64))  # the chunk does not enter
    assert (got[:, 0] < plain[:, 0]).all() and (got[:, 1] < plain[:, 1]).all()  # lse' < lse
    assert (got[:, 2] <= plain[:, 2]).all() and (got[:, 2] < ok.sum(1)).all()   # a rank among the valid actions
    old, _ = _evaluate(net, "yk_net_evaluate", S, tg, vv, csr, idx, n, 37)
    assert np.array_equal(old[:, exact], plain[:, exact])
    atol_u = 1e-11 * (1.0 + np.abs(x).max(1))
    for col in (0, 1, 3, 4, 5, 6, 7):
        assert (np.abs(old[:, col] - plain[:, col]) <= 1e-11 * np.abs(plain[:, col]) + atol_u).all(), col
    assert (old[:, 4] < 1.0).all()
    out = net.evaluate(S, tg, vv, policies=csr, idx=idx, masked=True, per_row=True)  # the Python surface
    assert np.array_equal(out["rows"].cpu().numpy().view(np.uint64), first.view(np.uint64))
    assert out["valid_mass"] == pytest.approx(1.0, abs=1e-12)


# ---------------------------------------------------------------- 7. the contract checker
def test_check_legal_names_the_first_offender(T):
    K, _ = T
    B = 100
    case, S, tg, vv, idx, _, _ = _setup(K, 64, 1, B, True, 0.0)
    indptr, cols, vals = R.csr_of(case["pi"])
    csr = tuple(_dev(a) for a in (indptr, cols, vals))
    assert K.check_legal(S, tg, csr, idx=idx) == (-1, 0)
    assert K.check_legal(S, tg, csr) == (-1, 0) and K.check_legal(S) == (-1, 0)  # (the whole buffer; states alone)
    order = case["idx"].astype(np.int64)
    ok = case["valid"]

    def invalid_of(r):
        return int(np.flatnonzero(~ok[r])[-1])
    # one target moved to an invalid column (batch position 41)
    t2 = case["targets"].copy()
    t2[order[41]] = invalid_of(order[41])
    assert K.check_legal(S, _dev(t2), csr, idx=idx) == (41, 2)
    t2[order[77]] = -1  # a later one, out of range: the lowest row is reported
    assert K.check_legal(S, _dev(t2), csr, idx=idx) == (41, 2)
    t3 = case["targets"].copy()
    t3[order[9]] = M.A
    assert K.check_legal(S, _dev(t3), csr, idx=idx) == (9, 2)
    assert K.check_legal(S, None, csr, idx=idx) == (-1, 0)  # targets not given: not checked
    # one CSR column moved to an invalid column (the last entry of batch position 58's row)
    c2 = cols.copy()
    c2[indptr[order[58] + 1] - 1] = invalid_of(order[58])
    bad = (_dev(indptr), _dev(c2), _dev(vals))
    assert K.check_legal(S, tg, bad, idx=idx) == (58, 3)
    assert K.check_legal(S, _dev(t2), bad, idx=idx) == (41, 2)  # position 41's target comes first
    v0 = vals.copy()
    v0[indptr[order[58] + 1] - 1] = 0.0  # p == 0 there: no violation
    assert K.check_legal(S, tg, (_dev(indptr), _dev(c2), _dev(v0)), idx=idx) == (-1, 0)
    # a state without a valid action inserted at batch position 3 (and one at 90)
    F = M.fixture()
    empty = F["states"][np.flatnonzero(F["cat"] == -1)[:2]]
    W = case["states"].copy()
    W[order[3]], W[order[90]] = empty[0], empty[1]
    assert K.check_legal(K.states_to_device(W), tg, csr, idx=idx) == (3, 1)
    assert K.check_legal(K.states_to_device(W), _dev(t2), bad, idx=idx) == (3, 1)


@pytest.mark.parametrize("symmetries", [("carry",), ("rolls",), ("groups",), ("carry", "rolls", "groups")])
def test_augmented_examples_keep_the_contract(T, symmetries):
    """K.augment_examples of 64 rows (every category of valid set) under every symmetry group: the boards keep a
    valid action, the mapped hard targets and policy columns stay valid - masked training may follow it."""
    K, _ = T
    case, S, tg, vv, idx, _, _ = _setup(K, 64, 1, 64, True, 0.0)
    order = idx.long()
    indptr, cols, vals = R.csr_of(case["pi"][case["idx"].astype(np.int64)])
    csr = (_dev(indptr), _dev(cols), _dev(vals))
    for key in (0, 1, 2):
        s2, t2, p2 = K.augment_examples(S[order].contiguous(), tg[order].contiguous(), csr, 17, key, symmetries)
        assert K.check_legal(s2, t2, p2) == (-1, 0), key
    assert not torch.equal(s2, S[order])  # (the augmentation did something)


# ---------------------------------------------------------------- 8. end to end
ARGS = dict(numMCTSSims=4, cpuct=1.5, tempThreshold=15, lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=64,
            vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3)


@pytest.fixture(scope="module")
def games(T):
    """4 hash-prior self-play games x 4 simulations: 192 examples."""
    from yacht_amd import engine, replay
    eng = engine.SelfPlayEngine(4, 4, 1.5, 15, prior="hash", max_moves=48)
    eng.run(31, 0)
    assert eng.stats()["errors"] == 0
    img = eng.pack_records()
    eng.close()
    sh = replay.examples_from_images(img, 4, 48, 4)
    assert len(sh) == 192
    return sh


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("target", ["argmax", "visits"])
def test_wrapper_trains_with_mask_illegal(T, games, amp, target):
    K, _ = T
    from yacht_amd import replay
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    torch.manual_seed(5)
    net = NNetWrapper(YachtGame(seed=21, env_id=500), dotdict(ARGS, amp=amp, maskIllegal=True, policy_target=target))
    before = {k: v.clone() for k, v in net.nnet.state_dict().items()}
    net.train(games, verbose=False)
    tr = net._trainer()
    n0 = tr.step_count  # 192 examples, batch 64, one epoch: 3 steps (GradScaler may skip one under amp)
    assert tr.legal_mask and (1 <= n0 <= 3 if amp else n0 == 3)
    after = net.nnet.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert all(not torch.equal(after[k], before[k]) for k in after)
    on, off = net.evaluate(games, masked=True), net.evaluate(games, masked=False)
    assert on["masked"] is True and off["masked"] is False and net.evaluate(games) == on  # None follows the knob
    assert on["policy_ce"] < off["policy_ce"] and on["policy_ce_soft"] < off["policy_ce_soft"]
    assert on["valid_mass"] == pytest.approx(1.0, abs=1e-12) and off["valid_mass"] < 1.0
    assert on["value_mse"] == off["value_mse"]
    # a pool with one corrupted target (argmax) / policy column (visits): ValueError before any step
    ok = K.unpack_mask(K.valid_mask(games.states, 1)[0]).bool()
    row = 100
    col = int(torch.nonzero(~ok[row])[0])
    P = dict(games.policies)
    targets = games.targets.clone()
    if target == "argmax":
        targets[row] = col
    else:
        P["pi_cols"] = P["pi_cols"].clone()
        P["pi_cols"][int(P["pi_indptr"][row])] = col
    bad = replay.ExampleShard(games.states, targets, games.values, policies=P, outcomes=games.outcomes)
    with pytest.raises(ValueError, match=f"example {row} "):
        net.train(bad, verbose=False)
    assert tr.step_count == n0
    net.train([games, games], verbose=False)  # (a clean pool still trains)
    assert tr.step_count > n0 and (amp or tr.step_count == 9)
