"""Both trainers held to a float64 step (tests/train_ref.py) at ragged and partial batches.

Every case: one Trainer whose max_batch differs from B (unless the case is the control), a batch
gathered through a shuffled idx out of a buffer three times as long, features from K.featurize
moved to the CPU so that both sides see the same bits, one backward - after a full max_batch
backward of other rows, as the last minibatch of an epoch follows full ones - then
tr.gradients() and tr.losses() against ref_step(..., float64).  tests/test_train_ref_host.py proves on the CPU that
the inputs cannot excuse a failure (no reference tensor near zero, the clip active where an update
is compared, torch float32 far inside the bounds).

Float32 trainer (csrc/yk_train.hip; the paths of gemm_rm each case reaches are in F32_PATHS):
per-tensor gradient relative norm < 1e-4 (the project's bound, test_gpu_train.py; torch float32
itself sits at 3e-6), ce / B and se / B within 1e-5 |ref| + 1e-6, the gradient sq-norm within
2.1e-4 (2 e + e^2 of the tensor bound); an empty soft row contributes exactly 0 cross-entropy.

Mixed-precision trainer (csrc/yk_train_amp.hip; tiles of 8 trunk rows, 16 head rows, 32-row dW
slices, every buffer strided by max_batch): the reference's own arithmetic is torch
autocast('cuda') + GradScaler on the GPU at the same init_scale; per tensor
d(ours, float64) <= 1.5 d(torch-AMP, float64) + 2e-3, each loss within
1.5 |torch-AMP - float64| + 1e-4 |ref| + 1e-7 (the factor and floors of
test_amp_steps_vs_torch_autocast_gradscaler), and the GradScaler state after apply() is torch's.

One optimiser step in both modes: the update p - p0 per tensor against the float64 step, no
further than 1.5 x torch's own distance (float32 on the CPU, floor 1e-3; AMP on the GPU, 2e-2).

Every test prints its worst tensor and the ratio to the reference's own error.

What the cases notice, checked once with arithmetic-only changes to the kernels: beta dropped in
the 64-wide NN k_sgemm, or 0.2 % added to the last split of its split-K pass - (512, 1, 961)
alone; the dW products' K rounded down to a multiple of 4 - every float32 case; k_amp_bwd reading
dpart with stride B instead of max_batch - every AMP case but the control; write_tl leaving a
32-row slice's padding rows unzeroed - the AMP cases whose last slice has whole 8-row pieces to
spare, which then hold what the full batch before left there; k_amp_masks ignoring the row offset - the
dropout case."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import train_ref as R  # noqa: E402

F32_PATHS = {
    (64, 1): "32-wide tiles with one-row and ragged tails; K = B not a multiple of 4; (B+3)/4 row blocks",
    (128, 2): "64-wide NT logits tiles with a one-row last tile; K = B over two and four 64-chunks",
    (512, 1): "the H = 512 instantiation; at B = 961 = 15 * 64 + 1 the only 64-wide NN tiles (16 x 8 = 128 of "
              "them): dA with split-K (4 splits of 832), dR1, and dH with beta = 1",
}
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


def _setup(K, H, NB, B, soft, dropout):
    """The case's device inputs and its CPU batch: (case, S, tg, vv, idx, csr, (X, target, values, masks))."""
    case = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))
    S = K.states_to_device(case["states"].copy())
    X = K.featurize(S).cpu().numpy()
    np.testing.assert_allclose(X, case["feat"], rtol=0, atol=1e-6)  # (the host file proved its inputs on these)
    idx64 = case["idx"].astype(np.int64)
    _, tgt, vals, masks = R.batch_of(case, soft, H, NB, B, dropout)
    tg = torch.tensor(case["targets"], device="cuda")
    vv = torch.tensor(case["values"], device="cuda")
    idx = torch.tensor(case["idx"], device="cuda")
    assert idx.dtype == torch.int32 and tg.dtype == torch.int32 and vv.dtype == torch.float32
    csr = tuple(torch.from_numpy(a).cuda() for a in R.csr_of(case["pi"])) if soft else None
    return case, S, tg, vv, idx, csr, (X[idx64], tgt, vals, masks)


def _ref(case, H, NB, B, soft, dropout, batch, dtype, update=False):
    key = (H, NB, B, soft, dropout, dtype, update)
    if key not in _REF:
        X, tgt, vals, masks = batch
        _REF[key] = R.ref_step(case["sd"], H, NB, X, tgt, vals, dtype, masks=masks, p=dropout, update=update)
    return _REF[key]


def _backward(tr, S, tg, vv, idx, csr, dropout):
    """A full max_batch backward of other rows first (hard targets, row offset 0), as every minibatch
    before an epoch's last one is: whatever it leaves in the max_batch-strided buffers, the dropout
    keep bits and the tiles' padding rows must not reach the batch under test.  Then that batch."""
    full = torch.arange(tr.max_batch, dtype=torch.int32, device="cuda").flip(0) % S.shape[0]
    tr.backward(S, tg, vv, idx=full)
    tr.backward(S, None if csr else tg, vv, idx=idx, row0=R.ROW0 if dropout else 0, policies=csr)


def _empty_row_alone(tr, case, S, tg, vv, csr):
    """The soft case's empty row (batch row 2) in a backward of its own: exactly 0 cross-entropy and
    no policy gradient at all, while the value head still learns from it."""
    row = int(case["idx"][2])
    assert not case["pi"][row].any()
    tr.backward(S, None, vv, idx=torch.tensor([row], dtype=torch.int32, device="cuda"), policies=csr)
    assert tr.losses()[0] == 0.0
    g = tr.gradients()
    assert not g["pi_head.2.bias"].numpy().any() and not g["pi_head.2.weight"].numpy().any()
    assert g["v_head.4.weight"].numpy().any()


# ---------------------------------------------------------------- the float32 trainer
@pytest.mark.parametrize("H,NB,max_batch,B,soft,dropout", R.F32_CASES)
def test_f32_step_vs_float64(T, H, NB, max_batch, B, soft, dropout):
    K, TR = T
    assert (max_batch == B) == (B == 961)
    case, S, tg, vv, idx, csr, batch = _setup(K, H, NB, B, soft, dropout)
    r64 = _ref(case, H, NB, B, soft, dropout, batch, torch.float64)
    r32 = _ref(case, H, NB, B, soft, dropout, batch, torch.float32)
    tr = TR.Trainer(case["sd"], H, NB, lr=2e-3, weight_decay=1e-4, max_batch=max_batch, vloss_weight=1.5,
                    dropout=dropout, seed=R.SEED_DROP, amp=False)
    _backward(tr, S, tg, vv, idx, csr, dropout)
    ce, se, _ = tr.losses()
    grads = {n: v.numpy() for n, v in tr.gradients().items()}  # (before the clip: backward() alone)
    tr.apply()
    sq = tr.losses()[2]
    rows = sorted((R.relnorm(grads[n], g), R.relnorm(r32["grads"][n], g), n) for n, g in r64["grads"].items())
    d, d32, name = rows[-1]
    print(f"f32 ({H}, {NB}, {B}) of {max_batch} soft={soft} p={dropout} [{F32_PATHS[(H, NB)]}]: worst {name} "
          f"{d:.3e} (torch float32 {d32:.3e}, ratio {d / max(d32, 1e-12):.2f}); ce {ce / B:.7f} ref {r64['ce']:.7f}; "
          f"mse {se / B:.7f} ref {r64['mse']:.7f}; sq-norm rel {abs(sq - r64['sqnorm']) / r64['sqnorm']:.3e}")
    for dd, _, n in rows:
        assert dd < 1e-4, ("grad", n, dd)
    assert abs(ce / B - r64["ce"]) <= 1e-5 * abs(r64["ce"]) + 1e-6, (ce / B, r64["ce"])
    assert abs(se / B - r64["mse"]) <= 1e-5 * abs(r64["mse"]) + 1e-6, (se / B, r64["mse"])
    assert abs(sq - r64["sqnorm"]) <= 2.1e-4 * r64["sqnorm"], (sq, r64["sqnorm"])
    if soft:
        _empty_row_alone(tr, case, S, tg, vv, csr)
    tr.close()


# ---------------------------------------------------------------- the mixed-precision trainer
def _torch_amp_step(case, H, NB, batch, dropout, init_scale):
    """The reference's GPU train step (NNet.py:141-155): autocast('cuda') + GradScaler('cuda'),
    clip 5.0, AdamW(2e-3, 1e-4) - losses, gradients after unscale_, parameters, scaler state."""
    X, tgt, vals, masks = batch
    model = R.make_model(case["sd"], H, NB, torch.float32, masks, dropout, device="cuda")
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    x, t, v = (torch.as_tensor(np.asarray(a)).cuda() for a in (X, tgt, vals))
    with torch.autocast("cuda"):
        loss, lp, lv = R.step_loss(model, x, t, v)
    scaler.scale(loss).backward()
    # fp16 overflow stays a factor 4 away on the reference side
    big = max(float(q.grad.abs().max()) for q in model.parameters())
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
    scale0 = R.amp_scale(B)
    tr = TR.Trainer(case["sd"], H, NB, lr=2e-3, weight_decay=1e-4, max_batch=max_batch, vloss_weight=1.5,
                    dropout=dropout, seed=R.SEED_DROP, amp=True, init_scale=scale0)
    _backward(tr, S, tg, vv, idx, csr, dropout)
    scale = tr.amp_state()["scale"]
    assert scale == scale0
    ce, se, _ = tr.losses()
    grads = {n: v.numpy().astype(np.float64) / scale for n, v in tr.gradients().items()}
    tr.apply()
    return tr, ce / B, se / B, grads


@pytest.mark.parametrize("H,NB,max_batch,B,soft,dropout", R.AMP_CASES)
def test_amp_step_vs_float64(T, H, NB, max_batch, B, soft, dropout):
    K, TR = T
    assert (max_batch == B) == (B == 128)  # (the control)
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
    print(f"amp ({H}, {NB}, {B}) of {max_batch} soft={soft} p={dropout} scale {R.amp_scale(B):g}: worst {name} "
          f"{d:.3e} (torch-AMP {damp:.3e}, ratio {d / max(damp, 1e-12):.2f}, {used:.2f} of the bound); "
          f"ce {ce:.7f} torch-AMP {ramp['ce']:.7f} ref {r64['ce']:.7f}; mse {mse:.7f} torch-AMP {ramp['mse']:.7f} "
          f"ref {r64['mse']:.7f}")
    for _, dd, da, n in rows:
        assert dd <= 1.5 * da + 2e-3, ("grad", n, dd, da)
    for k, ours in (("ce", ce), ("mse", mse)):
        assert abs(ours - r64[k]) <= 1.5 * abs(ramp[k] - r64[k]) + 1e-4 * abs(r64[k]) + 1e-7, (k, ours, ramp[k], r64[k])
    st = tr.amp_state()
    assert st["scale"] == ramp["scale"] and (st["steps"] == 1) == ramp["taken"] and st["found_inf"] == (not ramp["taken"])
    assert tr.step_count == st["steps"]
    if soft:
        _empty_row_alone(tr, case, S, tg, vv, csr)
    tr.close()


# ---------------------------------------------------------------- one optimiser step
@pytest.mark.parametrize("amp,H,NB,max_batch,B", R.UPDATE_CASES)
def test_one_step_update_vs_float64(T, amp, H, NB, max_batch, B):
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
        tr = TR.Trainer(case["sd"], H, NB, lr=2e-3, weight_decay=1e-4, max_batch=max_batch, vloss_weight=1.5,
                        dropout=0.0, amp=False)
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
    print(f"{'amp' if amp else 'f32'} update ({H}, {NB}, {B}) of {max_batch}: worst {name} {d:.3e} "
          f"(torch {'AMP' if amp else 'float32'} {dref:.3e}, ratio {d / max(dref, 1e-12):.2f}, {used:.2f} of the bound)")
    for _, dd, dr, n in rows:
        assert dd <= 1.5 * dr + floor, ("update", n, dd, dr)
    tr.close()
