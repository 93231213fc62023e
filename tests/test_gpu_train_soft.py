"""Soft policy targets on the GPU (yk_trainer_backward_soft / yk_trainer_step_soft,
NNetWrapper.train with policy_target="visits"): the policy head trained on the full MCTS visit
policy, loss F.cross_entropy(logits, pi) with probability targets.

* a one-hot CSR is the hard-target step, bit for bit, in both trainers;
* against torch float32 and torch autocast + GradScaler with the dense pi as the target, under
  the tolerances tests/test_gpu_train.py states for the hard step (same shapes, same formulas);
* unnormalised and empty rows, the gather through batch_idx, the fused-norm step, and the public
  classes (self-play -> ExampleShard -> NNetWrapper.train).
"""
import numpy as np
import pytest

from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = 3226
EDGE_COLS = [0, 31, 32, 3199, 3200, 3225]  # first / last action, a slice edge, the partial last slice


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import kernels as K
    from yacht_amd import nnet, train
    return K, nnet, train


def _sd(hidden, nblocks):
    return {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in spec.closed_form_weights(hidden, nblocks).items()}


def _relnorm(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _csr_of(pi):
    """dense float64 [n, 3226] -> device CSR of its nonzero entries (columns ascending)."""
    r, c = np.nonzero(pi)
    indptr = np.zeros(len(pi) + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=len(pi)), out=indptr[1:])
    return tuple(torch.from_numpy(x).cuda() for x in (indptr, c.astype(np.int32), pi[r, c].astype(np.float64)))


def _onehot_csr(tg):
    n = tg.numel()
    return (torch.arange(n + 1, dtype=torch.int64, device="cuda"), tg.to(torch.int32).contiguous(),
            torch.ones(n, dtype=torch.float64, device="cuda"))


def _bits(tr):
    """Everything a step leaves behind, as bytes: parameters, gradients, both moments."""
    m, v = tr.moments()
    return (tr.params().cpu().numpy().tobytes(), tr.grads().cpu().numpy().tobytes(),
            b"".join(m[k].numpy().tobytes() for k in m), b"".join(v[k].numpy().tobytes() for k in v))


@pytest.fixture(scope="module")
def visit_targets():
    """1536 visit policies as the engine makes them: counts / counts.sum() in float64, nnz drawn from
    {1, 2, 25, 100}; row 0 holds the edge columns, row 1 every action.  Computed once, shared."""
    rng = np.random.RandomState(21)
    n = 1536
    pi = np.zeros((n, A), dtype=np.float64)
    for i in range(n):
        nnz = int(rng.choice([1, 2, 25, 100]))
        cols = rng.choice(A, nnz, replace=False)
        if i == 0:
            cols = np.unique(np.concatenate([EDGE_COLS, rng.choice(A, 19, replace=False)]))
        if i == 1:
            cols = np.arange(A)
        counts = rng.randint(1, 20, len(cols)).astype(np.float64)
        pi[i, cols] = counts / counts.sum()
    assert all(pi[0, c] > 0 for c in EDGE_COLS) and (pi[1] > 0).all()
    assert {int(k) for k in np.unique((pi[:64] > 0).sum(1))} >= {1, 2, 25, 100}
    return pi


def _model_weights(N, H, NB, seed):
    torch.manual_seed(seed)
    model = N.YachtNNet(hidden=H, nblocks=NB, dropout=0.0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _data(K, golden, n, seed):
    W = golden("states.npz")["states"]
    W = np.concatenate([W] * (n // len(W) + 1))[:n]
    rng = np.random.RandomState(seed)
    S = K.states_to_device(W)
    vv = torch.tensor(rng.rand(n) * 2 - 1, dtype=torch.float32, device="cuda")
    return S, K.featurize(S), vv, rng


# ---------------------------------------------------------------- 1. one-hot == hard targets
@pytest.mark.parametrize("amp,H,NB,B,dropout", [
    (False, 64, 1, 63, 0.0), (False, 256, 6, 128, 0.0), (False, 64, 1, 63, 0.3),
    (True, 64, 1, 63, 0.0), (True, 128, 2, 32, 0.0), (True, 256, 6, 128, 0.0), (True, 128, 2, 32, 0.3)])
def test_onehot_csr_is_the_hard_step_bit_for_bit(T, golden, amp, H, NB, B, dropout):
    """The CSR of onehot(tg) through step_soft against Trainer.step(states, tg, ...): 3 steps over a
    permuted idx, byte-equal parameters, gradients, moments, losses, epoch loss and GradScaler
    state.  B = 63 / 32: the ragged last tile, the single-slice batch; H = 64: waves without
    columns; H = 128: the AMP width no other test runs."""
    K, N, TR = T
    S, _, vv, rng = _data(K, golden, 3 * B, 31)
    tg = torch.tensor(rng.randint(0, A, 3 * B), dtype=torch.int32, device="cuda")
    tg[:6] = torch.tensor(EDGE_COLS, dtype=torch.int32)
    perm = torch.tensor(rng.permutation(3 * B), dtype=torch.int32, device="cuda")
    csr = _onehot_csr(tg)
    kw = dict(max_batch=B, dropout=dropout, seed=17, amp=amp)
    hard, soft = TR.Trainer(_sd(H, NB), H, NB, **kw), TR.Trainer(_sd(H, NB), H, NB, **kw)
    hard.epoch_loss_begin(1.5)
    soft.epoch_loss_begin(1.5)
    for k in range(3):
        idx = perm[k * B:(k + 1) * B].contiguous()
        hard.step(S, tg, vv, idx=idx)
        soft.step(S, None, vv, idx=idx, policies=csr)
        assert hard.losses().tobytes() == soft.losses().tobytes(), k
    assert _bits(hard) == _bits(soft)
    assert hard.epoch_loss_end() == soft.epoch_loss_end()
    if amp:
        assert hard.amp_state() == soft.amp_state()
    assert hard.step_count == soft.step_count


# ---------------------------------------------------------------- 2. against torch float32
def _torch_step_reference(model, opt, x, pi, v, vw=1.5):
    import torch.nn.functional as F
    opt.zero_grad(set_to_none=True)
    out_pi, out_v = model(x)
    lp = F.cross_entropy(out_pi, pi)
    lv = F.mse_loss(out_v, v.reshape(-1, 1))
    loss = lp + vw * lv
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=5.0)
    opt.step()
    return float(lp.detach()), float(lv.detach())


def test_three_soft_steps_vs_torch_fp32(T, golden, visit_targets):
    """test_gpu_train.py::test_three_steps_vs_torch_fp32 with F.cross_entropy(out_pi, pi_dense) in
    the reference's place: its shape, its 3 steps, its tolerances."""
    K, N, TR = T
    H, NB, B = 256, 6, 128
    torch.manual_seed(3)
    model = N.YachtNNet(hidden=H, nblocks=NB, dropout=0.0).cuda().float().train()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    tr = TR.Trainer(sd0, H, NB, lr=2e-3, weight_decay=1e-4, max_batch=B, vloss_weight=1.5, dropout=0.0)
    torch.backends.cuda.matmul.allow_tf32 = False
    S, X, vv, _ = _data(K, golden, 3 * B, 0)
    pi = visit_targets[:3 * B]
    csr = _csr_of(pi)
    pi32 = torch.as_tensor(pi).float().cuda()
    tr.epoch_loss_begin(1.5)
    total = 0.0
    for k in range(3):
        sl = slice(k * B, (k + 1) * B)
        idx = torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device="cuda")
        tr.step(S, None, vv, idx=idx, policies=csr)
        lp, lv = _torch_step_reference(model, opt, X[sl], pi32[sl], vv[sl])
        ce, se, _ = tr.losses()
        print(f"step {k}: ce {ce / B:.7f} torch {lp:.7f}; mse {se / B:.7f} torch {lv:.7f}")
        assert abs(ce / B - lp) <= 1e-5 * abs(lp) + 1e-6 and abs(se / B - lv) <= 1e-5 * abs(lv) + 1e-6
        total += ce / B + 1.5 * se / B
    assert tr.epoch_loss_end() == (total, 3)
    grads = tr.gradients()
    params = tr.state_dict()
    m, v2 = tr.moments()
    for name, p in model.named_parameters():
        assert _relnorm(grads[name].numpy(), p.grad.detach().cpu().numpy()) < 1e-4, "grad " + name
        p_ref = p.detach().cpu().numpy()
        assert _relnorm(params[name].numpy() - sd0[name].numpy(), p_ref - sd0[name].numpy()) < 1e-3, "update " + name
        assert (np.abs(params[name].numpy() - p_ref) > 1e-5).mean() <= 1e-4, "param " + name
        st = opt.state[p]
        assert _relnorm(m[name].numpy(), st["exp_avg"].cpu().numpy()) < 1e-4, "exp_avg " + name
        assert _relnorm(v2[name].numpy(), st["exp_avg_sq"].cpu().numpy()) < 2e-4, "exp_avg_sq " + name
    assert tr.step_count == 3


# ---------------------------------------------------------------- 3. against torch autocast + GradScaler
def _torch_train_steps(sd0, H, NB, X, pi, vv, B, steps, amp, vw=1.5, init_scale=65536.0):
    """The reference's train() inner loop (NNet.py:132-165) on the GPU with the dense pi as the
    cross-entropy target: autocast('cuda') + GradScaler('cuda') (amp) or float32, AdamW, clip 5.0."""
    import torch.nn.functional as F
    from yacht_amd.nnet import YachtNNet
    model = YachtNNet(hidden=H, nblocks=NB, dropout=0.0).cuda().float()
    model.load_state_dict(sd0)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale) if amp else None
    losses, grads1 = [], None
    for k in range(steps):
        sl = slice(k * B, (k + 1) * B)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", enabled=amp):
            out_pi, out_v = model(X[sl])
            lp = F.cross_entropy(out_pi, pi[sl])
            lv = F.mse_loss(out_v, vv[sl].reshape(-1, 1))
            loss = lp + vw * lv
        if amp:
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
        else:
            loss.backward()
        if k == 0:
            grads1 = {n: p.grad.detach().float().cpu().numpy().copy() for n, p in model.named_parameters()}
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=5.0)
        if amp:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        losses.append((float(lp.detach()), float(lv.detach())))
    params = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    return params, losses, grads1, (scaler.get_scale() if amp else None)


@pytest.mark.parametrize("H,NB,B", [(256, 6, 512), (64, 1, 128)])
def test_soft_amp_steps_vs_torch_autocast_gradscaler(T, golden, visit_targets, H, NB, B):
    """test_gpu_train.py::test_amp_steps_vs_torch_autocast_gradscaler with the dense pi as the
    target: no further from torch-AMP than torch float32 is, x 1.5, plus that test's floors -
    losses, step-1 gradients, parameters; scale and step count equal."""
    K, N, TR = T
    sd0 = _model_weights(N, H, NB, 11)
    S, X, vv, _ = _data(K, golden, 3 * B, 4)
    pi = visit_targets[:3 * B]
    csr = _csr_of(pi)
    pi32 = torch.as_tensor(pi).float().cuda()
    torch.backends.cuda.matmul.allow_tf32 = False
    p_amp, l_amp, g_amp, scale_amp = _torch_train_steps(sd0, H, NB, X, pi32, vv, B, 3, True)
    p_f32, l_f32, g_f32, _ = _torch_train_steps(sd0, H, NB, X, pi32, vv, B, 3, False)
    tr = TR.Trainer(sd0, H, NB, lr=2e-3, weight_decay=1e-4, max_batch=B, vloss_weight=1.5, dropout=0.0, amp=True)
    ours_l = []
    g1 = None
    for k in range(3):
        idx = torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device="cuda")
        tr.backward(S, None, vv, idx=idx, policies=csr)
        if k == 0:
            scale = tr.amp_state()["scale"]
            g1 = {n: v.numpy() / scale for n, v in tr.gradients().items()}
        tr.apply()
        ce, se, _ = tr.losses()
        ours_l.append((ce / B, se / B))
    tol = lambda ref_gap, ref: 1.5 * ref_gap + 1e-4 * abs(ref) + 1e-7
    for k in range(3):
        for j in range(2):
            gap = abs(l_f32[k][j] - l_amp[k][j])
            print(f"step {k} loss[{j}]: ours {ours_l[k][j]:.7f} torch-amp {l_amp[k][j]:.7f} torch-f32 {l_f32[k][j]:.7f}")
            assert abs(ours_l[k][j] - l_amp[k][j]) <= tol(gap, l_amp[k][j]), (k, j)
    worst = []
    for name in g_amp:
        d_ours = _relnorm(g1[name], g_amp[name])
        d_f32 = _relnorm(g_f32[name], g_amp[name])
        worst.append((d_ours / max(d_f32, 1e-12), name, d_ours, d_f32))
        assert d_ours <= 1.5 * d_f32 + 2e-3, ("grad", name, d_ours, d_f32)
    print("worst grad ratios:", sorted(worst)[-3:])
    params = tr.state_dict()
    for name in p_amp:
        p0 = sd0[name].numpy()
        d_ours = _relnorm(params[name].numpy() - p0, p_amp[name] - p0)
        d_f32 = _relnorm(p_f32[name] - p0, p_amp[name] - p0)
        assert d_ours <= 1.5 * d_f32 + 2e-2, ("update", name, d_ours, d_f32)
    st = tr.amp_state()
    assert st["scale"] == scale_amp and tr.step_count == st["steps"]


# ---------------------------------------------------------------- 4. unnormalised and empty rows
@pytest.mark.parametrize("amp", [False, True])
def test_unnormalised_and_empty_rows(T, golden, visit_targets, amp):
    """s = sum p is not assumed to be 1: a third of the rows scaled to sum 0.5, one row without
    entries.  One step at (64, 1, 32) against torch with that dense target, under tests 2 and 3's
    tolerances; the empty row's cross-entropy and policy gradient are exactly 0.
    (amp: loss scale 2^10 on both sides.  At batch 32 the default 2^16 overflows fp16 in
    v_head.4.weight's gradient - in torch's step too, which GradScaler would skip - and inf
    against inf compares nothing.)"""
    K, N, TR = T
    H, NB, B = 64, 1, 32
    sd0 = _model_weights(N, H, NB, 5)
    S, X, vv, _ = _data(K, golden, B, 8)
    pi = visit_targets[:B].copy()
    pi[::3] *= 0.5
    pi[7] = 0.0
    assert abs(pi[3].sum() - 0.5) < 1e-12 and abs(pi[4].sum() - 1.0) < 1e-12
    csr = _csr_of(pi)
    assert int(csr[0][8] - csr[0][7]) == 0
    pi32 = torch.as_tensor(pi).float().cuda()
    torch.backends.cuda.matmul.allow_tf32 = False
    tr = TR.Trainer(sd0, H, NB, lr=2e-3, weight_decay=1e-4, max_batch=B, vloss_weight=1.5, dropout=0.0, amp=amp,
                    init_scale=1024.0)
    tr.backward(S, None, vv, policies=csr)
    ce, se, _ = tr.losses()
    _, l_f32, g_f32, _ = _torch_train_steps(sd0, H, NB, X, pi32, vv, B, 1, False)
    if amp:
        scale = tr.amp_state()["scale"]
        g = {n: v.numpy() / scale for n, v in tr.gradients().items()}
        _, l_amp, g_amp, _ = _torch_train_steps(sd0, H, NB, X, pi32, vv, B, 1, True, init_scale=1024.0)
        assert scale == 1024.0 and all(np.isfinite(x).all() for x in g_amp.values())
        for j, ours in enumerate((ce / B, se / B)):
            gap = abs(l_f32[0][j] - l_amp[0][j])
            print(f"loss[{j}]: ours {ours:.7f} torch-amp {l_amp[0][j]:.7f} torch-f32 {l_f32[0][j]:.7f}")
            assert abs(ours - l_amp[0][j]) <= 1.5 * gap + 1e-4 * abs(l_amp[0][j]) + 1e-7, j
        for name in g_amp:
            d_ours, d_f32 = _relnorm(g[name], g_amp[name]), _relnorm(g_f32[name], g_amp[name])
            assert d_ours <= 1.5 * d_f32 + 2e-3, ("grad", name, d_ours, d_f32)
    else:
        g = {n: v.numpy() for n, v in tr.gradients().items()}
        print(f"ce {ce / B:.7f} torch {l_f32[0][0]:.7f}; mse {se / B:.7f} torch {l_f32[0][1]:.7f}")
        assert abs(ce / B - l_f32[0][0]) <= 1e-5 * abs(l_f32[0][0]) + 1e-6
        assert abs(se / B - l_f32[0][1]) <= 1e-5 * abs(l_f32[0][1]) + 1e-6
        for name in g_f32:  # (unclipped on both sides: backward() alone, torch's before the clip)
            assert _relnorm(g[name], g_f32[name]) < 1e-4, "grad " + name
    # the empty row alone: CE exactly 0, no policy gradient at all
    tr.backward(S, None, vv, idx=torch.tensor([7], dtype=torch.int32, device="cuda"), policies=csr)
    assert tr.losses()[0] == 0.0
    g = tr.gradients()
    assert not g["pi_head.2.bias"].numpy().any() and not g["pi_head.2.weight"].numpy().any()
    assert g["v_head.4.weight"].numpy().any()


def test_soft_entry_points_check_their_arguments(T, golden, visit_targets):
    """NULL arrays and a batch outside 1 .. max_batch: YK_ERR_ARG (-1), nothing launched."""
    K, N, TR = T
    import yacht_amd
    lib = yacht_amd.lib()
    B = 8
    S, _, vv, _ = _data(K, golden, B, 8)
    ip, co, va = _csr_of(visit_targets[:B])
    tr = TR.Trainer(_sd(64, 1), 64, 1, max_batch=B, dropout=0.0)
    good = [tr.handle, S.data_ptr(), ip.data_ptr(), co.data_ptr(), va.data_ptr(), vv.data_ptr(), None, B, None]
    for f in (lib.yk_trainer_backward_soft, lib.yk_trainer_step_soft):
        for k in range(6):
            assert f(*[None if i == k else a for i, a in enumerate(good)]) == -1, k
        for b in (0, -1, B + 1):
            assert f(*good[:7], b, None) == -1, b
    assert tr.step_count == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. gather
@pytest.mark.parametrize("amp", [False, True])
def test_batch_idx_gathers_the_csr_rows(T, golden, visit_targets, amp):
    """step_soft with idx = perm on the full CSR == step_soft without idx on states, values and CSR
    physically reordered by perm (a repeated index included), bit for bit."""
    K, N, TR = T
    H, NB, B, n = 64, 1, 32, 96
    S, _, vv, rng = _data(K, golden, n, 14)
    pi = visit_targets[:n]
    perm = rng.permutation(n)[:B]
    perm[5] = perm[2]
    perm[B - 1] = 1  # the full row
    pt = torch.tensor(perm, dtype=torch.int32, device="cuda")
    kw = dict(max_batch=B, dropout=0.2, seed=3, amp=amp)
    a, b = TR.Trainer(_sd(H, NB), H, NB, **kw), TR.Trainer(_sd(H, NB), H, NB, **kw)
    a.step(S, None, vv, idx=pt, policies=_csr_of(pi))
    b.step(S[pt.long()].contiguous(), None, vv[pt.long()].contiguous(), policies=_csr_of(pi[perm]))
    assert a.losses().tobytes() == b.losses().tobytes()
    assert _bits(a) == _bits(b)


# ---------------------------------------------------------------- 6. fused step == backward + apply
@pytest.mark.parametrize("scale", [None, 2.0 ** 40])
def test_soft_amp_fused_norm_step_equals_backward_then_apply(T, golden, visit_targets, scale):
    """test_gpu_train.py::test_amp_fused_norm_step_equals_backward_then_apply's comparison with
    soft targets at (64, 1, 32): the same losses and GradScaler state, the grad sq-norm to 1e-12,
    the parameters to rtol 1e-6, over 3 steps; an overflowing step (scale 2^40) skipped alike."""
    K, N, TR = T
    H, NB, B = 64, 1, 32
    S, _, vv, _ = _data(K, golden, 3 * B, 9)
    csr = _csr_of(visit_targets[:3 * B])
    kw = dict(max_batch=B, dropout=0.1, amp=True)
    if scale:
        kw["init_scale"] = scale
    fused = TR.Trainer(_sd(H, NB), H, NB, **kw)
    split = TR.Trainer(_sd(H, NB), H, NB, **kw)
    for k in range(3):
        idx = torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device="cuda")
        fused.step(S, None, vv, idx=idx, policies=csr)
        split.backward(S, None, vv, idx=idx, policies=csr)
        split.apply()
        lf, ls = fused.losses(), split.losses()
        assert lf[0] == ls[0] and lf[1] == ls[1], k
        if np.isfinite(ls[2]):
            assert abs(lf[2] - ls[2]) <= 1e-12 * ls[2], (k, lf[2], ls[2])
        else:
            assert not np.isfinite(lf[2]), k
        assert fused.amp_state() == split.amp_state(), k
        np.testing.assert_allclose(fused.params().cpu().numpy(), split.params().cpu().numpy(), rtol=1e-6, atol=1e-9)
    if scale:
        assert fused.amp_state()["steps"] < 3


# ---------------------------------------------------------------- 7. through the public classes
@pytest.fixture(scope="module")
def selfplay_shards(T):
    """A 16-game, 8-simulation self-play at tempThreshold 0 (every policy one-hot) and 48 (every
    policy the visit distribution), as ExampleShards."""
    from yacht_amd import replay as R
    from yacht_amd.engine import SelfPlayEngine
    K, N, TR = T
    net = N.YkNet(spec.closed_form_weights(256, 6), 256, 6)
    out = {}
    for temp in (0, 48):
        eng = SelfPlayEngine(16, 8, 1.5, temp, net=net, max_moves=48)
        eng.run(23, 100)
        assert eng.stats()["errors"] == 0
        out[temp] = R.examples_from_images(eng.pack_records(), 16, 48, 8)
        eng.close()
    return out


def _wrapper(N, sd, amp, target=None):
    from yacht_amd.utils import dotdict
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=64, vloss_weight=1.5, cuda=True, hidden=64,
                   nblocks=1, dropout=0.0, amp=amp, seed=6)
    if target is not None:
        args["policy_target"] = target
    game = type("Game", (), {"getActionSize": lambda self: A})()
    w = N.NNetWrapper(game, args)
    w.nnet.load_state_dict(sd)
    return w


def _trained(N, sd, amp, target, examples):
    w = _wrapper(N, sd, amp, target)
    w.train(examples, verbose=False)
    return b"".join(v.numpy().tobytes() for v in w.nnet.state_dict().values())


@pytest.mark.parametrize("amp", [False, True])
def test_nnetwrapper_policy_target(T, selfplay_shards, amp):
    K, N, TR = T
    from yacht_amd import replay as R
    sd = _model_weights(N, 64, 1, 2)
    # (a) one-hot policies: "visits" is "argmax", bit for bit (and absent is "argmax")
    hot = selfplay_shards[0]
    assert len(hot) == 16 * 48 and int(hot.policies["pi_indptr"][-1]) == len(hot)
    base = _trained(N, sd, amp, "argmax", hot)
    assert _trained(N, sd, amp, None, hot) == base
    assert _trained(N, sd, amp, "visits", hot) == base
    # (b) visit policies: "visits" differs from "argmax", and is the hand-written soft loop
    vis = selfplay_shards[48]
    assert int(vis.policies["pi_indptr"][-1]) > len(vis)
    soft = _trained(N, sd, amp, "visits", vis)
    assert soft != _trained(N, sd, amp, "argmax", vis)
    tr = TR.Trainer(sd, 64, 1, lr=2e-3, weight_decay=1e-4, max_batch=64, vloss_weight=1.5, dropout=0.0, seed=6, amp=amp)
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    perm = torch.randperm(len(vis), generator=g, device="cuda").to(torch.int32)
    pol = R.as_device_policies(vis)
    for i in range(0, len(vis), 64):
        tr.step(vis.states, None, vis.values, idx=perm[i:i + 64], policies=pol)
    assert b"".join(v.numpy().tobytes() for v in tr.state_dict().values()) == soft
    # (c) the tuple form (dense float64 pi) trains to the same bits as the shard
    tuples = list(vis)
    assert isinstance(tuples[0], tuple) and len(tuples[0][1]) == A
    for x, y in zip(R.as_device_policies(tuples), pol):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert _trained(N, sd, amp, "visits", tuples) == soft
    # a history of both forms: the device concatenation is the host's
    hist = [tuples[:300], [], vis]
    for x, y in zip(R.as_device_policies(hist), R.policies_csr_host(hist)):
        assert np.array_equal(x.cpu().numpy(), y) and x.cpu().numpy().dtype == y.dtype
    assert R.as_device_examples(hist)[0].shape[0] == 300 + len(vis) == R.as_device_policies(hist)[0].numel() - 1
