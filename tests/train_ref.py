"""A plain torch restatement of one training step (NNetWrapper.train's inner loop, NNet.py:141-165)
for the trainer tests: YachtNNet on the CPU in a chosen dtype - float64 is the checker, float32
the reference's own arithmetic - with hard labels or a dense probability target, optional fixed
dropout keep masks (helpers.dropout_keep_np restates the trainers' Philox bits), and the inputs
the edge tests share (test infrastructure)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

A = 3226
EDGE_COLS = [0, 31, 32, 3199, 3200, 3225]  # first / last action, a slice edge, the partial last slice
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _FixedDropout(torch.nn.Module):
    """nn.Dropout with given keep masks: x * keep * 1/(1-p), as torch's dropout kernel scales."""

    def __init__(self, p):
        super().__init__()
        self.scale, self.keep = 1.0 / (1.0 - p), None

    def forward(self, x):
        return x * (self.keep.to(x.dtype) * self.scale)


def relnorm(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_model(sd, H, NB, dtype, masks=None, p=0.0, device="cpu"):
    """YachtNNet of the weights sd in `dtype`, train mode; masks (one [rows, H] keep array per
    dropout layer, 0: inp, 1 + b: block b) take the nn.Dropout modules' places, else dropout is 0."""
    from yacht_amd.nnet import YachtNNet
    model = YachtNNet(hidden=H, nblocks=NB, dropout=0.0).to(dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()})
    model = model.to(device)
    if masks is not None:
        assert len(masks) == 1 + NB
        drops = [_FixedDropout(p) for _ in range(1 + NB)]
        for d, m in zip(drops, masks):
            d.keep = torch.as_tensor(np.asarray(m)).to(device)
        model.inp[3] = drops[0]
        for b, blk in enumerate(model.blocks):
            blk.dropout = drops[1 + b]
    return model.train()


def step_loss(model, x, target, values, vw=1.5):
    """(total, ce mean, mse mean) of NNet.py:141-149: target int -> hard labels, float -> a dense
    probability target (F.cross_entropy's probability form: -sum p log_softmax, mean over rows).
    Targets and values stay float32 under autocast (both losses run in float32 there)."""
    out_pi, out_v = model(x)
    wide = torch.float64 if out_pi.dtype == torch.float64 else torch.float32
    lp = F.cross_entropy(out_pi, target.to(wide) if target.is_floating_point() else target.long())
    lv = F.mse_loss(out_v, values.reshape(-1, 1).to(wide))
    return lp + vw * lv, lp, lv


def ref_step(sd, H, NB, X, targets_or_pi, values, dtype, masks=None, p=0.0, vw=1.5, update=False):
    """One step on the CPU in `dtype`.  Returns a dict: ce, mse (the batch means); grads (per tensor,
    float64 numpy, before the clip); sqnorm / gnorm (the total gradient's sum of squares and norm,
    summed in float64); and - update - params after clip_grad_norm_(5.0) + AdamW(2e-3, 1e-4)."""
    model = make_model(sd, H, NB, dtype, masks, p)
    x = torch.tensor(np.asarray(X)).to(dtype)
    t = torch.tensor(np.asarray(targets_or_pi))
    v = torch.tensor(np.asarray(values)).to(dtype)
    loss, lp, lv = step_loss(model, x, t, v, vw)
    loss.backward()
    grads = {n: q.grad.detach().double().numpy().copy() for n, q in model.named_parameters()}
    sq = float(sum((g ** 2).sum() for g in grads.values()))
    out = dict(ce=float(lp.detach()), mse=float(lv.detach()), grads=grads, sqnorm=sq, gnorm=sq ** 0.5)
    if update:
        opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=5.0)
        opt.step()
        out["params"] = {n: q.detach().double().numpy().copy() for n, q in model.named_parameters()}
    return out


def model_weights(H, NB, seed):
    """YachtNNet's own initialisation under torch.manual_seed(seed), the LayerNorm affines drawn
    non-trivially (as tests/test_gpu_train.py does): a float32 state dict."""
    from yacht_amd.nnet import YachtNNet
    gen = torch.random.get_rng_state()
    torch.manual_seed(seed)
    model = YachtNNet(hidden=H, nblocks=NB, dropout=0.0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    torch.random.set_rng_state(gen)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


_CASES = {}


def case_inputs(H, NB, B, seed):
    """The inputs of one edge case, computed once per (H, NB, B, seed) and left unchanged:
    sd       float32 weights (model_weights);
    states   uint64[3B, 8] cycled from golden/states.npz, feat float32[3B, 59] their features;
    idx      int32[B], a shuffled subset of the 3B buffer rows (never arange);
    targets  int32[3B] hard labels - the batch's first rows hold EDGE_COLS where B allows;
    values   float32[3B] in (-1, 1);
    pi       float64[3B, 3226] visit policies, counts / sum with nnz from {1, 2, 25, 100}; the batch's
             row 0 holds EDGE_COLS, row 1 every action, row 2 (B >= 3) nothing."""
    key = (H, NB, B, seed)
    if key in _CASES:
        return _CASES[key]
    g = np.load(os.path.join(GOLDEN, "states.npz"))
    rng = np.random.RandomState(seed)
    n = 3 * B
    start = int(rng.randint(0, len(g["states"])))
    rows = (start + np.arange(n)) % len(g["states"])
    idx = rng.permutation(n)[:B].astype(np.int32)
    if B > 1 and np.array_equal(idx, np.arange(B)):
        idx = idx[::-1].copy()
    targets = rng.randint(0, A, n).astype(np.int32)
    k = min(B, len(EDGE_COLS))
    targets[idx[:k]] = EDGE_COLS[:k]
    values = (rng.rand(n) * 1.98 - 0.99).astype(np.float32)
    pi = np.zeros((n, A), dtype=np.float64)
    for i in range(n):
        cols = rng.choice(A, int(rng.choice([1, 2, 25, 100])), replace=False)
        counts = rng.randint(1, 20, len(cols)).astype(np.float64)
        pi[i, cols] = counts / counts.sum()
    special = [np.unique(np.concatenate([EDGE_COLS, rng.choice(A, 19, replace=False)])), np.arange(A), np.arange(0)]
    for j, cols in enumerate(special[:B]):
        counts = rng.randint(1, 20, len(cols)).astype(np.float64)
        pi[idx[j]] = 0.0
        pi[idx[j], cols] = counts / max(counts.sum(), 1.0)
    case = dict(sd=model_weights(H, NB, 1000 + seed), states=np.ascontiguousarray(g["states"][rows]),
                feat=np.ascontiguousarray(g["feat"][rows]), idx=idx, targets=targets, values=values, pi=pi)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CASES[key] = case
    return case


def csr_of(pi):
    """dense float64 [n, 3226] -> the CSR of its nonzero entries (indptr int64, cols int32 ascending,
    vals float64), as numpy arrays."""
    r, c = np.nonzero(pi)
    indptr = np.zeros(len(pi) + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=len(pi)), out=indptr[1:])
    return indptr, c.astype(np.int32), pi[r, c].astype(np.float64)


# ---- the cases of tests/test_gpu_train_edges.py, shared with tests/test_train_ref_host.py, which
# proves on the CPU that their inputs cannot excuse a failure: (H, NB, max_batch, B, soft, dropout)
ROW0, P_DROP, SEED_DROP = 37, 0.3, 23
F32_CASES = (
    [(64, 1, 256, b, False, 0.0) for b in (1, 5, 63, 65)] + [(128, 2, 256, b, False, 0.0) for b in (129, 193)] +
    [(512, 1, 64, 63, False, 0.0), (512, 1, 961, 961, False, 0.0),
     (64, 1, 256, 63, True, 0.0), (128, 2, 256, 129, True, 0.0),
     (64, 1, 256, 63, False, P_DROP), (128, 2, 256, 129, False, P_DROP)])
AMP_CASES = (
    [(64, 1, 128, b, False, 0.0) for b in (1, 7, 9, 17, 33, 63, 100)] + [(128, 2, 128, b, False, 0.0) for b in (17, 100)] +
    [(512, 1, 64, 17, False, 0.0), (512, 1, 64, 63, False, 0.0), (256, 6, 512, 100, False, 0.0),
     (64, 1, 128, 128, False, 0.0), (64, 1, 128, 63, True, 0.0), (128, 2, 128, 100, True, 0.0),
     (64, 1, 128, 63, False, P_DROP)])
UPDATE_CASES = [(False, 64, 1, 256, 63), (False, 128, 2, 256, 129), (True, 64, 1, 128, 63), (True, 128, 2, 128, 100)]


def amp_scale(B):
    """GradScaler's init_scale of an AMP case: 1024 (the project's value at batch 32) from B = 32,
    64 below - the scaled gradients stay a factor 4 below fp16's largest number on both sides."""
    return 1024.0 if B >= 32 else 64.0


def case_seed(H, NB, B):
    return 7 * H + 3 * NB + B


def batch_of(case, soft, H, NB, B, dropout, row0=ROW0, step=0):
    """The batch the trainer sees through idx: (X rows, targets or dense pi, values, masks or None)."""
    from helpers import dropout_keep_np
    idx = case["idx"].astype(np.int64)
    tgt = case["pi"][idx] if soft else case["targets"][idx]
    masks = None
    if dropout > 0:
        masks = [dropout_keep_np(SEED_DROP, L, step, B, H, dropout, row_base=row0) for L in range(1 + NB)]
    return case["feat"][idx], tgt, case["values"][idx], masks
