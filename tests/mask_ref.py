"""The legal-move mask restated in plain torch / numpy for its tests (test infrastructure,
CPU): batches of fixture states whose valid sets cover the shapes the masked kernels can get wrong, targets
that keep the mask's contract, one masked train step in a chosen dtype - float64 is the checker - and the
masked form of the held-out evaluation's rows.  Builds on tests/train_ref.py and tests/eval_ref.py.

The valid sets are the reference's own getValidMoves(state, 1), recorded in golden/states.npz.

Batch rows cycle through CATEGORIES: one valid action; 3024 valid actions (the most there can be); all valid
actions - more than one - inside one head part; exactly 2, 3, ..., 8 occupied head parts.  Head part p is the
columns 16 * (p * 202 // 8) .. 16 * ((p + 1) * 202 // 8) - 1 (eight runs of 25 or 26 sixteen-column tiles, as the
mixed-precision head kernel splits a row; the kernel's own cuts, over 204 tiles, lie at most 32 columns further
on, so a row of few occupied parts leaves most of the kernel's parts without a valid column either way).
Rows reach a trainer through a shuffled idx into a buffer three times as long, as in the edge tests; every
buffer row keeps the contract (a non-empty valid set, a valid target, a policy on valid columns)."""
import os

import numpy as np
import torch

import train_ref as R

A = R.A
NCAT = 10
PART_EDGES = [16 * (p * 202 // 8) for p in range(9)]
CATEGORIES = ["one valid action", "3024 valid actions", "one head part, several actions"] + \
             [f"{k} occupied head parts" for k in range(2, 9)]
_FIX = {}
_CASES = {}


def fixture():
    """states uint64[N, 8], feat f32[N, 59], valid bool[N, 3226] (player 1), cat int[N] (-1: no valid action)."""
    if not _FIX:
        g = np.load(os.path.join(R.GOLDEN, "states.npz"))
        valid = np.unpackbits(g["valid"], axis=-1, bitorder="little")[..., :A][:, 0].astype(bool)
        cnt = valid.sum(1)
        occ = np.stack([valid[:, PART_EDGES[p]:PART_EDGES[p + 1]].any(1) for p in range(8)], 1).sum(1)
        cat = np.full(len(valid), -2)
        cat[cnt == 0] = -1
        cat[cnt == 1] = 0
        cat[cnt == 3024] = 1
        cat[(occ == 1) & (cnt > 1)] = 2
        for k in range(2, 9):
            cat[(occ == k) & (cnt != 3024)] = 1 + k
        assert (cat != -2).all() and all((cat == c).any() for c in range(-1, NCAT))
        _FIX.update(states=g["states"], feat=g["feat"], valid=valid, cat=cat)
        for a in _FIX.values():
            a.setflags(write=False)
    return _FIX


def mask_case(H, NB, B, seed, soft_nnz=(1, 2, 25, 100)):
    """One case's inputs, computed once per (H, NB, B, seed) and left unchanged:
    sd float32 weights; states uint64[3B, 8], feat f32[3B, 59], valid bool[3B, 3226]; idx int32[B] shuffled
    (batch row j, of category j % 10, is buffer row idx[j]); targets int32[3B], a valid action each (batch row 0
    its first, row 1 its last); values f32[3B]; pi float64[3B, 3226], visit policies over min(|L|, one of
    {1, 2, 25, 100}) valid columns."""
    key = (H, NB, B, seed)
    if key in _CASES:
        return _CASES[key]
    F = fixture()
    rng = np.random.RandomState(seed)
    n = 3 * B
    idx = rng.permutation(n)[:B].astype(np.int32)
    if B > 1 and np.array_equal(idx, np.arange(B)):
        idx = idx[::-1].copy()
    rows = rng.choice(np.flatnonzero(F["cat"] >= 0), n)  # (never a state without a valid action)
    for j in range(B):
        rows[idx[j]] = rng.choice(np.flatnonzero(F["cat"] == j % NCAT))
    valid = F["valid"][rows]
    targets = np.zeros(n, dtype=np.int32)
    pi = np.zeros((n, A), dtype=np.float64)
    for i in range(n):
        L = np.flatnonzero(valid[i])
        targets[i] = rng.choice(L)
        cols = rng.choice(L, min(len(L), int(rng.choice(soft_nnz))), replace=False)
        counts = rng.randint(1, 20, len(cols)).astype(np.float64)
        pi[i, cols] = counts / counts.sum()
    targets[idx[0]] = np.flatnonzero(valid[idx[0]])[0]
    if B > 1:
        targets[idx[1]] = np.flatnonzero(valid[idx[1]])[-1]
    values = (rng.rand(n) * 1.98 - 0.99).astype(np.float32)
    case = dict(sd=R.model_weights(H, NB, 2000 + seed), states=np.ascontiguousarray(F["states"][rows]),
                feat=np.ascontiguousarray(F["feat"][rows]), valid=valid, idx=idx, targets=targets, values=values,
                pi=pi, cats=F["cat"][rows])
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CASES[key] = case
    return case


def case_seed(H, NB, B):
    return 11 * H + 5 * NB + B


def batch_of(case, soft, H, NB, B, dropout, row0=R.ROW0, step=0):
    """(X rows, targets or dense pi, values, valid, masks or None) of the batch the trainer sees through idx."""
    from helpers import dropout_keep_np
    idx = case["idx"].astype(np.int64)
    tgt = case["pi"][idx] if soft else case["targets"][idx]
    masks = None
    if dropout > 0:
        masks = [dropout_keep_np(R.SEED_DROP, L, step, B, H, dropout, row_base=row0) for L in range(1 + NB)]
    return case["feat"][idx], tgt, case["values"][idx], case["valid"][idx], masks


def masked_loss(model, x, target, values, valid, vw=1.5):
    """(total, ce mean, mse mean) of the step's loss with the policy softmax over the valid actions only:
    masked_fill(~valid, -inf), then log_softmax; hard labels (an integer target) or a dense probability target,
    -(where(p > 0, p * lp, 0)).sum(1).mean() - F.cross_entropy's probability form evaluates 0 * -inf.  valid
    None: the unmasked loss in the same formulas.  Under autocast the masking sees the fp16 logits and
    log_softmax runs in float32, as F.cross_entropy does there."""
    out_pi, out_v = model(x)
    if valid is not None:
        out_pi = out_pi.masked_fill(~valid, float("-inf"))
    wide = torch.float64 if out_pi.dtype == torch.float64 else torch.float32
    lp = torch.log_softmax(out_pi, dim=1)  # (float32 under autocast)
    if target.is_floating_point():
        p = target.to(wide)
        ce = -(torch.where(p > 0, p * lp, torch.zeros_like(lp))).sum(1).mean()
    else:
        ce = -lp.gather(1, target.long().reshape(-1, 1)).mean()
    lv = torch.nn.functional.mse_loss(out_v, values.reshape(-1, 1).to(wide))
    return ce + vw * lv, ce, lv


def ref_step(sd, H, NB, X, targets_or_pi, values, valid, dtype, masks=None, p=0.0, vw=1.5, update=False):
    """train_ref.ref_step with the masked loss (valid None: unmasked): one CPU step in `dtype`."""
    model = R.make_model(sd, H, NB, dtype, masks, p)
    x = torch.tensor(np.asarray(X)).to(dtype)
    t = torch.tensor(np.asarray(targets_or_pi))
    v = torch.tensor(np.asarray(values)).to(dtype)
    ok = None if valid is None else torch.tensor(np.asarray(valid))
    loss, lp, lv = masked_loss(model, x, t, v, ok, vw)
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


def never_valid(case, idx=None):
    """The columns invalid in every batch row (idx: another choice of buffer rows than the case's batch).  The
    cases' whole batches have none: a 3024-action row and a bidding row already cover all 3226 columns."""
    idx = case["idx"] if idx is None else idx
    return np.flatnonzero(~case["valid"][np.asarray(idx, dtype=np.int64)].any(0))


def idx_narrow_rows(case):
    """The case's batch rows of one valid action, of one occupied head part and of two: a batch whose
    never-valid set is not empty (tests/test_mask_host.py asserts it)."""
    idx = case["idx"]
    return idx[np.isin(case["cats"][idx.astype(np.int64)], (0, 2, 3))].copy()


def eval_rows(logits, v, valid, targets, values, csr=None, batch_idx=None):
    """eval_ref.rows over x' (float64): -inf at the invalid actions; column 4 is the valid mass of x' (1), the
    rank counts valid actions only, the entropy skips the terms with e_a = 0."""
    logits = np.asarray(logits)
    n = logits.shape[0]
    out = np.zeros((n, 16), dtype=np.float64)
    for i in range(n):
        r = int(batch_idx[i]) if batch_idx is not None else i
        ok = np.asarray(valid[r], dtype=bool)
        x = np.asarray(logits[i, :A], dtype=np.float32).astype(np.float64)
        x[~ok] = -np.inf
        t = int(targets[r])
        t_in = 0 <= t < A
        m = x.max()
        e = np.exp(x - m)
        s = e.sum()
        lse = m + np.log(s)
        if t_in:
            rank = int(np.count_nonzero(ok & (x > x[t])) + np.count_nonzero(ok[:t] & (x[:t] == x[t])))
        else:
            rank = A
        S = soft = tent = 0.0
        if csr is not None:
            indptr, cols, vals = csr
            a0, a1 = int(indptr[r]), int(indptr[r + 1])
            c = np.asarray(cols[a0:a1], dtype=np.int64)
            p = np.asarray(vals[a0:a1], dtype=np.float64)
            S = p.sum()
            inside = (c >= 0) & (c < A)
            soft = (p[inside] * (lse - x[c[inside]])).sum()
            pos = p > 0
            tent = -(p[pos] * np.log(p[pos])).sum()
        vd, z = np.float64(np.float32(v[i])), np.float64(np.float32(values[r]))
        d = vd - z
        nz = e > 0
        out[i] = [lse, lse - x[t] if t_in else 0.0, rank, lse - (e[nz] * x[nz]).sum() / s, e[ok].sum() / s, S, soft,
                  tent, vd, d, d * d, 1.0 if vd * z > 0 else 0.0, 1.0 if rank == 0 else 0.0,
                  1.0 if rank < 5 else 0.0, 0.0 if t_in else 1.0, 1.0]
    return out


# ---- the cases of tests/test_gpu_legal_mask.py, shared with tests/test_mask_host.py, which proves on the CPU
# that their inputs cannot excuse a failure: (H, NB, max_batch, B, soft, dropout)
F32_CASES = [(64, 1, 256, 7, False, 0.0), (64, 1, 256, 63, False, 0.0), (64, 1, 256, 63, True, 0.0),
             (128, 2, 256, 129, False, 0.0), (64, 1, 256, 63, False, R.P_DROP)]
AMP_CASES = [(64, 1, 128, b, False, 0.0) for b in (7, 17, 63, 100)] + \
            [(128, 2, 128, 100, True, 0.0), (256, 6, 512, 100, False, 0.0)]
# (at (128, 2) the batch of 100 clips - its gradient norm is 5.7 - the one of 129, at 4.0, does not)
UPDATE_CASES = [(False, 64, 1, 256, 63), (False, 128, 2, 256, 100), (True, 64, 1, 128, 63), (True, 128, 2, 128, 100)]
EXACT_CASE = (64, 1, 128, 17)
