"""The float64 training-step reference (tests/train_ref.py) and the inputs of
tests/test_gpu_train_edges.py, checked on the CPU so that neither can excuse a failure there:

* every float64 gradient tensor of every case is well away from zero (a relative norm against it
  means something), and the clip is active in the update cases;
* torch float32 on the CPU - the arithmetic the float32 trainer restates - stays well inside the
  bounds the GPU tests hold the trainer to: gradients 1e-5 (the GPU bound is 1e-4), one-step
  updates 7e-4 (the GPU floor is 1e-3), losses and the gradient sq-norm within the GPU bounds;
* ref_step itself: all-ones masks at p = 0 are the plain step bit for bit, and with a fixed mask
  the float64 gradient is the central finite difference of the float64 loss.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import train_ref as R  # noqa: E402

SHAPES = sorted({(c[0], c[1], c[3], c[4], c[5]) for c in R.F32_CASES + R.AMP_CASES})
UPDATES = sorted({(H, NB, B) for _, H, NB, _, B in R.UPDATE_CASES})
_REF = {}


def _steps(H, NB, B, soft, dropout, update=False):
    """(float64 step, float32 step) of a case, computed once."""
    key = (H, NB, B, soft, dropout, update)
    if key not in _REF:
        case = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))
        X, tgt, vv, masks = R.batch_of(case, soft, H, NB, B, dropout)
        _REF[key] = tuple(R.ref_step(case["sd"], H, NB, X, tgt, vv, dt, masks=masks, p=dropout, update=update)
                          for dt in (torch.float64, torch.float32))
    return _REF[key]


def test_case_inputs_are_what_the_cases_need():
    for H, NB, B, soft, dropout in SHAPES:
        case = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))
        idx = case["idx"]
        assert len(case["states"]) == 3 * B and len(np.unique(idx)) == B and idx.max() < 3 * B
        assert B == 1 or not np.array_equal(idx, np.arange(B))
        k = min(B, len(R.EDGE_COLS))
        assert list(case["targets"][idx[:k]]) == R.EDGE_COLS[:k]
        assert np.abs(case["values"]).max() < 1.0
        pi = case["pi"][idx]
        nnz = (pi > 0).sum(1)
        assert all(pi[0, c] > 0 for c in R.EDGE_COLS)
        if B >= 3:
            assert nnz[1] == R.A and nnz[2] == 0
        full = nnz > 0
        assert np.abs(pi[full].sum(1) - 1.0).max() < 1e-12
        if B >= 63:
            assert {int(x) for x in np.unique(nnz)} >= {0, 1, 2, 25, 100, R.A}
        if dropout:
            masks = R.batch_of(case, soft, H, NB, B, dropout)[3]
            assert len(masks) == 1 + NB and all(m.shape == (B, H) and 0.6 < m.mean() < 0.8 for m in masks)
            other = R.batch_of(case, soft, H, NB, B, dropout, row0=0)[3]
            assert not np.array_equal(masks[0], other[0])  # the row offset selects other masks


@pytest.mark.parametrize("H,NB,B,soft,dropout", SHAPES)
def test_float64_gradients_are_nonzero_and_float32_is_close(H, NB, B, soft, dropout):
    r64, r32 = _steps(H, NB, B, soft, dropout)
    small = min((np.linalg.norm(g), n) for n, g in r64["grads"].items())
    worst = max((R.relnorm(r32["grads"][n], g), n) for n, g in r64["grads"].items())
    print(f"smallest float64 tensor norm {small[0]:.3e} ({small[1]}); float32 worst rel {worst[0]:.3e} ({worst[1]}); "
          f"grad norm {r64['gnorm']:.3f}")
    assert small[0] > 1e-4, small
    assert worst[0] <= 1e-5, worst
    for k in ("ce", "mse"):
        assert abs(r32[k] - r64[k]) <= 0.5 * (1e-5 * abs(r64[k]) + 1e-6), k
    assert abs(r32["sqnorm"] - r64["sqnorm"]) <= 2.1e-5 * r64["sqnorm"]


def test_amp_loss_scales_keep_fp16_gradients_finite():
    """The float64 gradients times the case's loss scale stay below 2^13: the GPU test asserts 2^14
    of torch's scaled fp16-path gradients, itself a factor 4 below fp16's largest number."""
    for H, NB, _, B, soft, dropout in R.AMP_CASES + [(128, 2, 128, 100, False, 0.0)]:
        r64, _ = _steps(H, NB, B, soft, dropout)
        big = max(np.abs(g).max() for g in r64["grads"].values()) * R.amp_scale(B)
        assert big < 2.0 ** 13, (H, NB, B, big)


@pytest.mark.parametrize("H,NB,B", UPDATES)
def test_update_cases_clip_and_float32_update_is_close(H, NB, B):
    r64, r32 = _steps(H, NB, B, False, 0.0, update=True)
    assert r64["gnorm"] > 5.0, r64["gnorm"]
    sd = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))["sd"]
    worst = max((R.relnorm(r32["params"][n] - sd[n].numpy(), p - sd[n].numpy()), n) for n, p in r64["params"].items())
    print(f"grad norm {r64['gnorm']:.3f}; float32 worst update rel {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= 7e-4, worst
    # the update is the step of the clipped gradient: no tensor stands still
    assert all(np.linalg.norm(p - sd[n].numpy()) > 0 for n, p in r64["params"].items())


def test_all_ones_masks_at_p0_are_the_plain_step():
    H, NB, B = 64, 1, 63
    case = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))
    X, tgt, vv, _ = R.batch_of(case, False, H, NB, B, 0.0)
    ones = [np.ones((B, H), dtype=bool) for _ in range(1 + NB)]
    for dt in (torch.float64, torch.float32):
        a = R.ref_step(case["sd"], H, NB, X, tgt, vv, dt, update=True)
        b = R.ref_step(case["sd"], H, NB, X, tgt, vv, dt, masks=ones, p=0.0, update=True)
        assert a["ce"] == b["ce"] and a["mse"] == b["mse"] and a["sqnorm"] == b["sqnorm"]
        for n in a["grads"]:
            assert np.array_equal(a["grads"][n], b["grads"][n]) and np.array_equal(a["params"][n], b["params"][n]), n


@pytest.mark.parametrize("soft", [False, True])
def test_masked_gradient_is_the_finite_difference_of_the_loss(soft):
    """inp.0.weight sits below every dropout layer: its gradient is right only if the masks are
    applied, and scaled, in the backward as in the forward.  Central difference of the float64
    loss at the three entries of largest gradient in three different rows, to 1e-6 relative
    (h = 1e-5: truncation ~ h^2, rounding ~ 1e-16 |loss| / h, both below 1e-9 absolute)."""
    H, NB, B, p = 64, 1, 63, R.P_DROP
    case = R.case_inputs(H, NB, B, R.case_seed(H, NB, B))
    X, tgt, vv, masks = R.batch_of(case, soft, H, NB, B, p)
    g = R.ref_step(case["sd"], H, NB, X, tgt, vv, torch.float64, masks=masks, p=p)["grads"]["inp.0.weight"]
    model = R.make_model(case["sd"], H, NB, torch.float64, masks, p)
    x, t, v = torch.as_tensor(X).double(), torch.as_tensor(tgt), torch.as_tensor(vv).double()
    w = model.inp[0].weight
    rows = np.argsort(-np.abs(g).max(1))[:3]
    h = 1e-5
    for r in rows:
        c = int(np.argmax(np.abs(g[r])))
        vals = []
        with torch.no_grad():
            w0 = float(w[r, c])
            for s in (1.0, -1.0):
                w[r, c] = w0 + s * h
                vals.append(float(R.step_loss(model, x, t, v)[0]))
            w[r, c] = w0
        fd = (vals[0] - vals[1]) / (2 * h)
        print(f"inp.0.weight[{r}, {c}]: grad {g[r, c]:.9e} finite difference {fd:.9e}")
        assert abs(fd - g[r, c]) <= 1e-6 * abs(g[r, c]), (r, c, fd, g[r, c])
