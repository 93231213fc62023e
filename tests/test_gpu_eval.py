"""Held-out evaluation on the GPU: k_eval_rows against the float64 restatement
tests/eval_ref.py on synthetic logits, the column sums bit for bit; yk_net_logits against yk_net_predict;
yk_net_evaluate against the two of them, whatever the chunk; the hard cross-entropy against the reference's
own predict (tests/golden); NNetWrapper.evaluate over every form of examples; Coach's held-out set; the
command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref as R
from conftest import GOLDEN, PKG
from oracle import oracle as O
from oracle import spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, LD = 3226, 3264


@pytest.fixture(scope="module")
def Y():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import yacht_amd
    from yacht_amd import engine, kernels, nnet, replay
    return yacht_amd, engine, kernels, nnet, replay


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _metrics(Ymod, logits, ld, v, states, targets, values, csr, idx, n, rows=True):
    """yk_examples_metrics on device tensors -> (rows f64[n, 16] or None, sums f64[16])."""
    out = torch.full((max(n, 1), 16), 7.0, dtype=torch.float64, device="cuda") if rows else None
    sums = (C.c_double * 16)()
    p = [t.data_ptr() for t in csr] if csr is not None else [None] * 3
    rc = Ymod.lib().yk_examples_metrics(logits.data_ptr(), ld, v.data_ptr(), states.data_ptr(), targets.data_ptr(),
                                        values.data_ptr(), *p, idx.data_ptr() if idx is not None else None, n,
                                        out.data_ptr() if rows else None, sums, None)
    assert rc == 0
    return (out.cpu().numpy()[:n] if rows else None), np.array(list(sums))


# ------------------------------------------------------------------ 1. the kernel against float64
@pytest.fixture(scope="module")
def boards():
    """300 boards of tests/golden/states.npz and their valid masks for player 1 (the oracle's)."""
    W = np.load(os.path.join(GOLDEN, "states.npz"))["states"][:300]
    phase = (W[:, 0] >> np.uint64(4)) & np.uint64(1)
    carry = (W[:, 1] >> np.uint64(40)) & np.uint64(0xF)  # player 1's carry length
    used = (W[:, 1] >> np.uint64(44)) & np.uint64(0xFFF)
    assert (phase == 0).any() and (phase == 1).any()
    assert ((phase == 1) & (carry == 5)).any() and ((phase == 1) & (carry == 10)).any()
    assert ((phase == 1) & (carry >= 5) & (used == 0)).any()  # all 12 categories open
    return W, O.valid(W, 1)[0].astype(bool)


_CASES = {}


def _synthetic(n, boards):
    """n examples (boards spread over the 300), their special rows by i % 8, and the restatement's rows
    without and with a batch_idx - computed once per n."""
    if n in _CASES:
        return _CASES[n]
    W, ok = boards
    rng = np.random.default_rng(1000 + n)
    pick = np.arange(n) * 37 % 300
    x = rng.normal(scale=3.0, size=(n, A)).astype(np.float32)
    targets = rng.integers(0, A, size=n).astype(np.int32)
    values = rng.choice(np.array([-1.0, 0.0, 1.0], dtype=np.float32), size=n)
    v = np.tanh(rng.normal(size=n)).astype(np.float32)
    lens = rng.integers(1, 90, size=n)  # (more than 64 entries: a second chunk of the CSR row)
    for i in range(n):
        k = i % 8
        if k == 0:
            targets[i] = 0
        elif k == 1:
            targets[i], lens[i] = A - 1, 0  # an empty CSR row
        elif k == 2:
            targets[i] = -1
        elif k == 3:
            targets[i] = A
        elif k in (4, 7):  # a tie at the maximum, the target at the lower / the higher index
            x[i, [70, 3000]] = x[i].max() + 1.0
            targets[i] = 70 if k == 4 else 3000
        elif k == 5:  # f32 exp would flush most of this row to zero
            x[i] = np.linspace(-80.0, 80.0, A, dtype=np.float32)[rng.permutation(A)]
        elif k == 6:
            x[i] = np.float32(-1.25)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(A, size=l, replace=False)) for l in lens] + [[]]).astype(np.int32)
    vals = rng.random(len(cols))
    for i in range(n):
        a0, a1 = indptr[i], indptr[i + 1]
        if a1 > a0:
            vals[a0:a1] /= vals[a0:a1].sum()
            if i % 8 == 0:
                cols[a1 - 1] = A - 1  # an entry at the last column ...
                vals[a0:a1] *= 0.7    # ... and S != 1
    if n > 2:
        vals[indptr[2]] = 0.0  # a stored zero: no log(0) in the target entropy
    idx = rng.permutation(n).astype(np.int32)
    idx[-1] = idx[0]  # a permutation with a repeat
    case = dict(x=x, v=v, states=W[pick], ok=ok[pick], targets=targets, values=values, csr=(indptr, cols, vals),
                idx=idx)
    case["want"] = {False: R.rows(x, v, case["ok"], targets, values, case["csr"]),
                    True: R.rows(x[idx], v[idx], case["ok"], targets, values, case["csr"], batch_idx=idx)}
    _CASES[n] = case
    return case


@pytest.mark.parametrize("ld", [LD, A])
@pytest.mark.parametrize("use_idx", [False, True])
@pytest.mark.parametrize("n", [1, 4, 5, 17, 300])
def test_rows_kernel_against_float64(Y, boards, n, use_idx, ld):
    """n = 1, 4, 5: a partial block, a full one, one row past it; 17; 300: more than the 256 partials.
    Every padding column holds 1e30: a kernel that reads one cannot pass.

    Tolerance of columns 0, 1, 3-7 (derived, not measured): a sum of at most 3226 float64 terms in any order
    is within 3226 * 2^-53 = 3.6e-13 of exact relative to sum|terms| - at most max|x| for the entropy's
    mixed-sign sum - and the device's exp / log are within a few ulp of numpy's; rtol 1e-11 and atol
    1e-11 (1 + max|x|) leave a factor of about 30 over that for both."""
    c = _synthetic(n, boards)
    x, v = (c["x"][c["idx"]], c["v"][c["idx"]]) if use_idx else (c["x"], c["v"])
    lg = np.full((n, ld), 1e30, dtype=np.float32)
    lg[:, :A] = x
    args = (Y[0], _dev(lg), ld, _dev(v), _dev(c["states"].view(np.int64)), _dev(c["targets"]), _dev(c["values"]),
            tuple(_dev(a) for a in c["csr"]), _dev(c["idx"]) if use_idx else None, n)
    got, sums = _metrics(*args)
    want = c["want"][use_idx]
    exact = [2, 11, 12, 13, 14, 15]
    assert np.array_equal(got[:, exact], want[:, exact])
    assert np.array_equal(got[:, 8:11].view(np.uint64), want[:, 8:11].view(np.uint64))  # the same IEEE operations
    atol = 1e-11 * (1.0 + np.abs(x).max(1))
    for col in (0, 1, 3, 4, 5, 6, 7):
        err = np.abs(got[:, col] - want[:, col])
        tol = 1e-11 * np.abs(want[:, col]) + atol
        print(f"n {n} idx {use_idx} ld {ld} col {col}: max err / tol {float((err / tol).max()):.3g}")
        assert (err <= tol).all(), (col, int(np.argmax(err / tol)))
    assert np.array_equal(sums.view(np.uint64), R.sums(got).view(np.uint64))
    again, sums2 = _metrics(*args)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64)) and np.array_equal(sums2.view(np.uint64), sums.view(np.uint64))
    assert np.array_equal(_metrics(*args, rows=False)[1].view(np.uint64), sums.view(np.uint64))  # rows == NULL
    if not use_idx and ld == LD:  # without a CSR: columns 5-7 are zero, the others unchanged
        a = list(args)
        a[7] = None
        bare, _ = _metrics(*a)
        assert not bare[:, 5:8].any()
        keep = [0, 1, 2, 3, 4] + list(range(8, 16))
        assert np.array_equal(bare[:, keep].view(np.uint64), got[:, keep].view(np.uint64))


# ------------------------------------------------------------------ 2. yk_net_logits
def _net_states(hidden, nblocks):
    """The fixture's 32 states and 16 more boards: 48 rows, three 16-row tiles of the forward."""
    g = np.load(os.path.join(GOLDEN, f"predict_h{hidden}_b{nblocks}.npz"))
    more = np.load(os.path.join(GOLDEN, "states.npz"))["states"][1000:1016]
    return g, np.concatenate([g["states"], more])


@pytest.mark.parametrize("hidden,nblocks,precision", [(64, 1, "f32"), (256, 6, "f32"), (64, 1, "f16")])
def test_logits_are_the_predicts(Y, hidden, nblocks, precision):
    """softmax in float64 of the raw logits == yk_net_predict's pi at the tolerance the project holds predict
    to (rtol 1e-5 / atol 1e-7): they differ only by predict's own f32 x - m - l and expf.  v is the same
    forward's: bit-equal."""
    _, _, K, N, _ = Y
    _, W = _net_states(hidden, nblocks)
    net = N.YkNet(spec.closed_form_weights(hidden, nblocks), hidden, nblocks, precision=precision)
    S = K.states_to_device(W)
    lg, v = net.logits(S)
    pi, pv = net.predict_states(S)
    assert lg.shape == (48, LD) and lg.dtype == torch.float32
    x = lg.cpu().numpy()[:, :A].astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    np.testing.assert_allclose(e / e.sum(1, keepdims=True), pi.cpu().numpy(), rtol=1e-5, atol=1e-7)
    assert torch.equal(v, pv)
    assert net.errors() == 0


# ------------------------------------------------------------------ 3. yk_net_evaluate
@pytest.mark.parametrize("use_csr", [False, True])
@pytest.mark.parametrize("use_idx", [False, True])
def test_evaluate_is_forward_plus_metrics_whatever_the_chunk(Y, use_idx, use_csr):
    Ymod, _, K, N, _ = Y
    n = 50
    rng = np.random.default_rng(77)
    W = np.load(os.path.join(GOLDEN, "states.npz"))["states"][2000:2000 + n]
    net = N.YkNet(spec.closed_form_weights(64, 1), 64, 1)
    S = K.states_to_device(W)
    targets = _dev(rng.integers(-1, A + 1, size=n).astype(np.int32))
    values = _dev(rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=n))
    lens = rng.integers(0, 70, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(A, size=l, replace=False)) for l in lens]).astype(np.int32)
    csr = (_dev(indptr), _dev(cols), _dev(rng.random(len(cols)))) if use_csr else None
    idx = rng.permutation(n).astype(np.int32)
    idx[-1] = idx[0]
    idx = _dev(idx) if use_idx else None
    lg, v = net.logits(S[idx.long()] if use_idx else S)
    rows, sums = _metrics(Ymod, lg, LD, v, S, targets, values, csr, idx, n)
    assert np.isfinite(rows).all()
    for chunk in (16, 48, 0):
        out = net.evaluate(S, targets, values, policies=csr, idx=idx, chunk=chunk, per_row=True)
        assert np.array_equal(out["rows"].cpu().numpy().view(np.uint64), rows.view(np.uint64)), chunk
        want = N.eval_summary(sums, soft=use_csr)
        got = {k: x for k, x in out.items() if k != "rows"}
        assert got.keys() == want.keys()
        for k in want:  # (bit-equal sums: equal numbers; NaN cannot occur, the rows are finite)
            assert got[k] == want[k], (chunk, k)
    assert out["n"] == n and (out["policy_ce_soft"] is None) == (not use_csr)
    assert out["bad_targets"] == int(((targets < 0) | (targets >= A)).sum())
    empty = net.evaluate(S[:0], targets[:0], values[:0])  # n == 0: NaN means, no exception
    assert empty["n"] == 0 and np.isnan(empty["policy_ce"]) and np.isnan(empty["value_mse"])


# ------------------------------------------------------------------ 4. the reference's own predict
@pytest.mark.parametrize("hidden,nblocks", [(64, 1), (256, 6)])
def test_cross_entropy_against_the_references_predict(Y, hidden, nblocks):
    """tests/test_gpu_net.py holds pi to rtol 1e-5 / atol 1e-7 and v to 1e-5 of the fixture; through log, to
    first order, -log(pi[t]) is then within 1e-5 + 1e-7 / pi_ref[t] of the reference's."""
    _, _, K, N, _ = Y
    g, _ = _net_states(hidden, nblocks)
    net = N.YkNet(spec.closed_form_weights(hidden, nblocks), hidden, nblocks)
    t = g["pi"].argmax(1).astype(np.int32)
    S = K.states_to_device(g["states"])
    out = net.evaluate(S, _dev(t), _dev(np.zeros(len(t), np.float32)), per_row=True)
    rows = out["rows"].cpu().numpy()
    p = g["pi"][np.arange(len(t)), t].astype(np.float64)
    err = np.abs(rows[:, 1] - -np.log(p))
    print(f"h{hidden} b{nblocks}: max CE err / bound {float((err / (1e-5 + 1e-7 / p)).max()):.3g}, "
          f"max |v - v_ref| {float(np.abs(rows[:, 8] - g['v']).max()):.3g}")
    assert (err <= 1e-5 + 1e-7 / p).all()
    assert (np.abs(rows[:, 8] - g["v"].astype(np.float64)) <= 1e-5).all()


# ------------------------------------------------------------------ 5. the Python surface
ARGS = dict(numIters=2, numEps=6, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
            arenaCompare=6, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=2,
            batch_size=40, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3,
            amp=False)  # tests/test_gpu_coach.py's, the smallest Coach configuration of the suite; two iterations


def _wrapper(**extra):
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    torch.manual_seed(5)
    return NNetWrapper(YachtGame(seed=21, env_id=500), dotdict(ARGS, **extra))


def _halves(R_, sh, k):
    P = sh.policies
    ip = P["pi_indptr"]
    a = int(ip[k])

    def part(lo, hi, e0, e1):
        pol = dict(pi_indptr=ip[lo:hi + 1], pi_cols=P["pi_cols"][e0:e1], pi_vals=P["pi_vals"][e0:e1],
                   values64=P["values64"][lo:hi])
        return R_.ExampleShard(sh.states[lo:hi], sh.targets[lo:hi], sh.values[lo:hi], policies=pol,
                               outcomes=sh.outcomes[lo:hi])
    return [part(0, k, 0, a), part(k, len(sh), a, int(ip[-1]))]


@pytest.fixture(scope="module")
def shards(Y):
    """5 hash-prior games x 8 sims with root values, as a plain shard and as one built with value_mix 0.5."""
    _, E, _, _, R_ = Y
    eng = E.SelfPlayEngine(5, 8, 1.5, 15, prior="hash", max_moves=48, record_root_values=True)
    eng.run(31, 0)
    assert eng.stats()["errors"] == 0
    img = eng.pack_records()
    eng.close()
    return R_.examples_from_images(img, 5, 48, 8), R_.examples_from_images(img, 5, 48, 8, value_mix=0.5)


def test_wrapper_evaluate_over_every_form_of_examples(Y, shards):
    _, _, _, _, R_ = Y
    plain, mixed = shards
    assert len(plain) == 240 and not torch.equal(mixed.values, mixed.outcomes)
    net = _wrapper()
    want = net.evaluate(plain)
    assert want["n"] == 240 and want["bad_targets"] == 0
    assert net.evaluate(mixed) == want  # the outcomes, not the shard's training values
    assert net.evaluate(_halves(R_, plain, 100)) == want
    assert net.evaluate([plain]) == want
    tuples = list(plain)
    assert net.evaluate(tuples) == want
    assert net.evaluate([tuples[:100], tuples[100:]]) == want
    vw = ARGS["vloss_weight"]
    assert want["loss"] == want["policy_ce"] + vw * want["value_mse"]
    soft = net.evaluate(plain, target="visits")
    assert soft["loss"] == soft["policy_ce_soft"] + vw * soft["value_mse"] != want["loss"]
    assert {k: x for k, x in soft.items() if k != "loss"} == {k: x for k, x in want.items() if k != "loss"}
    assert _wrapper(policy_target="visits").evaluate(plain) == soft  # the default follows args.policy_target
    assert want["policy_kl"] >= -1e-12 and 0.0 < want["valid_mass"] <= 1.0
    assert 0.0 <= want["top1"] <= want["top5"] <= 1.0 and want["value_mse"] >= 0.0
    assert abs(want["policy_kl"] - (want["policy_ce_soft"] - want["target_entropy"])) < 1e-12  # every S is 1
    # a shard without policies: the hard numbers, the soft ones None; "visits" needs them
    bare = R_.ExampleShard(plain.states, plain.targets, plain.values)
    hard = net.evaluate(bare)
    assert hard["policy_ce_soft"] is None and hard["policy_kl"] is None and hard["loss"] == want["loss"]
    with pytest.raises(ValueError, match="policies"):
        net.evaluate(bare, target="visits")


# ------------------------------------------------------------------ 6. Coach
def _learn(tmp_path, name, **extra):
    from yacht_amd.coach import Coach
    ck = str(tmp_path / name)
    net = _wrapper(checkpoint=ck, load_folder_file=(ck, "best.pth.tar"), **extra)
    coach = Coach(net.game, net, net.args)
    coach.learn()
    return coach


def test_coach_holds_games_out(Y, tmp_path):
    on = _learn(tmp_path, "on", holdoutEps=4)
    off = _learn(tmp_path, "off")
    assert [e["new"]["n"] for e in on.eval_history] == [4 * 48, 8 * 48]
    assert [e["prev"]["n"] for e in on.eval_history] == [4 * 48, 8 * 48]
    assert on.last_eval is on.eval_history[-1] and set(on.last_eval) == {"prev", "new"}
    assert all(np.isfinite(e[k]["loss"]) for e in on.eval_history for k in e)
    assert on.eval_history[0]["prev"] != on.eval_history[0]["new"]  # the net was trained in between

    def keys(shards_):
        return {bytes(r) for s in shards_ for r in s.states.cpu().numpy().view(np.uint8).reshape(-1, 64)}
    assert [len(s) for s in on.holdoutHistory] == [4 * 48, 4 * 48]
    assert not keys(on.holdoutHistory) & keys(on.trainExamplesHistory)
    assert [len(s) for s in on.trainExamplesHistory] == [len(s) for s in off.trainExamplesHistory] == [6 * 48] * 2
    assert set(on.phase_times) == {"selfplay_s", "save_s", "train_s", "eval_s", "arena_s", "gate_s", "iteration_s"}
    assert on.phase_times["eval_s"] > 0
    # off: nothing of it exists
    assert set(off.phase_times) == {"selfplay_s", "save_s", "train_s", "arena_s", "gate_s", "iteration_s"}
    assert off.eval_history == [] and off.last_eval is None and off.holdoutHistory == []
    per_iter = ARGS["numEps"] + 2 * int(ARGS["arenaCompare"] / 2)
    assert off._next_env == 500 + ARGS["numIters"] * per_iter
    assert on._next_env == 500 + ARGS["numIters"] * (per_iter + 4)
    # the first iteration's training games are the same games either way (the held-out ones come after them)
    assert torch.equal(on.trainExamplesHistory[0].states, off.trainExamplesHistory[0].states)


# ------------------------------------------------------------------ 7. the command line
def test_command_line_prints_the_wrappers_dict(Y, shards, tmp_path):
    from yacht_amd import examples_io as X
    plain, _ = shards
    net = _wrapper(policy_target="visits")
    net.save_checkpoint(folder=str(tmp_path), filename="net.pth.tar")
    tuples = list(plain)[:96]
    X.save_examples(str(tmp_path / "held.npz"), [tuples[:48], tuples[48:]])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in [os.environ.get("PYTHONPATH")] if p]))

    def run(*extra):
        r = subprocess.run([sys.executable, "-m", "yacht_amd.evaluate", "--model", str(tmp_path / "net.pth.tar"),
                            "--examples", str(tmp_path / "held.npz"), *extra], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])
    assert run() == net.evaluate(tuples)  # (the checkpoint's policy_target: visits)
    assert run("--target", "argmax") == net.evaluate(tuples, target="argmax")
