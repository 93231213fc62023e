"""Weighted minibatch sampling on the GPU (yk_sample_weights / yk_sample_cdf / yk_sample_draw, K.sample_*,
NNetWrapper.train with args.trainSteps) against the restatement of
tests/sample_ref.py, which tests/test_sample_host.py holds to the oracle's Philox and to its own claims.

* the cumulative table, the drawn indices, the weights and K equal the restatement bit for bit - at the sizes
  around a chunk (256), a scan block (16 chunks) and an offsets tile (256 chunks), and at 2^21 and 2^21 + 1
  elements: a number of chunks that is a power of two (the search's first step), and one more;
* training with trainSteps = T takes exactly T steps and is a trainer stepped by hand with the restatement's
  indices, bit for bit - parameters, moments, GradScaler state - alone, on two ranks and inside the Coach.
"""
import os
import socket

import numpy as np
import pytest

import sample_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BIG = 8192 * 256  # 2^21: 8192 chunks, 32 offset tiles
SIZES = [1, 255, 256, 257, 513, 65537]


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from yacht_amd import kernels as K
    from yacht_amd import nnet
    from yacht_amd import replay
    return K, nnet, replay


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weight_sets(n, full=True):
    rng = np.random.RandomState(n % 1000 + 1)
    sets = {"ones": np.ones(n), "exp3": np.exp(3 * rng.randn(n))}
    if not full:
        return sets
    if n >= 3:
        z = np.exp(rng.randn(n))
        z[0] = z[n - 1] = 0.0
        if n >= 513:
            z[256:512] = 0.0  # a whole aligned chunk
        sets["zeros"] = z
    if n >= 2:
        a = np.full(n, 1e-300)
        a[0] = 1e300
        sets["absorbed"] = a
    sets["subnormal"] = 5e-324 * rng.randint(0 if n > 1 else 1, 50, n)
    if n > 1:
        sets["subnormal"][n // 2] = 5e-324
    return sets


_REF = {}


def _ref_cdf(n, name, full=True):
    """(w, the restatement's cdf, total), computed once per (n, set)."""
    if (n, name) not in _REF:
        w = _weight_sets(n, full)[name]
        _REF[n, name] = (w,) + R.cdf(w)
    return _REF[n, name]


# ---------------------------------------------------------------- 1. the cumulative table
@pytest.mark.parametrize("n", SIZES + [4096, 4097, BIG, BIG + 1])
def test_cdf_is_the_restatement_bit_for_bit(T, n):
    K = T[0]
    full = n < BIG
    for name in _weight_sets(n, full):
        w, want, total = _ref_cdf(n, name, full)
        got, gt = K.sample_cdf(_dev(w))
        again, at = K.sample_cdf(_dev(w))
        g = got.cpu().numpy()
        assert g.dtype == np.float64 and g.tobytes() == want.tobytes(), (n, name)
        assert np.float64(gt).tobytes() == np.float64(total).tobytes() and gt == g[-1], (n, name)
        assert torch.equal(got, again) and at == gt, (n, name)
        assert (np.diff(g) >= 0).all(), (n, name)


def test_cdf_refuses_weights_it_cannot_normalise(T):
    K = T[0]
    base = np.exp(np.random.RandomState(4).randn(513))
    for pos in (0, 255, 256, 512):
        for bad in (-1.0, -5e-324, np.nan, np.inf):
            w = base.copy()
            w[pos] = bad
            with pytest.raises(ValueError, match="weights"):
                K.sample_cdf(_dev(w))
    for n in (1, 513):
        with pytest.raises(ValueError, match="weights"):
            K.sample_cdf(_dev(np.zeros(n)))
    with pytest.raises(ValueError, match="weights"):
        K.sample_cdf(_dev(np.full(513, 1e308)))  # every weight finite, the total is not
    assert K.sample_cdf(_dev(base))[1] > 0  # and the call after a refusal is a good one
    with pytest.raises(ValueError):
        K.sample_cdf(_dev(base.astype(np.float32)))
    from yacht_amd._lib import YK_ERR_ARG, YkError
    with pytest.raises(YkError) as e:
        K.sample_cdf(_dev(np.zeros(0)))
    assert e.value.code == YK_ERR_ARG


# ---------------------------------------------------------------- 2. the draws
SEED = 0xFEDCBA9876543210  # (above 2^32: both key words are used)


@pytest.mark.parametrize("n", SIZES + [BIG, BIG + 1])
def test_draws_are_the_restatement_bit_for_bit(T, n):
    K = T[0]
    full = n < BIG
    runs = 0
    for name in _weight_sets(n, full):
        _, table, total = _ref_cdf(n, name, full)
        d = _dev(table)
        for m in (1, 63, 64, 65, 4097):
            for first in (0, 2**32 - 3):  # (the second: the carry into counter word 1)
                for key in (0, 0xFFFFFFFF):
                    if not full and (m, first == 0, key == 0) not in ((4097, True, True), (65, False, False)):
                        continue
                    got = K.sample_draw(d, SEED, key, first, m).cpu().numpy()
                    want = R.draw(table, SEED, key, first, m)
                    assert got.dtype == np.int32 and np.array_equal(got, want), (n, name, m, first, key)
                    runs += 1
        if n == 1:
            assert not K.sample_draw(d, 5, 6, 7, 100).any()  # one element: every draw is it
    assert runs == (2 * 2 if not full else 20 * len(_weight_sets(n)))


@pytest.mark.parametrize("m,first", [(65536, 0), (65537, 0), (65537, 2**32 - 3), (262145, 2**32 - 3), (1048576, 0),
                                     (1048577, 2**32 - 3), (1048576 + 70001, 2**32 - 70000)])
def test_many_draws_are_the_restatement_bit_for_bit(T, m, first):
    """k_sample_draw's paths by m: up to 65536 a thread takes one draw (at most 256 blocks); from 65537 up to
    four in one group, draw r + d * (the grid's threads), over 256 blocks up to 262,144 and ceil(m / 1024) blocks
    up to 1,048,576; from 1,048,577 the grid stays at 1024 blocks and a thread loops over further groups."""
    K = T[0]
    for name in ("exp3", "zeros"):
        _, table, _ = _ref_cdf(65537, name)
        got = K.sample_draw(_dev(table), SEED, 0xFFFFFFFF, first, m).cpu().numpy()
        want = R.draw(table, SEED, 0xFFFFFFFF, first, m)
        assert np.array_equal(got, want), (name, m, first)


def test_draw_ranges_out_and_no_draws(T):
    K = T[0]
    _, table, _ = _ref_cdf(65537, "exp3")
    d = _dev(table)
    whole = K.sample_draw(d, 11, 2, 2**32 - 100, 300)
    part = K.sample_draw(d, 11, 2, 2**32 - 100 + 37, 200)
    assert torch.equal(whole[37:237], part)  # a range of draws is that range of the longer call
    assert not torch.equal(whole, K.sample_draw(d, 11, 3, 2**32 - 100, 300))  # another key, other draws
    assert not torch.equal(whole, K.sample_draw(d, 12, 2, 2**32 - 100, 300))
    buf = torch.full((400,), -7, dtype=torch.int32, device="cuda")
    out = K.sample_draw(d, 11, 2, 2**32 - 100, 300, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, whole) and bool((buf[300:] == -7).all())
    none = K.sample_draw(d, 11, 2, 0, 0, out=buf)  # m = 0: a no-op
    assert none.numel() == 0 and torch.equal(buf[:300], whole) and K.sample_draw(d, 1, 2, 3, 0).numel() == 0
    with pytest.raises(ValueError):
        K.sample_draw(d, 11, 2, 0, 500, out=buf)
    from yacht_amd._lib import YK_ERR_ARG, YkError
    with pytest.raises(YkError) as e:
        K.sample_draw(d, 11, 2, 0, -1)
    assert e.value.code == YK_ERR_ARG


def test_a_draw_that_rounds_up_to_the_total(T):
    """A total of three subnormal steps: u * total rounds to the total for every u > 5/6 (found on the CPU:
    the assertion below), and those draws land on the first element that reaches the total - index 2, not the
    zero-weight elements behind it and not n."""
    K = T[0]
    w = np.array([5e-324, 0.0, 1e-323, 0.0, 0.0])
    table, total = R.cdf(w)
    t = R.uniforms(9, 1, 0, 4096) * total
    assert total == 1.5e-323 and (t == total).sum() > 400 and (t < total).sum() > 400
    got, gt = K.sample_cdf(_dev(w))
    assert got.cpu().numpy().tobytes() == table.tobytes() and gt == total
    idx = K.sample_draw(got, 9, 1, 0, 4096).cpu().numpy()
    assert np.array_equal(idx, R.draw(table, 9, 1, 0, 4096))
    assert set(idx[t == total].tolist()) == {2} and set(idx.tolist()) == {0, 2}


# ---------------------------------------------------------------- 3. the weights
def _table(n, ld, seed, plain=False):
    """A synthetic per-row table: columns 5-7 as a soft cross-entropy run would leave them, 1e30 in the padding
    and noise elsewhere; unless plain, rows without a policy (S = 0), with a negative KL and with NaN."""
    rng = np.random.RandomState(seed)
    rows = rng.randn(n, ld)
    rows[:, 16:] = 1e30
    rows[:, 5] = 1.0 + 1e-9 * rng.randn(n)
    rows[:, 7] = 3 * rng.rand(n)
    rows[:, 6] = rows[:, 7] + rng.rand(n) ** 2
    if not plain:
        rows[::7, 5] = 0.0
        rows[3::11, 6] = rows[3::11, 7] - 0.25
        rows[5::13, 5:8] = np.nan
        rows[6::17, 6] = np.nan
        rows[2:3, 6] = np.inf
    return rows


def _segments(n, nseg):
    if nseg == 1:
        return [n], [1.0]
    if nseg == 3:
        return [n // 3, 0, n - n // 3], [0.25, 0.5, 1.0]
    cut = np.sort(np.random.RandomState(nseg).randint(0, n + 1, nseg - 1))
    lens = np.diff(np.concatenate([[0], cut, [n]])).tolist()
    return lens, [0.97 ** (nseg - 1 - s) for s in range(nseg)]


# (k_sample_ksum adds 32 rows per thread and trip while row j + 31 * 256 exists: n >= 7937 enters that loop - at
# 7937 thread 0 alone - and 25576 is three trips plus a tail of different lengths over the threads)
@pytest.mark.parametrize("n,ld", [(1, 16), (1000, 16), (5000, 20), (7936, 16), (7937, 16), (25576, 20)])
def test_weights_are_the_restatement_bit_for_bit(T, n, ld):
    K = T[0]
    rows = _table(n, ld, n)
    d = _dev(rows)
    for nseg in (1, 3, 64):
        lens, fac = _segments(n, nseg)
        for sigma in (0.0, 0.5, 1.0):
            got, gk = K.sample_weights(d, lens, fac, sigma)
            want, wk = R.weights(rows, lens, fac, sigma)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (nseg, sigma)
            assert np.float64(gk).tobytes() == np.float64(wk).tobytes(), (nseg, sigma)
        got, gk = K.sample_weights(None, lens, fac, 0.0)  # no table: recency alone
        assert gk == 0.0 and got.cpu().numpy().tobytes() == R.weights(None, lens, fac, 0.0)[0].tobytes()
    assert d.cpu().numpy().tobytes() == rows.tobytes()  # (the table is read only)
    if n > 1:
        want, wk = R.weights(rows, [n], [1.0], 0.5)
        assert wk > 0 and want.std() > 0 and (want[::7] == 0.5).all()  # no policy: the uniform half alone


def test_weights_of_a_table_without_surprise_and_the_argument_checks(T):
    K = T[0]
    n = 700
    rows = _table(n, 16, 1, plain=True)
    rows[:, 6] = rows[:, 7]  # KL 0 everywhere: K = 0, s = 1
    got, gk = K.sample_weights(_dev(rows), [300, 400], [0.5, 1.0], 0.5)
    want, wk = R.weights(rows, [300, 400], [0.5, 1.0], 0.5)
    assert gk == wk == 0.0 and got.cpu().numpy().tobytes() == want.tobytes()
    assert want.tolist() == [0.5] * 300 + [1.0] * 400
    from yacht_amd._lib import YK_ERR_ARG, YkError
    d = _dev(rows)
    for bad in (lambda: K.sample_weights(None, [n], [1.0], 0.5),          # sigma > 0 needs the table
                lambda: K.sample_weights(d, [n], [1.0], 1.5),
                lambda: K.sample_weights(d, [n], [1.0], float("nan")),
                lambda: K.sample_weights(d, [n], [-1.0], 0.5),
                lambda: K.sample_weights(d, [n], [float("inf")], 0.5),
                lambda: K.sample_weights(d[:, :15].contiguous(), [n], [1.0], 0.5),   # ld < 16
                lambda: K.sample_weights(d, [10] * 70, [1.0] * 70, 0.5),            # 70 segments
                lambda: K.sample_weights(None, [], [], 0.0)):
        with pytest.raises(YkError) as e:
            bad()
        assert e.value.code == YK_ERR_ARG
    with pytest.raises(ValueError):
        K.sample_weights(d, [n - 1], [1.0], 0.5)  # the segments do not cover the table


# ---------------------------------------------------------------- 4. training
A = 3226
STEPS, BATCH, EPOCHS, TSEED = 7, 32, 3, 6


@pytest.fixture(scope="module")
def history(T):
    """Three shards of 96 examples (2 games x 48 moves of an 8-simulation hash-prior self-play) with their
    real policies: the history NNetWrapper.train takes."""
    return _history(T[2])


def _history(RP):
    from yacht_amd.engine import SelfPlayEngine
    out = []
    for it in range(3):
        eng = SelfPlayEngine(2, 8, 1.5, 15, prior="hash", max_moves=48)
        eng.run(23, 100 + 2 * it)
        assert eng.stats()["errors"] == 0
        out.append(RP.examples_from_images(eng.pack_records(), 2, 48, 8))
        eng.close()
    assert [len(s) for s in out] == [96, 96, 96]
    return out


def _wrapper(N, sd, amp, target, **extra):
    from yacht_amd.utils import dotdict
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=EPOCHS, batch_size=BATCH, vloss_weight=1.5, cuda=True, hidden=64,
                   nblocks=1, dropout=0.1, amp=amp, seed=TSEED, policy_target=target, **extra)
    game = type("Game", (), {"getActionSize": lambda self: A})()
    w = N.NNetWrapper(game, args)
    w.nnet.load_state_dict(sd)
    return w


def _init(N):
    torch.manual_seed(2)
    return {k: v.detach().clone() for k, v in N.YachtNNet(hidden=64, nblocks=1, dropout=0.0).state_dict().items()}


def _everything(w):
    tr = w._tr
    m, v = tr.moments()
    out = [tr.params().cpu().numpy().tobytes(), b"".join(m[k].numpy().tobytes() for k in m),
           b"".join(v[k].numpy().tobytes() for k in v), tr.step_count,
           b"".join(t.numpy().tobytes() for t in w.nnet.state_dict().values())]
    if tr.amp:
        out.append(sorted(tr.amp_state().items()))
    return out


def _reference_indices(T, w, history, gamma, sigma, steps=STEPS, batch=BATCH):
    """The restatement's draws for one train call of wrapper w on the history: the per-row table of w's net as
    it stands (the device's, which tests/test_gpu_eval.py holds to its own restatement), then numpy alone."""
    K, N, RP = T
    states, targets, values = RP.as_device_examples(history)
    rows = None
    if sigma > 0:
        rows = w.yk_net().evaluate(states, targets, values, policies=RP.as_device_policies(history),
                                   per_row=True)["rows"].cpu().numpy()
    J = len(history)
    wts, _ = R.weights(rows, [len(s) for s in history], [float(gamma) ** (J - 1 - j) for j in range(J)], sigma)
    table, _ = R.cdf(wts)
    return R.draw(table, TSEED, w._trainer().step_count & 0xFFFFFFFF, 0, steps * batch), wts


def _train_by_hand(T, w, history, gamma, sigma, target, symmetries=()):
    K, N, RP = T
    tr = w._trainer()
    idx, wts = _reference_indices(T, w, history, gamma, sigma)
    states, targets, values = RP.as_device_examples(history)
    pol = RP.as_device_policies(history) if target == "visits" else None
    for e in range(EPOCHS):
        a, b = e * STEPS // EPOCHS, (e + 1) * STEPS // EPOCHS
        st, tg, pl = states, targets, pol
        if symmetries:
            st, tg, pl = K.augment_examples(states, targets, pol, TSEED, tr.step_count & 0xFFFFFFFF, symmetries)
        for k in range(a, b):
            tr.step(st, tg, values, idx=_dev(idx[k * BATCH:(k + 1) * BATCH]), **({"policies": pl} if pol else {}))
    with torch.no_grad():
        w.nnet.load_state_dict(tr.state_dict())
    return idx, wts


@pytest.mark.parametrize("amp", [True, False])
@pytest.mark.parametrize("target", ["argmax", "visits"])
@pytest.mark.parametrize("gamma,sigma", [(1.0, 0.0), (0.5, 0.5)])
def test_sampled_training_is_a_trainer_stepped_by_hand(T, history, gamma, sigma, target, amp):
    """Two train calls of trainSteps = 7 (the second with a step count, hence a key, that is not 0) against a
    second trainer given the restatement's indices step by step: bit-equal parameters, moments, step count
    and GradScaler state.  In f32 every call advances the step count by exactly 7; under amp the GradScaler
    may skip a step (not counted, as torch's): the steps taken plus the halvings of the loss scale are 7."""
    K, N, RP = T
    sd = _init(N)
    knobs = dict(trainSteps=STEPS, sampleRecency=gamma, sampleSurprise=sigma)
    a = _wrapper(N, sd, amp, target, **knobs)
    b = _wrapper(N, sd, amp, target)
    for call in range(2):
        before = a._trainer().step_count
        scale = a._tr.amp_state()["scale"] if amp else 1.0
        a.train(history, verbose=False)
        idx, wts = _train_by_hand(T, b, history, gamma, sigma, target)
        # a skipped step halves the loss scale (and it grows only every 2000 steps): taken + skipped = 7 attempts
        skipped = int(np.log2(scale / a._tr.amp_state()["scale"])) if amp else 0
        assert a._tr.step_count - before + skipped == STEPS and skipped >= 0
        assert _everything(a) == _everything(b), call
        assert (wts.std() > 0) == (gamma != 1.0)
    assert 0 < a._tr.step_count <= 2 * STEPS
    if not amp:  # and the default path is another training altogether: epochs of permutations, 27 steps
        c = _wrapper(N, sd, amp, target)
        c.train(history, verbose=False)
        assert c._tr.step_count == EPOCHS * 9


def test_sampled_training_with_symmetries(T, history):
    K, N, RP = T
    sd = _init(N)
    sym = ("carry", "rolls", "groups")
    a = _wrapper(N, sd, True, "visits", trainSteps=STEPS, sampleRecency=0.5, sampleSurprise=0.5, symmetries=sym)
    b = _wrapper(N, sd, True, "visits")
    a.train(history, verbose=True)  # (with the report lines: three rounds)
    _train_by_hand(T, b, history, 0.5, 0.5, "visits", sym)
    assert _everything(a) == _everything(b)
    c = _wrapper(N, sd, True, "visits", trainSteps=STEPS, sampleRecency=0.5, sampleSurprise=0.5)
    c.train(history, verbose=False)
    assert _everything(c)[0] != _everything(a)[0]


def test_fewer_steps_than_rounds_and_one_segment(T, history):
    """trainSteps = 2 over 3 epochs: rounds of 0, 1 and 1 steps; a single shard is one segment (recency has
    nothing to act on), and so is a list of tuples."""
    K, N, RP = T
    sd = _init(N)
    a = _wrapper(N, sd, False, "argmax", trainSteps=2, sampleRecency=0.5)
    a.train(history[0], verbose=True)
    assert a._tr.step_count == 2
    b = _wrapper(N, sd, False, "argmax")
    idx = R.draw(R.cdf(np.ones(96))[0], TSEED, 0, 0, 2 * BATCH)
    states, targets, values = RP.as_device_examples(history[0])
    for k in range(2):
        b._trainer().step(states, targets, values, idx=_dev(idx[k * BATCH:(k + 1) * BATCH]))
    assert _everything(a)[:4] == _everything(b)[:4]
    c = _wrapper(N, sd, False, "argmax", trainSteps=2, sampleRecency=0.5)
    c.train(list(history[0]), verbose=False)
    assert _everything(c) == _everything(a)


def test_knobs_that_cannot_be_served_raise(T, history):
    K, N, RP = T
    sd = _init(N)
    bare = [RP.ExampleShard(s.states, s.targets, s.values) for s in history]
    w = _wrapper(N, sd, False, "argmax", trainSteps=STEPS, sampleSurprise=0.5)
    with pytest.raises(ValueError, match="policies"):
        w.train(bare, verbose=False)
    assert w._trainer().step_count == 0
    _wrapper(N, sd, False, "argmax", trainSteps=STEPS, sampleRecency=0.5).train(bare, verbose=False)  # recency alone: fine
    for knobs in (dict(sampleRecency=0.5), dict(sampleSurprise=0.5), dict(trainSteps=-1), dict(trainSteps=3, sampleRecency=0.0)):
        w = _wrapper(N, sd, False, "argmax", **knobs)
        with pytest.raises(ValueError, match="trainSteps|sampleRecency"):
            w.train(history, verbose=False)
        assert getattr(w, "_tr", None) is None  # before any device work
    with pytest.raises(ValueError, match="examples"):
        _wrapper(N, sd, False, "argmax", trainSteps=3).train([], verbose=False)


# ---------------------------------------------------------------- 5. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out):
    import sys
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (here, os.path.join(here, "nypc-yacht-auction_amd"), os.path.join(here, "tests")):
        sys.path.insert(0, p)
    torch.cuda.set_device(0)  # both ranks share the one GPU of the box
    from yacht_amd import nnet as N
    from yacht_amd import replay as RP
    hist = _history(RP)
    sd = _init(N)
    for mode in ("replicated", "split", "per_rank"):
        w = _wrapper(N, sd, False, "visits", trainSteps=STEPS, sampleRecency=0.5, sampleSurprise=0.5, ddp_batch=mode)
        w.train(hist, verbose=False)
        out[f"{mode}{rank}"] = (_everything(w), w._tr.step_count)
    dist.destroy_process_group()


def test_two_ranks_sharing_gpu0(T, history):
    import torch.multiprocessing as mp
    K, N, RP = T
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.start_processes(_rank_worker, args=(2, _free_port(), out), nprocs=2, start_method="spawn")
    single = _wrapper(N, _init(N), False, "visits", trainSteps=STEPS, sampleRecency=0.5, sampleSurprise=0.5)
    single.train(history, verbose=False)
    # replicated: every rank takes the whole drawn minibatch's step - the single process, bit for bit
    assert out["replicated0"][0] == out["replicated1"][0] == _everything(single)
    # split and per_rank: the same draws on both ranks, the gradients all-reduced - both ranks identical
    for mode in ("split", "per_rank"):
        assert out[f"{mode}0"] == out[f"{mode}1"] and out[f"{mode}0"][1] == STEPS
    assert out["per_rank0"][0][0] != out["replicated0"][0][0]  # (64 drawn rows per step, not 32)


# ---------------------------------------------------------------- 6. Coach
COACH = dict(numIters=2, numEps=6, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000, numMCTSSims=4,
             arenaCompare=6, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3, weight_decay=1e-4, epochs=2,
             batch_size=40, vloss_weight=1.5, cuda=True, hidden=64, nblocks=1, dropout=0.0, seed=3,
             amp=False)  # tests/test_gpu_coach.py's, the smallest Coach configuration of the suite; two iterations


def test_coach_with_sampled_training(T, tmp_path):
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    ck = str(tmp_path / "ck")
    torch.manual_seed(5)
    args = dotdict(COACH, checkpoint=ck, load_folder_file=(ck, "best.pth.tar"), trainSteps=5, sampleRecency=0.5,
                   sampleSurprise=0.5)
    game = YachtGame(seed=21, env_id=500)
    coach = Coach(game, NNetWrapper(game, args), args)
    coach.learn()
    assert coach.nnet._trainer().step_count == 10
    assert set(coach.phase_times) == {"selfplay_s", "save_s", "train_s", "arena_s", "gate_s", "iteration_s"}
    assert [len(s) for s in coach.trainExamplesHistory] == [6 * 48] * 2
    with pytest.raises(ValueError, match="trainSteps"):
        Coach(game, NNetWrapper(game, args), dotdict(COACH, sampleRecency=0.5))
