"""Soft policy targets, the host half (no GPU): the CSR of the full policies that
policy_target="visits" trains on, from the reference's (board, pi, v) tuples, and the argument
checks of the soft entry points."""
import os

import numpy as np
import pytest

import yacht_amd
from conftest import REPO
from yacht_amd import examples_io as X
from yacht_amd import replay as R


@pytest.fixture(scope="module")
def hist():
    return X.load_reference_examples(os.path.join(REPO, "tests", "golden", "examples_ref.pkl"))


def _dense(csr, n):
    indptr, cols, vals = csr
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    assert indptr.shape == (n + 1,) and indptr[0] == 0 and indptr[-1] == len(cols) == len(vals)
    pi = np.zeros((n, 3226))
    for k in range(n):
        c = cols[indptr[k]:indptr[k + 1]]
        assert (np.diff(c) > 0).all(), k  # ascending, no duplicates
        pi[k, c] = vals[indptr[k]:indptr[k + 1]]
    return pi


def test_tuple_list_gives_the_dense_pi_exactly(hist):
    flat = [e for it in hist for e in it]
    assert flat and any(np.count_nonzero(p) > 1 for _, p, _ in flat)
    csr = R.policies_csr_host(flat)
    want = np.array([p for _, p, _ in flat], dtype=np.float64)
    assert np.array_equal(_dense(csr, len(flat)), want)
    assert (csr[2] != 0).all() and len(csr[1]) == np.count_nonzero(want)  # the nonzero entries, no others
    # more rows than one conversion chunk
    many = (flat * (1100 // len(flat) + 1))[:1100]
    assert np.array_equal(_dense(R.policies_csr_host(many), 1100), np.array([p for _, p, _ in many]))


def test_history_concatenates_with_offsets(hist):
    flat = [e for it in hist for e in it]
    a, b = flat[:len(flat) // 3], flat[len(flat) // 3:]
    assert a and b
    whole = R.policies_csr_host(flat)
    parts = R.policies_csr_host([a, [], b])  # an empty iteration contributes nothing
    for x, y in zip(whole, parts):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    ia, ib = R.policies_csr_host(a)[0], R.policies_csr_host(b)[0]
    assert np.array_equal(parts[0], np.concatenate([ia, ib[1:] + ia[-1]]))
    empty = R.policies_csr_host([[], []])
    assert np.array_equal(empty[0], [0]) and len(empty[1]) == 0 and len(empty[2]) == 0


def test_examples_file_round_trip_keeps_the_csr(hist, tmp_path):
    p = str(tmp_path / "buf.npz")
    X.save_examples(p, hist)
    back = X.load_examples(p)
    for x, y in zip(R.policies_csr_host(hist), R.policies_csr_host(back)):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_shard_without_policies_names_the_option():
    shard = R.ExampleShard(np.zeros((2, 8), np.int64), np.zeros(2, np.int32), np.zeros(2, np.float32))
    for f in (R.policies_csr_host, R.as_device_policies):
        with pytest.raises(ValueError, match="policy_target"):
            f(shard)
        with pytest.raises(ValueError, match="policy_target"):
            f([shard])


def test_unknown_policy_target_raises():
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    game = type("Game", (), {"getActionSize": lambda self: 3226})()
    args = dotdict(lr=2e-3, weight_decay=1e-4, epochs=1, batch_size=8, vloss_weight=1.5, cuda=True, hidden=64,
                   nblocks=1, dropout=0.0, policy_target="soft")
    with pytest.raises(ValueError, match="policy_target"):
        NNetWrapper(game, args).train([], verbose=False)


def test_soft_entry_points_reject_null_arguments_without_a_gpu():
    lib = yacht_amd.lib()
    for f in (lib.yk_trainer_backward_soft, lib.yk_trainer_step_soft):
        assert f(None, None, None, None, None, None, None, 1, None) == -1
