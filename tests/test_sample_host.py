"""The weighted minibatch sampling without a GPU: tests/sample_ref.py - the
restatement tests/test_gpu_sample.py holds the device to - against oracle/spec.py's Philox and its own
claims (a nondecreasing table, zero weights never drawn, the t >= total rule, the drawn frequencies), and the
knob checks and the round partition of yacht_amd.replay."""
import numpy as np
import pytest

import sample_ref as R
from oracle import spec


def test_vectorised_philox_is_the_specs_and_the_domain_is_new():
    rng = np.random.RandomState(1)
    js = [0, 1, 2**32 - 1, 2**32, 2**32 + 5, 2**63 + 11] + [int(x) for x in rng.randint(0, 2**62, 20)]
    for seed, key in ((0, 0), (20240607, 3), (0xFEDCBA9876543210, 0xFFFFFFFF)):
        c = [np.array([j & 0xFFFFFFFF for j in js], dtype=np.uint64), np.array([j >> 32 for j in js], dtype=np.uint64)]
        got = R.philox(c[0], c[1], key, R.DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
        for n, j in enumerate(js):
            want = spec.philox4x32_10(j & 0xFFFFFFFF, j >> 32, key, R.DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
            assert tuple(int(w[n]) for w in got) == want
            x = want[0] | (want[1] << 32)
            assert R.uniforms(seed, key, j, 1)[0] == (x >> 11) * (1.0 / 9007199254740992.0)
            for tag in (0, 0x40000000, 0x80000000):  # the game streams, the symmetries, the root noise at move 0
                assert spec.philox4x32_10(j & 0xFFFFFFFF, j >> 32, key, tag, seed & 0xFFFFFFFF, seed >> 32) != want
        # tag 0 is the game stream itself: draw64(seed, env = key, ctr = j)
        assert int(R.uniforms(seed, key, 7, 1, domain=0)[0] * 2**53) == spec.draw64(seed, key, 7) >> 11
    # a range of draws is that range of a longer call, across the carry into counter word 1
    whole = R.uniforms(5, 9, 2**32 - 3, 8)
    assert np.array_equal(whole[3:], R.uniforms(5, 9, 2**32, 5)) and len(set(whole.tolist())) == 8


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 65537])
def test_reference_cdf_is_nondecreasing(n):
    w = np.exp(3 * np.random.RandomState(n).randn(n))
    c, total = R.cdf(w)
    assert (np.diff(c) >= 0).all() and total == c[-1] and c[0] == w[0]
    assert abs(total - np.sum(w)) <= 1e-12 * total  # (and it is the sum, in another order)
    # every chunk's last element is the next chunk's offset: the two-level search equals the flat one
    for i0 in range(256, n, 256):
        assert np.array_equal(c[i0:i0 + 256], c[i0 - 1] + np.cumsum(w[i0:i0 + 256]))


def test_zero_weights_are_never_drawn_and_the_total_rule():
    w = np.array([0.0, 2.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    c, total = R.cdf(w)
    assert total == 3.0
    idx = R.draw(c, 3, 4, 0, 20000)
    assert set(idx.tolist()) == {1, 4}
    # t at and past the total: the first index that reaches the total, not n and not a trailing zero
    assert R.locate(c, np.array([0.0, 1.999, 2.0, 2.999, 3.0, 3.5])).tolist() == [1, 1, 4, 4, 4, 4]
    # an absorbed weight is a zero weight
    c, total = R.cdf(np.array([1e300, 1e-300, 1e-300]))
    assert total == 1e300 and R.locate(c, np.array([0.0, 1e300])).tolist() == [0, 0]
    # leading zeros: t = 0 lands on the first positive weight
    assert R.locate(R.cdf(np.array([0.0, 0.0, 5.0]))[0], np.array([0.0])).tolist() == [2]


@pytest.mark.parametrize("seed,key", [(20240607, 3), (1, 0), (99, 12345)])
def test_drawn_frequencies(seed, key):
    """n = 1000, weights exp(N(0, 1)) with every 7th zero, m = 2^20: the chi-square statistic over the positive
    cells lies within 5 standard deviations of its degrees of freedom (a chi-square with dof degrees has
    mean dof and variance 2 dof)."""
    n, m = 1000, 2**20
    w = np.exp(np.random.RandomState(7).randn(n))
    w[::7] = 0.0
    c, total = R.cdf(w)
    counts = np.bincount(R.draw(c, seed, key, 0, m), minlength=n)
    assert counts[w == 0].sum() == 0
    pos = w > 0
    expect = m * w[pos] / w[pos].sum()
    chi2 = float((((counts[pos] - expect) ** 2) / expect).sum())
    dof = int(pos.sum()) - 1
    z = (chi2 - dof) / np.sqrt(2 * dof)
    print(f"seed {seed} key {key}: chi2 {chi2:.1f}, dof {dof}, z {z:+.2f}")
    assert abs(chi2 - dof) <= 5 * np.sqrt(2 * dof)


def test_reference_weights():
    rows = np.zeros((6, 16))
    rows[:, 5] = [1.0, 1.0, 0.0, 2.0, np.nan, 1.0]
    rows[:, 6] = [3.0, 1.0, 5.0, 5.0, 1.0, np.inf]
    rows[:, 7] = [1.0, 2.0, 1.0, 1.0, 0.0, 0.0]
    assert R.kl(rows).tolist() == [2.0, 0.0, 0.0, 2.0, 0.0, 0.0]  # negative, no policy, NaN, infinite: 0
    w, K = R.weights(rows, [2, 0, 4], [0.25, 0.5, 1.0], 0.5)
    assert K == 4.0 and w.tolist() == [0.25 * 2.0, 0.25 * 0.5, 0.5, 2.0, 0.5, 0.5]
    w, K = R.weights(rows, [6], [1.0], 1.0)
    assert w.tolist() == [3.0, 0.0, 0.0, 3.0, 0.0, 0.0] and w.sum() == 6.0  # sigma 1: the mean weight stays 1
    assert R.weights(None, [2, 1], [0.5, 1.0], 0.0)[0].tolist() == [0.5, 0.5, 1.0]
    w, K = R.weights(np.zeros((3, 16)), [3], [2.0], 1.0)  # K == 0: s = 1
    assert K == 0.0 and w.tolist() == [2.0, 2.0, 2.0]
    k = np.random.RandomState(2).rand(1000)
    assert abs(R.ksum(k) - np.sum(k)) < 1e-10 and R.ksum(k[:1]) == k[0]


def test_knob_checks_and_the_round_partition():
    from yacht_amd.replay import check_sample_knobs, sample_rounds
    assert check_sample_knobs() == (0, 1.0, 0.0)
    assert check_sample_knobs(7, 0.5, 1) == (7, 0.5, 1.0)
    assert check_sample_knobs(3, 1, 0) == (3, 1.0, 0.0)
    for bad in ((-1, 1.0, 0.0), (2.5, 1.0, 0.0), (True, 1.0, 0.0), (4, 0.0, 0.0), (4, 1.5, 0.0), (4, float("nan"), 0.0),
                (4, 1.0, -0.1), (4, 1.0, 1.1), (4, 1.0, float("nan")),
                (0, 0.5, 0.0), (0, 1.0, 0.5)):  # the weights set while the sampling is off
        with pytest.raises(ValueError):
            check_sample_knobs(*bad)
    for T, E in ((7, 3), (400, 15), (2, 5), (1, 1), (15, 15), (0, 4), (29310, 15)):
        r = sample_rounds(T, E)
        assert len(r) == E and r[0][0] == 0 and r[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(a <= b for a, b in r)
        assert sum(b - a for a, b in r) == T
        assert all(a == e * T // E for e, (a, _) in enumerate(r))
        assert max(b - a for a, b in r) <= -(-T // E)
    assert sample_rounds(7, 3) == [(0, 2), (2, 4), (4, 7)]
    assert [b - a for a, b in sample_rounds(2, 5)] == [0, 0, 1, 0, 1]  # T < E leaves empty rounds
    assert all(a == b for a, b in sample_rounds(0, 4))                  # T = 0 is off


def test_sample_segments():
    from yacht_amd.replay import ExampleShard, sample_segments
    ex = ("board", [0.0], 1.0)
    assert sample_segments([ex, ex, ex], 0.5) == ([3], [1.0])
    assert sample_segments([[ex, ex], [], [ex]], 0.5) == ([2, 1], [0.25, 1.0])
    assert sample_segments([[ex], [ex, ex], [ex]], 1.0) == ([1, 2, 1], [1.0, 1.0, 1.0])
    assert sample_segments([[[ex], [ex]], [ex]], 0.5) == ([2, 1], [0.5, 1.0])
    assert sample_segments([], 0.5) == ([0], [1.0])
    with pytest.raises(ValueError):
        sample_segments([[ex]] * 65, 0.5)
    import torch
    sh =ExampleShard(torch.zeros((4, 8), dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(4))
    assert sample_segments(sh, 0.5) == ([4], [1.0])
    assert sample_segments([sh, [ex], sh], 0.5) == ([4, 1, 4], [0.25, 0.5, 1.0])
