"""The weighted minibatch sampling restated in numpy float64 (include/yacht_hip.h,
yk_sample_weights / yk_sample_cdf / yk_sample_draw): oracle/spec.py's Philox vectorised, the cumulative table
as per-chunk np.cumsum plus a Python loop for the chunks' offsets, and K in tests/eval_ref.py's summation
order - one float64 operation per step, so the device's numbers can be compared bit for bit."""
import numpy as np

CHUNK, NPART = 256, 256
DOMAIN = 0x20000000  # counter word 3 of the sampling draws
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """spec.philox4x32_10 over arrays of counters (uint64 arrays holding 32-bit words; scalar key words)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, ((p0 >> S32) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(seed, key, first, m, domain=DOMAIN):
    """u of draws first .. first + m - 1: counter (j lo, j hi, key, domain), key (seed lo, seed hi),
    x = x0 | x1 << 32, u = (x >> 11) * 2^-53."""
    j = (np.uint64(int(first) & (2**64 - 1)) + np.arange(m, dtype=np.uint64))  # (wraps mod 2^64 like the device)
    seed = int(seed) & (2**64 - 1)
    x0, x1, _, _ = philox(j & M32, j >> S32, np.uint64(int(key) & 0xFFFFFFFF), np.uint64(domain), seed & 0xFFFFFFFF, seed >> 32)
    x = x0 | (x1 << S32)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def kl(rows):
    """k_i = max(0, (c - h) / S) when S > 0 and the quotient is finite, else 0 (columns 5, 6, 7)."""
    rows = np.asarray(rows, dtype=np.float64)
    S, c, h = rows[:, 5], rows[:, 6], rows[:, 7]
    with np.errstate(all="ignore"):
        q = (c - h) / S
    ok = (S > 0) & np.isfinite(q) & (q > 0)
    return np.where(ok, q, 0.0)


def ksum(k):
    """The sum in eval_ref.sums' order: partial j = ((0.0 + k[j]) + k[j + 256]) + ...; K = ((0.0 + partial 0) +
    partial 1) + ... + partial 255."""
    k = np.asarray(k, dtype=np.float64)
    partials = np.zeros(NPART, dtype=np.float64)
    for g in range((len(k) + NPART - 1) // NPART):
        blk = k[g * NPART:(g + 1) * NPART]
        partials[:len(blk)] = partials[:len(blk)] + blk
    total = np.float64(0.0)
    for j in range(NPART):
        total = total + partials[j]
    return float(total)


def weights(rows, seg_lens, seg_factors, surprise):
    """(w float64[n], K): w[i] = factor of i's segment * s_i, s_i = 1 when surprise == 0 or K == 0, else
    (1 - surprise) + surprise * ((n k_i) / K).  rows None (surprise 0 only): K = 0."""
    n = int(sum(seg_lens))
    sigma = np.float64(surprise)
    fac = np.repeat(np.asarray(seg_factors, dtype=np.float64), np.asarray(seg_lens, dtype=np.int64))
    K = 0.0
    s = np.ones(n, dtype=np.float64)
    if rows is not None:
        k = kl(rows)
        K = ksum(k)
        if sigma != 0 and K != 0:
            with np.errstate(all="ignore"):
                a = np.float64(n) * k
                b = a / np.float64(K)
                c2 = sigma * b
                s = (np.float64(1.0) - sigma) + c2
    else:
        assert sigma == 0
    return fac * s, K


def cdf(w):
    """(cdf float64[n], total): L = the sequential inclusive sum from 0.0 within each chunk of 256; O[0] = 0.0,
    O[c + 1] = O[c] + L[last of c]; cdf[i] = O[c] + L[i]."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    out = np.empty(n, dtype=np.float64)
    off = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, CHUNK):
            L = np.cumsum(np.concatenate([[0.0], w[i0:i0 + CHUNK]]))[1:]  # (sequential; from 0.0 as the device)
            out[i0:i0 + CHUNK] = off + L
            off = off + L[-1]
    return out, float(out[-1])


def locate(table, t):
    """searchsorted(table, t, 'right'), and where that is n the first i with table[i] >= table[-1]."""
    table = np.asarray(table, dtype=np.float64)
    i = np.searchsorted(table, t, side="right")
    first_total = np.searchsorted(table, table[-1], side="left")
    return np.where(i >= len(table), first_total, i).astype(np.int32)


def draw(table, seed, key, first, m):
    """idx int32[m] of draws first .. first + m - 1 in the cumulative table."""
    table = np.asarray(table, dtype=np.float64)
    t = uniforms(seed, key, first, m) * table[-1]
    return locate(table, t)
