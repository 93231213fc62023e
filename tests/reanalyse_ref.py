"""The reanalysis' three device calls restated in numpy (include/yacht_hip.h,
yk_reanalyse_select / yk_policies_from_counts / yk_policies_splice): oracle/spec.py's Philox for the
selection, Python loops for the rows - one float64 operation per step, so the device's numbers can be
compared bit for bit."""
import numpy as np

from oracle import spec

A = 3226
DOMAIN = 0x10000000  # counter word 3 of the selection draws
M32, M64 = 0xFFFFFFFF, 2**64 - 1


def uniform(seed, key, k):
    """u of example k: counter (k lo, k hi, key, DOMAIN), key (seed lo, seed hi), x = x0 | x1 << 32,
    u = (x >> 11) * 2^-53."""
    seed, k = int(seed) & M64, int(k) & M64
    x0, x1, _, _ = spec.philox4x32_10(k & M32, k >> 32, int(key) & M32, DOMAIN, seed & M32, seed >> 32)
    return float((x0 | (x1 << 32)) >> 11) * (1.0 / 9007199254740992.0)


def select(n, index_base, seed, key, fraction):
    """The chosen rows i of 0 .. n-1, ascending (int32): row i is example index_base + i (mod 2^64), chosen iff
    its uniform lies below fraction."""
    return np.asarray([i for i in range(int(n)) if uniform(seed, key, int(index_base) + i) < fraction], dtype=np.int32)


def from_counts(counts):
    """counts int32[n][3226] -> (indptr int64[n+1], cols int32, vals float64, targets int32[n], n_empty): the
    positive counts of every row in ascending action order, each over their sequential float64 sum; the target
    the lowest action among the largest counts, -1 for a row without a positive count."""
    counts = np.asarray(counts, dtype=np.int32).reshape(-1, A)
    indptr, cols, vals, targets, n_empty = [0], [], [], [], 0
    for row in counts:
        pos = np.nonzero(row > 0)[0]
        if len(pos) == 0:
            n_empty += 1
            targets.append(-1)
        else:
            s = np.float64(0.0)
            for c in row[pos]:
                s = s + np.float64(c)
            cols.append(pos.astype(np.int32))
            vals.append(row[pos].astype(np.float64) / s)
            targets.append(int(pos[np.argmax(row[pos])]))  # (argmax: the first of the largest)
        indptr.append(indptr[-1] + len(pos))
    return (np.asarray(indptr, dtype=np.int64), np.concatenate(cols) if cols else np.zeros(0, dtype=np.int32),
            np.concatenate(vals) if vals else np.zeros(0, dtype=np.float64), np.asarray(targets, dtype=np.int32), n_empty)


def splice(indptr, cols, vals, idx, new_indptr, new_cols, new_vals):
    """Rows idx (strictly ascending) of the CSR replaced by the rows of the new CSR; an empty new row keeps the
    old one.  Returns (indptr, cols, vals), indptr[0] = 0."""
    n = len(indptr) - 1
    idx = [int(x) for x in idx]
    assert all(0 <= x < n for x in idx) and all(a < b for a, b in zip(idx, idx[1:]))
    src = {x: j for j, x in enumerate(idx) if new_indptr[j + 1] > new_indptr[j]}
    out_ip, out_c, out_v = [0], [], []
    for i in range(n):
        if i in src:
            a, b, c, v = int(new_indptr[src[i]]), int(new_indptr[src[i] + 1]), new_cols, new_vals
        else:
            a, b, c, v = int(indptr[i]), int(indptr[i + 1]), cols, vals
        out_c.append(np.asarray(c[a:b], dtype=np.int32))
        out_v.append(np.asarray(v[a:b], dtype=np.float64))
        out_ip.append(out_ip[-1] + (b - a))
    return (np.asarray(out_ip, dtype=np.int64), np.concatenate(out_c) if out_c else np.zeros(0, dtype=np.int32),
            np.concatenate(out_v) if out_v else np.zeros(0, dtype=np.float64))
