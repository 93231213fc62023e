"""The held-out evaluation's numbers restated in numpy float64 (include/yacht_hip.h,
yk_examples_metrics): ``rows`` computes the 16 columns of every example with np.exp / np.log, ``sums``
repeats the column sums' order with explicit loops, so the device's sums can be compared bit for bit."""
import numpy as np

ASIZE, NCOL, NPART = 3226, 16, 256


def rows(logits, v, valid, targets, values, csr=None, batch_idx=None):
    """logits f32[n, >= 3226] and v f32[n] (row i belongs to example r = batch_idx[i], or i); valid
    bool[N, 3226] (getValidMoves of example r's board for player 1), targets int[N], values f32[N] and
    csr = (indptr[N + 1], cols, vals f64) or None, indexed by r -> float64 [n, 16]."""
    logits = np.asarray(logits)
    n = logits.shape[0]
    out = np.zeros((n, NCOL), dtype=np.float64)
    for i in range(n):
        r = int(batch_idx[i]) if batch_idx is not None else i
        x32 = np.asarray(logits[i, :ASIZE], dtype=np.float32)
        x = x32.astype(np.float64)
        t = int(targets[r])
        t_in = 0 <= t < ASIZE
        m = x.max()
        e = np.exp(x - m)
        s = e.sum()
        lse = m + np.log(s)
        if t_in:
            rank = int(np.count_nonzero(x > x[t]) + np.count_nonzero(x[:t] == x[t]))
        else:
            rank = ASIZE
        S = soft = tent = 0.0
        if csr is not None:
            indptr, cols, vals = csr
            a0, a1 = int(indptr[r]), int(indptr[r + 1])
            c = np.asarray(cols[a0:a1], dtype=np.int64)
            p = np.asarray(vals[a0:a1], dtype=np.float64)
            S = p.sum()
            ok = (c >= 0) & (c < ASIZE)
            soft = (p[ok] * (lse - x[c[ok]])).sum()
            pos = p > 0
            tent = -(p[pos] * np.log(p[pos])).sum()
        vd, z = np.float64(np.float32(v[i])), np.float64(np.float32(values[r]))
        d = vd - z
        out[i] = [lse, lse - x[t] if t_in else 0.0, rank, lse - (e * x).sum() / s,
                  e[np.asarray(valid[r], dtype=bool)].sum() / s, S, soft, tent, vd, d, d * d,
                  1.0 if vd * z > 0 else 0.0, 1.0 if rank == 0 else 0.0, 1.0 if rank < 5 else 0.0,
                  0.0 if t_in else 1.0, 1.0]
    return out


def sums(rows_):
    """The column sums in the kernels' order: partial j (0..255) = ((0.0 + row j) + row j + 256) + ... in
    ascending order; the sum = ((0.0 + partial 0) + partial 1) + ... + partial 255.  Explicit loops: one
    float64 addition per element and step, nothing left to np.sum's own order."""
    rows_ = np.asarray(rows_, dtype=np.float64).reshape(-1, NCOL)
    n = rows_.shape[0]
    partials = np.zeros((NPART, NCOL), dtype=np.float64)
    for g in range((n + NPART - 1) // NPART):  # row group g: rows 256 g .. 256 g + 255, one per partial
        blk = rows_[g * NPART:(g + 1) * NPART]
        partials[:blk.shape[0]] = partials[:blk.shape[0]] + blk
    total = np.zeros(NCOL, dtype=np.float64)
    for j in range(NPART):
        total = total + partials[j]
    return total
