"""Numpy restatement of the search-value targets (include/yacht_hip.h:
yk_engine_config_t.record_root_values and yk_examples_value_targets).  Every operation is one float64
operation on scalars, rounded on its own; the result is rounded to float32 once at the end."""
import numpy as np

ZERO_WORD = np.uint32(0x80000000)  # +0 and -0 are both recorded as this word
NAN_WORD = np.uint32(0x7FC00000)   # what an absent value (word 0) decodes to


def root_value(triples):
    """q64 of a root from its (action, N, Q) triples in ascending action order: the visit-weighted mean of Q
    over the edges with N > 0 (NaN when there is none)."""
    num, den = np.float64(0.0), np.float64(0.0)
    for _, n, q in triples:
        if int(n) > 0:
            w = np.float64(int(n))
            num = num + w * np.float64(q)
            den = den + w
    return num / den if den != 0 else np.float64("nan")


def encode(q32):
    """float32 value(s) -> the uint32 word(s) of info[..., 7]: the bit pattern, +-0 as 0x80000000."""
    w = np.asarray(q32, dtype=np.float32).view(np.uint32)
    return np.where((w << np.uint32(1)) == 0, ZERO_WORD, w).astype(np.uint32)


def decode(words):
    """uint32 word(s) -> float32: the bit pattern, NaN for the zero word ("no value recorded")."""
    w = np.asarray(words).astype(np.uint32)
    return np.where(w == 0, NAN_WORD, w).astype(np.uint32).view(np.float32)


def value_targets(q, z, players, n_moves, beta, lam):
    """One game.  q float32[>= T] decoded root values (NaN where absent), z float64[>= T] outcomes, players
    int[>= T] (+1 / -1), T = n_moves -> float32[T] targets.  lam == 1 skips the recursion (G_t = Z_t) and
    beta == 0 the q_t term, so (0, 1) reads no q."""
    T = int(n_moves)
    beta, lam = np.float64(beta), np.float64(lam)
    one = np.float64(1.0)
    p = [np.float64(int(players[t])) for t in range(T)]
    qd = [np.float64(np.float32(q[t])) for t in range(T)]
    W = [p[t] * qd[t] for t in range(T)]
    Z = [p[t] * np.float64(z[t]) for t in range(T)]
    G = list(Z)
    if lam != 1.0:
        for t in range(T - 2, -1, -1):
            G[t] = (one - lam) * W[t + 1] + lam * G[t + 1]
    out = np.zeros(T, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            target = p[t] * G[t]
            v = target if beta == 0.0 else (one - beta) * target + beta * qd[t]
            out[t] = np.float32(v)
    return out


def needs_missing(words, n_moves, beta, lam):
    """bool[T]: move t's formula reads a root value whose word is 0 - its own when beta != 0, any later
    move's when lam != 1 (what yk_examples_value_targets counts in n_missing)."""
    T = int(n_moves)
    absent = np.asarray(words[:T]).astype(np.uint32) == 0
    out = np.zeros(T, dtype=bool)
    for t in range(T):
        out[t] = (beta != 0.0 and absent[t]) or (lam != 1.0 and absent[t + 1:].any())
    return out
