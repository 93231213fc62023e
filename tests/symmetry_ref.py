"""Reference restatement of the symmetry augmentation.  TEST INFRASTRUCTURE ONLY.

The normative definition yk_examples_augment implements, in plain Python / NumPy on the packed words of
oracle/spec.py.  Example k (a global index into the pooled examples), epoch key t, seed and a bit-set of
CARRY / ROLLS / GROUPS give a state transform T and an action bijection A_k of 0..3225:

* draw i is Philox4x32-10 with counter (i, k & 0xffffffff, t, 0x40000000) under key (seed lo, seed hi);
  below_i(n) = (x1 * n) >> 32 with x1 the output's word 1 (the game streams' rule; their counter word 3 is 0
  and the root noise's is 0x80000000 | move, so the three domains are disjoint);
* a list of length L with first draw b is permuted by Fisher-Yates: perm = [0..L-1]; for m = L-1 .. 1:
  j = below_{b + (L-1-m)}(m + 1), swap perm[m], perm[j]; new[i] = old[perm[i]];
* first draws: p1 carry 0, p2 carry 16, rollA 32, rollB 40; the group swap happens iff draw 48's x1 >> 31.
"""
import itertools

import numpy as np

from oracle import spec

M32 = spec.M32
ASIZE = spec.ACTION_SIZE
NBID, NCOMB, LEVELS = spec.NUM_BID_ACTIONS, spec.NUM_COMB, spec.BID_LEVELS
CARRY, ROLLS, GROUPS = 1, 2, 4
FLAG_OF = {"carry": CARRY, "rolls": ROLLS, "groups": GROUPS}
BASE_P1, BASE_P2, BASE_A, BASE_B, DRAW_SWAP = 0, 16, 32, 40, 48
COMBOS = list(itertools.combinations(range(10), 5))
RANK = {c: i for i, c in enumerate(COMBOS)}


def x1(i, k, t, seed):
    return spec.philox4x32_10(i & M32, k & M32, t & M32, 0x40000000, seed & M32, (seed >> 32) & M32)[1]


def below(i, n, k, t, seed):
    return (x1(i, k, t, seed) * n) >> 32


def fisher_yates(L, b, k, t, seed):
    perm = list(range(L))
    for m in range(L - 1, 0, -1):
        j = below(b + (L - 1 - m), m + 1, k, t, seed)
        perm[m], perm[j] = perm[j], perm[m]
    return perm


def _nib(v, n):
    return [(v >> (4 * i)) & 0xF for i in range(n)]


def _pack(d):
    return sum(int(x) << (4 * i) for i, x in enumerate(d))


def plan(words, k, t, seed, flags):
    """The draws example k's state asks for: perm1 / perm2 over the carries' own lengths, permA / permB over
    the rolls (identity when the flag is off or the roll absent) and whether the groups are swapped."""
    w0 = int(words[0])
    n1, n2 = (int(words[1]) >> 40) & 0xF, (int(words[4]) >> 40) & 0xF
    hasA, hasB = (w0 >> 5) & 1, (w0 >> 6) & 1
    return dict(
        perm1=fisher_yates(n1, BASE_P1, k, t, seed) if flags & CARRY else list(range(n1)),
        perm2=fisher_yates(n2, BASE_P2, k, t, seed) if flags & CARRY else list(range(n2)),
        permA=fisher_yates(5, BASE_A, k, t, seed) if flags & ROLLS and hasA else list(range(5)),
        permB=fisher_yates(5, BASE_B, k, t, seed) if flags & ROLLS and hasB else list(range(5)),
        swap=bool(flags & GROUPS) and bool(x1(DRAW_SWAP, k, t, seed) >> 31))


def transform_state(words, pl):
    """T: the 8 words of the augmented state.  Everything the plan does not name is copied."""
    w = [int(x) for x in words]
    for base, perm in ((1, pl["perm1"]), (4, pl["perm2"])):
        old = _nib(w[base], len(perm))
        w[base] = (w[base] & ~((1 << (4 * len(perm))) - 1)) | _pack([old[p] for p in perm])
    w0 = w[0]
    ra, rb = _nib(w0 >> 24, 5), _nib(w0 >> 44, 5)
    ra, rb = [ra[p] for p in pl["permA"]], [rb[p] for p in pl["permB"]]
    hasA, hasB = (w0 >> 5) & 1, (w0 >> 6) & 1
    b1, b2 = (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF
    if pl["swap"]:
        ra, rb, hasA, hasB = rb, ra, hasB, hasA
        b1, b2 = (b if b == 0xFF else b ^ 0x80 for b in (b1, b2))
    w[0] = (w0 & 0x9F) | (hasA << 5) | (hasB << 6) | (b1 << 8) | (b2 << 16) | (_pack(ra) << 24) | (_pack(rb) << 44)
    return np.array(w, dtype=np.uint64)


def map_action(a, words, pl):
    """A_k: a bijection of 0..3225 (examples are canonical boards: the mover is p1)."""
    a = int(a)
    phase = (int(words[0]) >> 4) & 1
    if phase == 0 and 0 <= a < NBID:
        return (a + LEVELS) % NBID if pl["swap"] else a
    if phase == 1 and NBID <= a < ASIZE:
        cat, ci = divmod(a - NBID, NCOMB)
        c = COMBOS[ci]
        if c[4] < len(pl["perm1"]):
            inv = {p: i for i, p in enumerate(pl["perm1"])}  # old position p moves to perm^-1(p)
            return NBID + cat * NCOMB + RANK[tuple(sorted(inv[p] for p in c))]
    return a


def action_table(words, pl):
    """[A_k(a) for a in 0..3225] as int32, computed per combo instead of per action (map_action, 12 categories
    at a time; tests/test_symmetry_host.py holds the two equal)."""
    t = np.arange(ASIZE, dtype=np.int32)
    phase = (int(words[0]) >> 4) & 1
    if phase == 0:
        if pl["swap"]:
            t[:NBID] = (t[:NBID] + LEVELS) % NBID
    else:
        n1 = len(pl["perm1"])
        inv = {p: i for i, p in enumerate(pl["perm1"])}
        ci = np.array([RANK[tuple(sorted(inv[p] for p in c))] if c[4] < n1 else i for i, c in enumerate(COMBOS)],
                      dtype=np.int32)
        t[NBID:] = (NBID + NCOMB * np.arange(12, dtype=np.int32)[:, None] + ci[None, :]).reshape(-1)
    return t


def augment(states, targets, indptr, cols, vals, seed, epoch_key, flags, index_base=0):
    """(states', targets', cols', vals') of rows i = example index_base + i; targets and the CSR may be None.
    A row's entries keep their values and are written in ascending new column order."""
    states = np.asarray(states, dtype=np.uint64).reshape(-1, 8)
    n = len(states)
    out_s = np.zeros_like(states)
    out_t = None if targets is None else np.zeros(n, dtype=np.int32)
    out_c = None if cols is None else np.array(cols, dtype=np.int32, copy=True)
    out_v = None if vals is None else np.array(vals, dtype=np.float64, copy=True)
    for i in range(n):
        pl = plan(states[i], index_base + i, epoch_key, seed, flags)
        out_s[i] = transform_state(states[i], pl)
        if targets is not None:
            out_t[i] = map_action(targets[i], states[i], pl)
        if cols is not None:
            a0, a1 = int(indptr[i]), int(indptr[i + 1])
            new = action_table(states[i], pl)[np.asarray(cols[a0:a1], dtype=np.int64)] if a1 > a0 else \
                np.zeros(0, dtype=np.int32)
            order = np.argsort(new, kind="stable")
            out_c[a0:a1] = new[order]
            out_v[a0:a1] = np.asarray(vals[a0:a1], dtype=np.float64)[order]
    return out_s, out_t, out_c, out_v


def flags_of(symmetries):
    f = 0
    for s in symmetries:
        f |= FLAG_OF[s]
    return f


# ------------------------------------------------------------------ hand-made states
def hand_states():
    """Packed states no self-play reaches together: carry lengths 0 / 5 / 10 for either player, rounds 1, 2
    and 13, both phases, pending bids none / one / both, a roll absent."""
    def player(carry, used=0, cats=(), bid=0):
        wa = _pack(carry) | (len(carry) << 40) | (used << 44)
        wb = sum(int(c) << (8 * i) for i, c in enumerate(cats[:8]))
        wc = sum(int(c) << (8 * i) for i, c in enumerate(cats[8:12])) | ((bid & M32) << 32)
        return [wa, wb, wc]

    def state(rnd, phase, ra, rb, b1, b2, p1, p2):
        w0 = rnd | (phase << 4) | ((1 << 5) if ra else 0) | ((1 << 6) if rb else 0) | (b1 << 8) | (b2 << 16)
        w0 |= (_pack(ra) << 24) | (_pack(rb) << 44)
        return [w0, *p1, *p2, 0]

    NONE = 0xFF
    A10, B16 = 10, 0x80 | 16  # (A, 5000), (B, 8000)
    d10, e10 = [1, 2, 3, 4, 5, 6, 6, 5, 3, 1], [2, 2, 4, 4, 6, 1, 3, 3, 5, 5]
    rA, rB = [1, 3, 3, 5, 6], [2, 2, 4, 6, 1]
    cats = (3, 0, 9, 0, 0, 0, 21, 0, 0, 15, 0, 0)
    S = [
        state(1, 0, rA, rB, NONE, NONE, player([]), player([])),                    # round 1, nothing pending
        state(1, 0, rA, rB, NONE, B16, player([]), player([])),                     # round 1, one pending
        state(2, 0, rA, rB, NONE, NONE, player(d10[:5]), player(e10[:5])),          # round 2 bid, 5 / 5
        state(2, 0, rA, rB, NONE, A10, player(d10[:5]), player(e10[:5], bid=-5000)),
        state(2, 0, rA, rB, A10, B16, player(d10[:5]), player(e10[:5])),            # both pending
        state(2, 0, rA, rB, B16, B16, player(d10[:5], bid=2500), player(e10[:5])),  # both, same group and amount
        state(2, 1, rA, rB, A10, B16, player(d10), player(e10)),                    # score, 10 / 10
        state(7, 1, rA, rB, A10, A10, player(d10, 0x045, cats, 1500), player(e10[:5], 0x245, cats, -1500)),
        state(7, 1, rA, rB, B16, A10, player(d10[:5], 0x045, cats), player(e10, 0x0C5, cats)),
        state(7, 0, rA, [], NONE, NONE, player(d10[:5], 0x045, cats), player(e10[:5], 0x0C5, cats)),  # rollB absent
        state(7, 0, [], rB, NONE, A10, player(d10[:5], 0x045, cats), player(e10[:5], 0x0C5, cats)),  # rollA absent
        state(12, 0, rA, rB, NONE, B16, player(d10[:5], 0x7FF, cats), player(e10[:5], 0x7FF, cats)),
        state(13, 1, rA, rB, NONE, NONE, player(d10, 0x3FF, cats), player(e10, 0x3FF, cats)),    # round 13, 10 / 10
        state(13, 1, rA, rB, NONE, NONE, player(d10[:5], 0x7FF, cats), player(e10, 0x3FF, cats)),  # 5 / 10
        state(13, 1, rA, rB, NONE, NONE, player([], 0xFFF, cats, 7000), player([], 0xFFF, cats)),  # ended, 0 / 0
        state(5, 1, rA, rB, A10, B16, player([]), player(e10)),                     # nothing valid: carry 0 / 10
        state(5, 1, rA, rB, A10, B16, player(d10), player([])),                     # 10 / 0
        state(6, 1, rA, rB, A10, B16, player(d10[:7], 0x111, cats), player(e10[:3], 0x111, cats)),  # lengths 7 / 3
    ]
    return np.array(S, dtype=np.uint64)
