"""Batched Game-plugin kernels on device tensors (thin layer over include/yacht_hip.h).

States are ``torch.int64[n, 8]`` CUDA tensors holding the packed uint64 words
(``state.pack``).  Every function enqueues on the current torch stream.  There is no CPU
path: CPU tensors are rejected.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

ACTION_SIZE = 3226
MASK_WORDS = 101
FEATURES = 59


def _dev(x, dtype):
    t = torch.as_tensor(x, dtype=dtype)
    if not t.is_cuda:
        t = t.to("cuda")
    return t.contiguous()


def states_to_device(words) -> torch.Tensor:
    """numpy uint64[n, 8] (or [8]) -> CUDA int64[n, 8]."""
    a = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1, 8))
    return torch.from_numpy(a.view(np.int64)).to("cuda")


def states_to_host(t: torch.Tensor) -> np.ndarray:
    return t.detach().to("cpu").contiguous().numpy().view(np.uint64).reshape(-1, 8)


def _bcast(x, n, dtype):
    t = _dev(x, dtype)
    if t.dim() == 0:
        t = t.expand(n)
    return t.reshape(n).contiguous()


def init_board(seed: int, env_ids, ctr):
    env = _dev(env_ids, torch.int32).reshape(-1)
    n = env.numel()
    c = _bcast(ctr, n, torch.int64).clone()
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    call("yk_init_board", ptr(out), ptr(c), ptr(env), seed & (2**64 - 1), n, stream_ptr())
    return out, c


def step(states, players, actions, seed: int, env_ids, ctr):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    ac = _bcast(actions, n, torch.int32)
    env = _bcast(env_ids, n, torch.int32)
    c = _bcast(ctr, n, torch.int64).clone()
    out = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    npl = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int8, device="cuda")
    call("yk_step", ptr(st), ptr(pl), ptr(ac), seed & (2**64 - 1), ptr(env), ptr(c), ptr(out), ptr(npl),
         ptr(status), n, stream_ptr())
    return out, npl, status, c


def valid_mask(states, players):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    mask = torch.zeros((n, MASK_WORDS), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    call("yk_valid_mask", ptr(st), ptr(pl), ptr(mask), ptr(cnt), n, stream_ptr())
    return mask, cnt


def unpack_mask(mask: torch.Tensor) -> torch.Tensor:
    """[n, 101] int32 bit words -> [n, 3226] uint8 (bit a & 31 of word a >> 5)."""
    bits = torch.arange(32, device=mask.device, dtype=torch.int32)
    dense = ((mask.unsqueeze(-1) >> bits) & 1).reshape(mask.shape[0], -1)[:, :ACTION_SIZE]
    return dense.to(torch.uint8)


def ended(states, players):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    r = torch.zeros(n, dtype=torch.float64, device="cuda")
    tot = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    call("yk_ended", ptr(st), ptr(pl), ptr(r), ptr(tot), n, stream_ptr())
    return r, tot


def score_utility(states, players, weight: float, scale: float):
    """The score-margin utility of each state seen from its player (yk_score_utility): states int64[n, 8]
    (or uint64 words), players +1 / -1 (a scalar is broadcast), weight w in [0, 1], scale c > 0 in game points ->
    (u float64[n], margin int32[n]).  u = (1 - w) * game_ended + w * x / (1 + |x|), x = player * margin / c; 0.0 for a
    state that is not terminal (its margin is still written).  ValueError for a bad weight or scale."""
    from .replay import check_score_knobs
    if weight is None or scale is None:
        raise ValueError("score_utility needs a weight and a scale")
    w, c = check_score_knobs(weight, scale)
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    m = torch.zeros(n, dtype=torch.int32, device="cuda")
    call("yk_score_utility", ptr(st), ptr(pl), n, w, c, ptr(u), ptr(m), stream_ptr())
    return u, m


def canonical(states, players):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    out = torch.empty_like(st)
    call("yk_canonical", ptr(st), ptr(pl), ptr(out), n, stream_ptr())
    return out


def score_table(states, players):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pl = _bcast(players, n, torch.int32)
    out = torch.empty((n, 12, 252), dtype=torch.int32, device="cuda")
    call("yk_score_table", ptr(st), ptr(pl), ptr(out), n, stream_ptr())
    return out


def score_dice(dice):
    d = _dev(dice, torch.int8).reshape(-1, 5)
    out = torch.empty((d.shape[0], 12), dtype=torch.int32, device="cuda")
    call("yk_score_dice", ptr(d), ptr(out), d.shape[0], stream_ptr())
    return out


def featurize(states):
    st = _dev(states, torch.int64).reshape(-1, 8)
    x = torch.empty((st.shape[0], FEATURES), dtype=torch.float32, device="cuda")
    call("yk_featurize", ptr(st), ptr(x), st.shape[0], stream_ptr())
    return x


def key_hash(states):
    st = _dev(states, torch.int64).reshape(-1, 8)
    out = torch.empty(st.shape[0], dtype=torch.int64, device="cuda")
    call("yk_key_hash", ptr(st), ptr(out), st.shape[0], stream_ptr())
    return out


def hash_prior(states):
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    pi = torch.empty((n, ACTION_SIZE), dtype=torch.float32, device="cuda")
    v = torch.empty(n, dtype=torch.float32, device="cuda")
    call("yk_hash_prior", ptr(st), ptr(pi), ptr(v), n, stream_ptr())
    return pi, v


def dirichlet_noise(seed: int, env_ids, moves, nvalid, alpha: float):
    """The self-play engine's root noise (yk_dirichlet_noise): float64[n, 3226], row i the Dirichlet(alpha)
    sample over nvalid[i] valid actions of game env_ids[i] at move moves[i], 0 past nvalid[i]."""
    # env ids are uint32 in the ABI (the engine takes any 32-bit env_base): through int64, the low 32 bits
    env = _dev(env_ids, torch.int64).reshape(-1)
    env = (((env & 0xFFFFFFFF) + 2**31) % 2**32 - 2**31).to(torch.int32).contiguous()
    n = env.numel()
    mv = _bcast(moves, n, torch.int32)
    nv = _bcast(nvalid, n, torch.int32)
    eta = torch.empty((n, ACTION_SIZE), dtype=torch.float64, device="cuda")
    call("yk_dirichlet_noise", seed & (2**64 - 1), ptr(env), ptr(mv), ptr(nv), float(alpha), ptr(eta), n,
         stream_ptr())
    return eta


SYMMETRIES = {"carry": 1, "rolls": 2, "groups": 4}  # YK_SYM_CARRY / YK_SYM_ROLLS / YK_SYM_GROUPS


def symmetry_flags(symmetries) -> int:
    """An iterable over {"carry", "rolls", "groups"} -> yk_examples_augment's flags.  An unknown name (or a
    bare string, which would iterate as letters) raises ValueError; touches no device."""
    if isinstance(symmetries, str):
        symmetries = (symmetries,)
    flags = 0
    for name in symmetries:
        if name not in SYMMETRIES:
            raise ValueError(f"unknown symmetry {name!r}: choose from {sorted(SYMMETRIES)}")
        flags |= SYMMETRIES[name]
    return flags


def check_policy_columns(policies):
    """ValueError unless every column of the CSR (pi_indptr, pi_cols, pi_vals) is an action, 0 .. 3225 - what
    yk_examples_augment requires of its rows.  One device reduction pair; synchronises."""
    cols = policies[1]
    if cols.numel():
        lo, hi = int(cols.min()), int(cols.max())
        if lo < 0 or hi >= ACTION_SIZE:
            raise ValueError(f"policy columns must lie in 0 .. {ACTION_SIZE - 1}, found {lo} .. {hi}")


def augment_examples(states, targets, policies, seed: int, epoch_key: int, symmetries, index_base: int = 0, out=None):
    """A random symmetry of every example (yk_examples_augment): row i is example
    index_base + i of the pool, drawn for (seed, epoch_key).  states int64[n, 8]; targets int32[n] or None;
    policies the device CSR (pi_indptr, pi_cols, pi_vals) of as_device_policies, the ExampleShard.policies
    dict, or None; symmetries an iterable over {"carry", "rolls", "groups"} (empty: a copy).  Returns device
    tensors (states', targets', policies'), policies' sharing pi_indptr with the input; `out` - an earlier
    return value for inputs of the same sizes - is written instead of new tensors.  Columns must be actions
    (check_policy_columns); the inputs are not modified."""
    flags = symmetry_flags(symmetries)
    st = _dev(states, torch.int64).reshape(-1, 8)
    n = st.shape[0]
    tg = None if targets is None else _dev(targets, torch.int32).reshape(n)
    if isinstance(policies, dict):
        policies = (policies["pi_indptr"], policies["pi_cols"], policies["pi_vals"])
    if policies is not None:
        indptr, cols, vals = policies
        if indptr.dtype != torch.int64 or cols.dtype != torch.int32 or vals.dtype != torch.float64:
            raise TypeError("policies: pi_indptr int64, pi_cols int32, pi_vals float64")
        if indptr.numel() != n + 1:
            raise ValueError(f"pi_indptr has {indptr.numel()} entries for {n} examples")
    o_st, o_tg, o_pol = out if out is not None else (None, None, None)
    if o_st is None:
        o_st = torch.empty_like(st)
    if tg is not None and o_tg is None:
        o_tg = torch.empty_like(tg)
    if policies is not None and o_pol is None:
        o_pol = (indptr, torch.empty_like(cols), torch.empty_like(vals))
    if o_st.shape != st.shape or (tg is not None and o_tg.shape != tg.shape) or \
            (policies is not None and (o_pol[1].shape != cols.shape or o_pol[2].shape != vals.shape)):
        raise ValueError("out does not match the inputs' sizes")
    csr = [None] * 5
    if policies is not None:
        # (an empty CSR's cols / vals may have no storage: any non-null pointer does, nothing reads it)
        csr = [ptr(indptr), ptr(cols) or ptr(indptr), ptr(vals) or ptr(indptr),
               ptr(o_pol[1]) or ptr(o_st), ptr(o_pol[2]) or ptr(o_st)]
    call("yk_examples_augment", ptr(st), None if tg is None else ptr(tg), csr[0], csr[1], csr[2], n,
         int(index_base), seed & (2**64 - 1), int(epoch_key) & 0xFFFFFFFF, flags, ptr(o_st),
         None if tg is None else ptr(o_tg), csr[3], csr[4], stream_ptr())
    return o_st, (o_tg if tg is not None else None), \
        ((indptr, o_pol[1], o_pol[2]) if policies is not None else None)


# ---------------------------------------------------------------- legal-move mask
LEGAL_KINDS = {1: "the state has no valid action", 2: "the hard target is not a valid action",
               3: "a policy entry with p > 0 sits on an invalid action"}


def check_legal(states, targets=None, policies=None, idx=None):
    """The contract of masked training over examples (yk_examples_check_legal): every row has a valid action,
    its hard target (targets int32[N], or None: not checked) is valid, and every entry with p > 0 of its policy
    row (the device CSR, or None: not checked) sits on a valid action.  idx int32[n]: the rows to check (all
    when None).  Returns (first_bad, kind): (-1, 0) when clean, else the lowest offending position and a key of
    LEGAL_KINDS.  Synchronises."""
    import ctypes as C
    st =_dev(states, torch.int64).reshape(-1, 8)
    n = int(idx.numel()) if idx is not None else st.shape[0]
    tg = None if targets is None else _dev(targets, torch.int32)
    csr = [None, None, None]
    if policies is not None:
        indptr, cols, vals = _csr(policies)
        csr = [ptr(indptr), ptr(cols) or ptr(indptr), ptr(vals) or ptr(indptr)]
    bad, kind = C.c_int64(-1), C.c_int(0)
    call("yk_examples_check_legal", ptr(st), None if tg is None else ptr(tg), *csr,
         None if idx is None else ptr(_dev(idx, torch.int32)), n, C.byref(bad), C.byref(kind), stream_ptr())
    return int(bad.value), int(kind.value)


# ---------------------------------------------------------------- weighted minibatch sampling
def sample_weights(rows, seg_lens, seg_factors, surprise: float):
    """Per-example sampling weights (yk_sample_weights): w[i] = seg_factors[segment of i] * s_i over the
    sum(seg_lens) pooled examples, segment s being the next seg_lens[s] of them (zeros allowed; 1 to 64
    segments, factors finite and >= 0).  rows: YkNet.evaluate(..., per_row=True)'s device float64 [n, >= 16]
    table, or None when surprise is 0 (then s_i = 1).  Returns (w float64[n] on the device, K) with K the
    summed policy KL the surprise term is normalised by.  Synchronises."""
    import ctypes as C
    lens = [int(x) for x in seg_lens]
    fac = [float(x) for x in seg_factors]
    if len(lens) != len(fac):
        raise ValueError(f"{len(lens)} segment lengths for {len(fac)} factors")
    n, nseg = sum(lens), len(lens)
    ld = 0
    if rows is not None:
        if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[0] != n:
            raise ValueError(f"rows must be float64[{n}, >= 16]")
        ld = int(rows.shape[1])
    seg_ptr = (C.c_int64 * (nseg + 1))(*np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).tolist())
    seg_fac = (C.c_double * max(nseg, 1))(*fac)
    w = torch.empty(max(n, 0), dtype=torch.float64, device="cuda")
    ksum = C.c_double()
    call("yk_sample_weights", None if rows is None else ptr(rows), ld, seg_ptr, seg_fac, nseg, float(surprise), n,
         ptr(w) if n > 0 else None, C.byref(ksum), stream_ptr())
    return w, float(ksum.value)


def sample_cdf(w):
    """The cumulative distribution of device float64 weights (yk_sample_cdf), nondecreasing, in an order fixed
    by their number: (cdf float64[n], total = cdf[-1]).  ValueError when a weight is negative or NaN or the
    total is not finite and positive.  Synchronises."""
    import ctypes as C
    if w.dtype != torch.float64 or w.dim() != 1:
        raise ValueError("w must be float64[n]")
    n = int(w.numel())
    cdf = torch.empty_like(w)
    total = C.c_double()
    try:
        call("yk_sample_cdf", ptr(w) if n else None, n, ptr(cdf) if n else None, C.byref(total), stream_ptr())
    except _lib.YkError as e:
        if e.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError("sampling weights must be >= 0 with a finite, positive total") from None
    return cdf, float(total.value)


def sample_draw(cdf, seed: int, key: int, first: int, m: int, out=None):
    """m draws with replacement from the distribution of sample_cdf's table (yk_sample_draw): int32[m] device
    indices, draw r being draw first + r of the stream (seed, key) - equal calls give equal indices, and a
    range of draws is that range of a longer call.  `out`: an int32 device tensor of at least m elements to
    write into (its first m are returned).  Asynchronous on the current stream."""
    if cdf.dtype != torch.float64 or cdf.dim() != 1:
        raise ValueError("cdf must be float64[n]")
    m = int(m)
    if out is None:
        out = torch.empty(max(m, 0), dtype=torch.int32, device="cuda")
    elif out.dtype != torch.int32 or out.dim() != 1 or out.numel() < m:
        raise ValueError(f"out must be int32 with at least {m} elements")
    n = int(cdf.numel())
    call("yk_sample_draw", ptr(cdf) if n else None, n, seed & (2**64 - 1), int(key) & 0xFFFFFFFF,
         int(first) & (2**64 - 1), m, ptr(out) if m > 0 else None, stream_ptr())
    return out[:m]


# ---------------------------------------------------------------- reanalysis
def reanalyse_select(n: int, seed: int, key: int, fraction: float, index_base: int = 0, count_only: bool = False):
    """Which of n examples a refresh reanalyses (yk_reanalyse_select): row i is example index_base + i of the
    window, chosen iff its Philox uniform for (seed, key) lies below `fraction`.  Returns the chosen rows as a
    device int32 tensor, ascending - or only their number with count_only.  Synchronises."""
    import ctypes as C
    n = int(n)
    args = (n, int(index_base) & (2**64 - 1), seed & (2**64 - 1), int(key) & 0xFFFFFFFF, float(fraction))
    m = C.c_int64()
    call("yk_reanalyse_select", *args, None, 0, C.byref(m), stream_ptr())
    if count_only:
        return int(m.value)
    idx = torch.empty(int(m.value), dtype=torch.int32, device="cuda")
    if m.value:
        call("yk_reanalyse_select", *args, ptr(idx), int(m.value), C.byref(m), stream_ptr())
    return idx


def _csr(policies):
    if isinstance(policies, dict):
        policies = (policies["pi_indptr"], policies["pi_cols"], policies["pi_vals"])
    indptr, cols, vals = policies
    if indptr.dtype != torch.int64 or cols.dtype != torch.int32 or vals.dtype != torch.float64:
        raise TypeError("policies: pi_indptr int64, pi_cols int32, pi_vals float64")
    if indptr.dim() != 1 or indptr.numel() < 1:
        raise ValueError("pi_indptr needs n + 1 entries")
    return indptr, cols, vals


def policies_from_counts(counts):
    """Root visit counts as policy rows (yk_policies_from_counts).  counts: device int32[n, 3226], what
    yk_mcts_search writes.  Returns ((pi_indptr, pi_cols, pi_vals), targets int32[n], n_empty): row r holds the
    actions with a positive count, ascending, with N / sum N in float64; targets[r] is the most visited action
    (the lowest on ties), -1 for the n_empty rows without a positive count.  Synchronises."""
    import ctypes as C
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != ACTION_SIZE:
        raise ValueError(f"counts must be int32[n, {ACTION_SIZE}]")
    n = int(counts.shape[0])
    indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    targets = torch.empty(n, dtype=torch.int32, device="cuda")
    nnz, empty = C.c_int64(), C.c_int64()
    cp, tp = (ptr(counts), ptr(targets)) if n else (None, None)
    call("yk_policies_from_counts", cp, n, ptr(indptr), None, None, 0, tp, C.byref(nnz), C.byref(empty), stream_ptr())
    k = int(nnz.value)
    cols = torch.empty(k, dtype=torch.int32, device="cuda")
    vals = torch.empty(k, dtype=torch.float64, device="cuda")
    if k:
        call("yk_policies_from_counts", cp, n, ptr(indptr), ptr(cols), ptr(vals), k, tp, C.byref(nnz), C.byref(empty),
             stream_ptr())
    return (indptr, cols, vals), targets, int(empty.value)


def policies_splice(policies, idx, new_policies):
    """Rows idx of a policy CSR replaced by the rows of another (yk_policies_splice): idx a device int32
    tensor, strictly ascending within the old CSR's rows; new row j becomes row idx[j] unless it is empty,
    then the old row stays.  Returns the new device CSR (pi_indptr, pi_cols, pi_vals); the inputs are not
    modified.  ValueError for an idx that is not strictly ascending or out of range.  Synchronises."""
    import ctypes as C
    indptr, cols, vals = _csr(policies)
    nip, ncols, nvals = _csr(new_policies)
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise TypeError("idx must be an int32 vector")
    n, m = int(indptr.numel()) - 1, int(idx.numel())
    if nip.numel() != m + 1:
        raise ValueError(f"the new CSR has {nip.numel() - 1} rows for {m} indices")
    out_ip = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64()
    # (an empty CSR's cols / vals may have no storage: any non-null pointer does, nothing reads it)
    src = (ptr(indptr), ptr(cols) or ptr(indptr), ptr(vals) or ptr(indptr), n, ptr(idx) if m else None, m,
           ptr(nip) if m else None, ptr(ncols) or ptr(nip), ptr(nvals) or ptr(nip))
    try:
        call("yk_policies_splice", *src, ptr(out_ip), None, None, 0, C.byref(nnz), stream_ptr())
        k = int(nnz.value)
        out_cols = torch.empty(k, dtype=torch.int32, device="cuda")
        out_vals = torch.empty(k, dtype=torch.float64, device="cuda")
        if k:
            call("yk_policies_splice", *src, ptr(out_ip), ptr(out_cols), ptr(out_vals), k, C.byref(nnz), stream_ptr())
    except _lib.YkError as e:
        if e.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError(f"idx must be strictly ascending within 0 .. {n - 1}") from None
    return out_ip, out_cols, out_vals


# ---------------------------------------------------------------- playout cap
def examples_full_rows(images, n_envs: int, max_moves: int, sims: int, n_games: int = -1, count_only: bool = False,
                       stream=None):
    """The examples of full moves in record images (yk_examples_full_rows): images a device uint8 tensor
    [R, nbytes] as examples_from_images takes it, the examples numbered as yk_examples_from_records numbers
    them with skip = 0.  Returns the numbers of the examples whose move was not a fast move of the playout
    cap as a device int32 tensor, ascending - or only their count with count_only.  Synchronises."""
    import ctypes as C
    imgs = images.reshape(images.shape[0] if images.dim() > 1 else 1, -1).contiguous()
    args = (ptr(imgs), int(imgs.shape[0]), int(n_envs), int(max_moves), int(sims), int(n_games))
    sp = stream_ptr(stream)
    m = C.c_int64()
    call("yk_examples_full_rows", *args, None, 0, C.byref(m), sp)
    if count_only:
        return int(m.value)
    idx = torch.empty(int(m.value), dtype=torch.int32, device="cuda")
    if m.value:
        call("yk_examples_full_rows", *args, ptr(idx), int(m.value), C.byref(m), sp)
    return idx


def policies_take(policies, idx):
    """Rows idx of a policy CSR (yk_policies_take): idx a device int32 tensor within the CSR's rows, in any
    order and with repeats; out row j is row idx[j] bit for bit.  Returns the device CSR (pi_indptr, pi_cols,
    pi_vals); the input is not modified.  ValueError for an index out of range.  Synchronises."""
    import ctypes as C
    indptr, cols, vals = _csr(policies)
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise TypeError("idx must be an int32 vector")
    n, m = int(indptr.numel()) - 1, int(idx.numel())
    out_ip = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64()
    # (an empty CSR's cols / vals may have no storage: any non-null pointer does, nothing reads it)
    src = (ptr(indptr), ptr(cols) or ptr(indptr), ptr(vals) or ptr(indptr), n, ptr(idx) if m else None, m)
    try:
        call("yk_policies_take", *src, ptr(out_ip), None, None, 0, C.byref(nnz), stream_ptr())
        k = int(nnz.value)
        out_cols = torch.empty(k, dtype=torch.int32, device="cuda")
        out_vals = torch.empty(k, dtype=torch.float64, device="cuda")
        if k:
            call("yk_policies_take", *src, ptr(out_ip), ptr(out_cols), ptr(out_vals), k, C.byref(nnz), stream_ptr())
    except _lib.YkError as e:
        if e.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError(f"idx must lie within 0 .. {n - 1}") from None
    return out_ip, out_cols, out_vals


# ---------------------------------------------------------------- policy target pruning
def policy_prune(indptr, cols, counts, q, p, ns, k: float, cpuct: float, stream=None):
    """Policy target pruning of rows of root counts (yk_policy_prune), the rule k_move_end applies after a forced
    move: device tensors indptr int64 [n + 1], and per entry cols int32 (the action), counts int32 (N), q
    float64 (Q), p float32 (P); ns int32 [n] (each row's root visit count); k the forced-playouts knob and cpuct
    the search's.  Returns the pruned counts as a new device int32 tensor; the best child of a row (the largest
    count, the lowest column among equals) keeps its count, k = 0 copies.  ValueError for row pointers that
    start below 0 or decrease.  Synchronises."""
    want = ((indptr, torch.int64), (cols, torch.int32), (counts, torch.int32), (q, torch.float64),
            (p, torch.float32), (ns, torch.int32))
    for t, dt in want:
        if t.dtype != dt or t.dim() != 1:
            raise TypeError("policy_prune takes vectors: indptr int64, cols / counts / ns int32, q float64, p float32")
    n = int(indptr.numel()) - 1
    if n < 0 or int(ns.numel()) != n or not (cols.numel() == counts.numel() == q.numel() == p.numel()):
        raise ValueError("policy_prune: indptr has n + 1 entries, ns n, and cols / counts / q / p one per edge")
    out = torch.empty_like(counts)
    # (an empty CSR's tensors may have no storage: any non-null pointer does, nothing is read or written there)
    spare = torch.empty(2, dtype=torch.int64, device="cuda")
    a = [ptr(t) or ptr(spare) for t in (cols, counts, q, p, ns)]
    try:
        call("yk_policy_prune", ptr(indptr), a[0], a[1], a[2], a[3], a[4], n, float(k), float(cpuct),
             ptr(out) or ptr(spare[1:]), stream_ptr(stream))
    except _lib.YkError as err:
        if err.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError("policy_prune: indptr must start at >= 0 and never decrease") from None
    return out


# ---------------------------------------------------------------- first-play urgency
def fpu_pick(indptr, p, counts, q, ns, cpuct: float, reduction: float, stream=None):
    """The UCB pick under first-play urgency of nodes given as a CSR (yk_fpu_pick), the rule of the search
    kernels' FPU instantiations: device tensors indptr int64 [n + 1], and per entry p float32 (P), counts int32
    (N; 0: an unvisited edge), q float64 (Q); ns int32 [n] (each node's visit count); cpuct the search's and
    reduction the rule's r.  Returns (pick, unvisited), device int32 [n]: the picked entry's index within its
    row (-1: an empty row) and 1 where that entry is an unvisited edge.  ValueError for row pointers that start
    below 0 or decrease.  Synchronises."""
    want = ((indptr, torch.int64), (p, torch.float32), (counts, torch.int32), (q, torch.float64), (ns, torch.int32))
    for t, dt in want:
        if t.dtype != dt or t.dim() != 1:
            raise TypeError("fpu_pick takes vectors: indptr int64, p float32, counts / ns int32, q float64")
    n = int(indptr.numel()) - 1
    if n < 0 or int(ns.numel()) != n or not (p.numel() == counts.numel() == q.numel()):
        raise ValueError("fpu_pick: indptr has n + 1 entries, ns n, and p / counts / q one per edge")
    pick = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    unv = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    # (an empty CSR's tensors may have no storage: any non-null pointer does, nothing is read or written there)
    spare = torch.empty(2, dtype=torch.int64, device="cuda")
    a = [ptr(t) or ptr(spare) for t in (p, counts, q, ns)]
    try:
        call("yk_fpu_pick", ptr(indptr), a[0], a[1], a[2], a[3], n, float(cpuct), float(reduction), ptr(pick), ptr(unv),
             stream_ptr(stream))
    except _lib.YkError as err:
        if err.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError("fpu_pick: indptr must start at >= 0 and never decrease") from None
    return pick[:n], unv[:n]


# ---------------------------------------------------------------- self-play temperatures
def temperature_schedule(early: float, final: float, halflife, n_moves: int):
    """yk_temperature_schedule: float64[n_moves], T(m) = final + (early - final) * 2 ** (-m / halflife) - the table
    an engine uploads, bit for bit the Python expression (early == final needs no halflife).  Host only."""
    out = np.zeros(max(int(n_moves), 1), dtype=np.float64)
    call("yk_temperature_schedule", float(early), float(final), float(halflife or 0.0), int(n_moves), out.ctypes.data)
    return out[:int(n_moves)]


def temperature_pick(indptr, counts, temps, u, stream=None):
    """The move draw from N ** (1 / T) on rows of visit counts given as a CSR (yk_temperature_pick), the device
    function k_move_end runs: device tensors indptr int64 [n + 1], counts int32 per entry, and per row temps
    float64 (T) and u float64 (the uniform).  Returns (pick, total): device int32 [n], the drawn entry's index
    within its row (-1: nothing to draw from), and float64 [n], the sum of the weights.  ValueError for row
    pointers that start below 0, decrease or reach past counts, or a T that is not finite and > 0.
    Synchronises."""
    want = ((indptr, torch.int64), (counts, torch.int32), (temps, torch.float64), (u, torch.float64))
    for t, dt in want:
        if t.dtype != dt or t.dim() != 1:
            raise TypeError("temperature_pick takes vectors: indptr int64, counts int32, temps / u float64")
    n = int(indptr.numel()) - 1
    if n < 0 or int(temps.numel()) != n or int(u.numel()) != n:
        raise ValueError("temperature_pick: indptr has n + 1 entries, temps and u n")
    if int(indptr[-1]) > int(counts.numel()):
        raise ValueError("temperature_pick: indptr reaches past counts")
    pick = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    total = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    spare = torch.empty(2, dtype=torch.int64, device="cuda")
    a = [ptr(t) or ptr(spare) for t in (counts, temps, u)]
    try:
        call("yk_temperature_pick", ptr(indptr), a[0], a[1], a[2], n, ptr(pick), ptr(total), stream_ptr(stream))
    except _lib.YkError as err:
        if err.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError("temperature_pick: indptr must start at >= 0 and never decrease, and every T must be "
                         "finite and > 0") from None
    return pick[:n], total[:n]


def root_temper(p, nvalid, temps, stream=None):
    """The root policy temperature on rows of compact priors (yk_root_temper), the device function k_root_noise
    runs: device tensors p float32 [n, 3226] (row i compact over its first nvalid[i] entries), nvalid int32 [n],
    temps float64 [n].  Returns float32 [n, 3226]: P' = f32(P ** (1 / T) / S) over those entries, 0 past them; a
    row at T == 1.0 exactly is copied.  ValueError for a T that is not finite and > 0.  Synchronises."""
    if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != ACTION_SIZE:
        raise TypeError(f"root_temper takes p float32 [n, {ACTION_SIZE}]")
    n = int(p.shape[0])
    if nvalid.dtype != torch.int32 or temps.dtype != torch.float64 or nvalid.shape != (n,) or temps.shape != (n,):
        raise TypeError("root_temper takes nvalid int32 [n] and temps float64 [n]")
    out = torch.empty_like(p)
    if n == 0:
        return out
    try:
        call("yk_root_temper", ptr(p), ptr(nvalid), ptr(temps), n, ptr(out), stream_ptr(stream))
    except _lib.YkError as err:
        if err.code != _lib.YK_ERR_RANGE:
            raise
        raise ValueError("root_temper: every T must be finite and > 0") from None
    return out


__all__ = ["states_to_device", "states_to_host", "init_board", "step", "valid_mask", "unpack_mask", "ended",
           "canonical", "score_table", "score_dice", "featurize", "key_hash", "hash_prior", "dirichlet_noise",
           "augment_examples", "symmetry_flags", "check_policy_columns", "SYMMETRIES", "sample_weights",
           "sample_cdf", "sample_draw", "reanalyse_select", "policies_from_counts", "policies_splice",
           "examples_full_rows", "policies_take", "policy_prune", "fpu_pick", "temperature_schedule",
           "temperature_pick", "root_temper", "score_utility", "_lib"]


def greedy_action(states):
    """GreedyYachtPlayer's heuristic on canonical boards: the action, or -1 where the player
    falls back to a random legal action (YachtPlayers.py:199-214)."""
    st = _dev(states, torch.int64).reshape(-1, 8)
    out = torch.empty(st.shape[0], dtype=torch.int32, device="cuda")
    call("yk_greedy_action", ptr(st), ptr(out), st.shape[0], stream_ptr())
    return out
