"""The replay buffer (Coach.py:84-101): self-play examples kept on the device.

Coach.learn keeps ``trainExamplesHistory``, one deque of ``(canonicalBoard, pi, v)`` per
iteration.  At config 5's scale (65536 games x 48 moves per iteration) those Python lists do
not fit (a dense pi is 3226 floats), and NNetWrapper.train only uses ``argmax(pi)`` of them
(NNet.py:145-146).  So an iteration's examples are an ``ExampleShard``: device arrays of
packed boards (64 B), argmax targets and float32 values, built by ``yk_examples_from_records``
straight from the (all-gathered) trajectory record images, plus the full visit policies as a
device CSR (``yk_examples_policies``) for the examples file (Coach.py:144-151), for code that
iterates the reference's tuples, and for training on them (``policy_target="visits"``:
``as_device_policies``).  The record images are not kept.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import deque

import numpy as np
import torch

from ._lib import YK_ERR_STATE, YK_OK, YkError, call, lib, stream_ptr
from .kernels import augment_examples  # (a random symmetry of every example; listed with the buffer's functions)
from .kernels import policies_from_counts, policies_splice, reanalyse_select  # (the reanalysis' device calls)
from .kernels import examples_full_rows, policies_take  # (the playout cap's: the full moves' examples)
from .kernels import policy_prune  # (policy target pruning on rows of counts)


def _vcap(max_moves: int, sims: int) -> int:
    return 2 * max_moves * max(sims, 32)


class ExampleShard:
    """One iteration's examples (``iterationTrainExamples``, Coach.py:86-90) on the device:
    ``states`` int64[n, 8] (packed canonical boards), ``targets`` int32[n] (argmax pi),
    ``values`` float32[n], and - when built from record images - ``policies``: the full visit
    policies as a device CSR (``pi_indptr`` int64[n+1], ``pi_cols`` int32, ``pi_vals`` float64,
    ``values64`` float64[n]; yk_examples_policies).  ``len`` and iteration behave like the
    reference's deque of ``(YachtState, pi list, v)`` tuples.

    ``values`` is what NNetWrapper.train fits the value head to.  By default it is the outcome z; built
    with ``value_mix`` / ``value_lambda`` it is the search-value target, and the shard
    also carries ``outcomes`` (z, float32) and ``root_values`` (each move's root value, float32).  The
    tuples, ``policies["values64"]`` and the examples files keep the reference's v, the outcome.

    ``n_searched`` (shards built from record images) is the number of moves the images hold for the shard's
    games, before the playout cap's filter (``full_only``) and the ``maxlen`` cut."""

    def __init__(self, states, targets, values, policies=None, outcomes=None, root_values=None):
        self.states, self.targets, self.values = states, targets, values
        self.policies = policies
        self.outcomes = values if outcomes is None else outcomes
        self.root_values = root_values
        self.n_searched = None
        self.reanalysis = None  # replay.reanalyse's report on the shard it returns: {"n", "n_empty", "chunks"}
        self._host = None

    def __len__(self):
        return int(self.targets.numel())

    def host(self) -> dict:
        """Host arrays of the shard with the full policies (float64 as MCTS.getActionProb returns
        them): states u64[n, 8], pi_indptr i64[n+1], pi_cols i32, pi_vals f64, values f64[n],
        targets i32[n].  One device-to-host copy of the compact arrays, cached."""
        if self._host is None:
            if self.policies is None:
                raise ValueError("this shard was not built from record images: it has no policies")
            P = self.policies
            self._host = dict(states=self.states.cpu().numpy().view(np.uint64), values=P["values64"].cpu().numpy(),
                              targets=self.targets.cpu().numpy(), pi_indptr=P["pi_indptr"].cpu().numpy(),
                              pi_cols=P["pi_cols"].cpu().numpy(), pi_vals=P["pi_vals"].cpu().numpy())
        return self._host

    def __iter__(self):
        from .state import ACTION_SIZE, unpack
        h = self.host()
        for k in range(len(self)):
            pi = [0.0] * ACTION_SIZE
            a0, a1 = int(h["pi_indptr"][k]), int(h["pi_indptr"][k + 1])
            for c, v in zip(h["pi_cols"][a0:a1], h["pi_vals"][a0:a1]):
                pi[int(c)] = float(v)
            yield unpack(h["states"][k]), pi, float(h["values"][k])

    def __getitem__(self, k):
        from .state import ACTION_SIZE, unpack
        h = self.host()
        k = range(len(self))[k]
        pi = [0.0] * ACTION_SIZE
        a0, a1 = int(h["pi_indptr"][k]), int(h["pi_indptr"][k + 1])
        for c, v in zip(h["pi_cols"][a0:a1], h["pi_vals"][a0:a1]):
            pi[int(c)] = float(v)
        return unpack(h["states"][k]), pi, float(h["values"][k])


def check_value_knobs(value_mix, value_lambda):
    """(beta, lambda) of the search-value targets as floats; ValueError unless both lie in [0, 1]."""
    beta, lam = float(value_mix), float(value_lambda)
    if not 0.0 <= beta <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"value_mix must lie in [0, 1], got {value_mix!r}")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"value_lambda must lie in [0, 1], got {value_lambda!r}")
    return beta, lam


def check_playout_knobs(playoutFastSims=None, playoutFullProb=None, numMCTSSims=None):
    """(fast_sims, full_prob) of the playout cap randomization as (int, float): playoutFastSims
    unset or 0 is off, else an int with 2 <= playoutFastSims <= numMCTSSims (one simulation on a fresh root
    leaves every visit count zero); playoutFullProb (default 1) in (0, 1] with the cap on - at 0 no move would
    be a training example.  ValueError otherwise, and for a playoutFullProb != 1 while the cap is off (it would
    silently do nothing)."""
    fast = 0 if playoutFastSims is None else playoutFastSims
    if isinstance(fast, bool) or not isinstance(fast, (int, np.integer)) or fast < 0:
        raise ValueError(f"playoutFastSims must be an int >= 2 (or 0 / unset: off), got {playoutFastSims!r}")
    p = float(1.0 if playoutFullProb is None else playoutFullProb)
    if not 0.0 <= p <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"playoutFullProb must lie in [0, 1], got {playoutFullProb!r}")
    fast = int(fast)
    if fast == 0:
        if p != 1.0:
            raise ValueError("playoutFullProb needs playoutFastSims: without a fast cap every move is searched in "
                             "full and the probability would do nothing")
        return 0, 1.0
    sims = numMCTSSims
    if sims is None or isinstance(sims, bool) or int(sims) != sims:
        raise ValueError(f"playoutFastSims needs numMCTSSims, got {numMCTSSims!r}")
    if not 2 <= fast <= int(sims):
        raise ValueError(f"playoutFastSims must lie in 2 .. numMCTSSims = {int(sims)}, got {playoutFastSims!r}")
    if p <= 0.0:
        raise ValueError("playoutFullProb must be > 0 with playoutFastSims set: no move would be searched in full, "
                         "and there would be no training examples")
    return fast, p


def check_sample_knobs(trainSteps=0, sampleRecency=1.0, sampleSurprise=0.0):
    """(T, gamma, sigma) of the weighted minibatch sampling as (int, float, float):
    trainSteps an int >= 0 (0: off - the epochs of full permutations), sampleRecency in (0, 1],
    sampleSurprise in [0, 1].  ValueError otherwise, and when gamma != 1 or sigma != 0 while the sampling
    is off (they would silently do nothing)."""
    if isinstance(trainSteps, bool) or int(trainSteps) != trainSteps or trainSteps < 0:
        raise ValueError(f"trainSteps must be an int >= 0, got {trainSteps!r}")
    T, gamma, sigma = int(trainSteps), float(sampleRecency), float(sampleSurprise)
    if not 0.0 < gamma <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"sampleRecency must lie in (0, 1], got {sampleRecency!r}")
    if not 0.0 <= sigma <= 1.0:
        raise ValueError(f"sampleSurprise must lie in [0, 1], got {sampleSurprise!r}")
    if T == 0 and (gamma != 1.0 or sigma != 0.0):
        raise ValueError("sampleRecency / sampleSurprise need trainSteps > 0: without it training runs "
                         "epochs of full permutations and the weights would do nothing")
    return T, gamma, sigma


def check_forced_knobs(forcedPlayoutsK=None, forcedPrune=None):
    """(k, prune) of the forced playouts and the policy target pruning as (float, bool):
    forcedPlayoutsK unset or 0 is off, else a finite number > 0 (KataGo uses 2); forcedPrune (default True)
    a bool - False forces without pruning the recorded counts, for ablation.  ValueError otherwise, and for
    forcedPrune=False while the forcing is off (it would silently do nothing)."""
    k = 0.0 if forcedPlayoutsK is None else forcedPlayoutsK
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise ValueError(f"forcedPlayoutsK must be a number >= 0 (0 / unset: off), got {forcedPlayoutsK!r}")
    k = float(k)
    if not 0.0 <= k < float("inf"):  # (a NaN fails the comparison)
        raise ValueError(f"forcedPlayoutsK must be finite and >= 0, got {forcedPlayoutsK!r}")
    prune = True if forcedPrune is None else forcedPrune
    if not isinstance(prune, (bool, np.bool_)):
        raise ValueError(f"forcedPrune must be a bool, got {forcedPrune!r}")
    if k == 0.0 and not prune:
        raise ValueError("forcedPrune=False needs forcedPlayoutsK > 0: without forced playouts nothing is pruned "
                         "anyway and the switch would do nothing")
    return k, bool(prune)


def check_fpu_knobs(fpuReduction=None, fpuRootReduction=None):
    """(reduction, root_reduction) of the first-play urgency as (float or None, float or None):
    fpuReduction unset is off - (None, None) - else a finite number >= 0 (0 is legal and is not off: unvisited
    edges then start at the parent's estimate); fpuRootReduction (default: fpuReduction) is the reduction at
    depth 0 of a search.  ValueError for anything else, and for fpuRootReduction without fpuReduction (it
    would silently do nothing)."""
    def number(name, x):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number >= 0 (unset: off), got {x!r}")
        x = float(x)
        if not (x >= 0.0) or math.isinf(x):
            raise ValueError(f"{name} must be finite and >= 0, got {x!r}")
        return x
    if fpuReduction is None:
        if fpuRootReduction is not None:
            raise ValueError("fpuRootReduction needs fpuReduction: without it first-play urgency is off and the "
                             "root reduction would silently do nothing")
        return None, None
    r = number("fpuReduction", fpuReduction)
    return r, (r if fpuRootReduction is None else number("fpuRootReduction", fpuRootReduction))


def fpu_knobs_of(args) -> dict:
    """args.fpuReduction / args.fpuRootReduction, checked, as SelfPlayEngine's keyword arguments - what everything
    that searches for a Coach passes to its engine, so a net trained on FPU searches is gated and played under
    them as well."""
    get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
    r, rr = check_fpu_knobs(get("fpuReduction", None), get("fpuRootReduction", None))
    return dict(fpu_reduction=r, fpu_root_reduction=rr)


def check_score_knobs(scoreUtility=None, scoreScale=None):
    """(weight, scale) of the score-margin utility as (float or None, float or None): both unset is
    off - (None, None) - else scoreUtility a number in [0, 1] (0 is legal and is not off: it gives the same values
    as off) and scoreScale a finite number > 0, in game points (a pip is 1000 points).  There is no default
    scale.  ValueError for anything else, for scoreScale without scoreUtility (alone it would silently do nothing)
    and for scoreUtility without scoreScale."""
    def number(name, x, what):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number {what} (unset: off), got {x!r}")
        return float(x)
    if scoreUtility is None:
        if scoreScale is not None:
            raise ValueError("scoreScale needs scoreUtility: without it the score-margin utility is off and the "
                             "scale would silently do nothing")
        return None, None
    w = number("scoreUtility", scoreUtility, "in [0, 1]")
    if not 0.0 <= w <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"scoreUtility must lie in [0, 1], got {scoreUtility!r}")
    if scoreScale is None:
        raise ValueError("scoreUtility needs scoreScale (game points, > 0): there is no default scale")
    c = number("scoreScale", scoreScale, "> 0")
    if not (c > 0.0) or math.isinf(c):
        raise ValueError(f"scoreScale must be finite and > 0, got {scoreScale!r}")
    return w, c


def score_knobs_of(args) -> dict:
    """args.scoreUtility / args.scoreScale, checked, as SelfPlayEngine's keyword arguments - what everything that
    searches for a Coach passes to its engine next to fpu_knobs_of, so the terminal values of every search are in
    the unit the value head was trained on."""
    get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
    w, c = check_score_knobs(get("scoreUtility", None), get("scoreScale", None))
    return dict(score_utility=w, score_scale=c)


MOVE_TEMPERATURE_RANGE = (0.05, 100.0)  # visit counts are 16-bit: 65535 ** 20 ~ 2e96 is finite in float64
ROOT_TEMPERATURE_RANGE = (0.25, 10.0)


def check_temperature_knobs(moveTemperature=None, moveTemperatureEarly=None, rootPolicyTemperature=None,
                            rootPolicyTemperatureEarly=None, temperatureHalflife=None) -> dict:
    """The self-play temperatures, checked, as SelfPlayEngine's keyword arguments.  Each schedule is
    T(m) = final + (early - final) * 2 ** (-m / halflife) over the real move m: moveTemperature (the final value,
    in [0.05, 100]; unset: off) draws a temp-1 move from N ** (1 / T), rootPolicyTemperature (in [0.25, 10];
    unset: off) searches the self-play root with P ** (1 / T) renormalised.  An Early defaults to its final
    value; temperatureHalflife (> 0, shared) is required when an Early differs from its final value.
    ValueError otherwise, and for an Early or a halflife without a final value (alone it would silently do
    nothing)."""
    def number(name, x, lo, hi):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number in [{lo}, {hi}] (unset: off), got {x!r}")
        x = float(x)
        if not lo <= x <= hi:  # (a NaN fails the comparison)
            raise ValueError(f"{name} must lie in [{lo}, {hi}], got {x!r}")
        return x

    def pair(name, final, early, rng):
        if final is None:
            if early is not None:
                raise ValueError(f"{name}Early needs {name}: without it the schedule is off and the early value "
                                 "would silently do nothing")
            return None, None
        f = number(name, final, *rng)
        return f, (f if early is None else number(name + "Early", early, *rng))

    mf, me = pair("moveTemperature", moveTemperature, moveTemperatureEarly, MOVE_TEMPERATURE_RANGE)
    rf, re_ = pair("rootPolicyTemperature", rootPolicyTemperature, rootPolicyTemperatureEarly, ROOT_TEMPERATURE_RANGE)
    h = temperatureHalflife
    if h is not None:
        if mf is None and rf is None:
            raise ValueError("temperatureHalflife needs moveTemperature or rootPolicyTemperature: without a "
                             "schedule it would silently do nothing")
        if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)):
            raise ValueError(f"temperatureHalflife must be a number > 0, got {h!r}")
        h = float(h)
        if not 0.0 < h < float("inf"):  # (a NaN fails the comparison)
            raise ValueError(f"temperatureHalflife must be finite and > 0, got {temperatureHalflife!r}")
    elif (mf is not None and me != mf) or (rf is not None and re_ != rf):
        raise ValueError("temperatureHalflife (> 0) is required when an Early temperature differs from its final "
                         "value")
    return dict(move_temperature=mf, move_temperature_early=me, root_policy_temperature=rf,
                root_policy_temperature_early=re_, temperature_halflife=h)


def temperature_knobs_of(args) -> dict:
    """args.moveTemperature / moveTemperatureEarly / rootPolicyTemperature / rootPolicyTemperatureEarly /
    temperatureHalflife, checked, as SelfPlayEngine's keyword arguments (self-play and the held-out games only:
    the arenas, the plugin and the reanalysis pass nothing)."""
    get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
    return check_temperature_knobs(get("moveTemperature", None), get("moveTemperatureEarly", None),
                                   get("rootPolicyTemperature", None), get("rootPolicyTemperatureEarly", None),
                                   get("temperatureHalflife", None))


def check_ema_knobs(emaDecay=0.0, emaEvery=1):
    """(decay, every) of the averaged weights as (float, int): emaDecay in [0, 1) (0 / unset:
    off - the net that plays is the raw iterate), emaEvery an int >= 1 (the shadow moves after every emaEvery-th
    optimiser apply).  ValueError otherwise, and for an emaEvery != 1 while the average is off (it would
    silently do nothing)."""
    decay = float(0.0 if emaDecay is None else emaDecay)
    if not 0.0 <= decay < 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"emaDecay must lie in [0, 1), got {emaDecay!r}")
    every = 1 if emaEvery is None else emaEvery
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"emaEvery must be an int >= 1, got {emaEvery!r}")
    if decay == 0.0 and every != 1:
        raise ValueError("emaEvery needs emaDecay > 0: without it no averaged weights are kept and the interval "
                         "would do nothing")
    return decay, int(every)


def check_mask_knobs(maskIllegal=False) -> bool:
    """args.maskIllegal of the legal-move mask as a bool: False / unset - the policy loss is
    the reference's, a softmax over all 3226 actions - or True - over each example's valid actions only.
    ValueError for anything that is not a bool (1, "yes" and the like would silently pick a side)."""
    if maskIllegal is None:
        return False
    if not isinstance(maskIllegal, (bool, np.bool_)):
        raise ValueError(f"maskIllegal must be a bool, got {maskIllegal!r}")
    return bool(maskIllegal)


def sample_rounds(trainSteps: int, epochs: int):
    """The trainSteps sampled steps split over `epochs` rounds: [(first step, one past the last)] per round,
    round e = floor(e T / E) .. floor((e + 1) T / E) - 1; empty rounds (T < E) have first == past."""
    T, E = int(trainSteps), int(epochs)
    return [(e * T // E, (e + 1) * T // E) for e in range(E)]


def _count_examples(x) -> int:
    if isinstance(x, ExampleShard):
        return len(x)
    items = list(x)
    if not items or _is_example(items[0]):
        return len(items)
    return sum(_count_examples(y) for y in items)


def sample_segments(examples, gamma: float = 1.0):
    """The sampling segments of what NNetWrapper.train takes, in as_device_examples' row order:
    (lengths, factors).  A list of shards or lists (trainExamplesHistory) gives one segment per non-empty
    item, item j of J weighing gamma ** (J - 1 - j) - the last iteration has age 0; anything else is one
    segment of factor 1."""
    if not isinstance(examples, ExampleShard):
        items = list(examples)
        if items and not _is_example(items[0]):
            lens = [_count_examples(x) for x in items]
            J = len(items)
            segs = [(n, float(gamma) ** (J - 1 - j)) for j, n in enumerate(lens) if n]
            if len(segs) > 64:
                raise ValueError(f"the weighted sampling takes at most 64 non-empty history items, got {len(segs)}")
            if segs:
                return [n for n, _ in segs], [f for _, f in segs]
            return [0], [1.0]
        return [len(items)], [1.0]
    return [len(examples)], [1.0]


def examples_from_images(images: torch.Tensor, n_envs: int, max_moves: int, sims: int, n_games: int = -1,
                         maxlen: int = None, stream=None, value_mix: float = 0.0,
                         value_lambda: float = 1.0, full_only: bool = False, score_utility=None,
                         score_scale=None) -> ExampleShard:
    """Record images (device uint8 [R, nbytes]: every rank's yk_engine_pack_records after the
    all-gather) -> ExampleShard of the first n_games games, keeping the last `maxlen` examples
    (the maxlenOfQueue deque, Coach.py:86-90).  The shard holds only compact arrays (examples and
    the policies' CSR, about a third of the images' bytes); the images can be released.

    value_mix (beta) and value_lambda (lambda), off at (0, 1): the shard's ``values`` become the
    search-value targets of yk_examples_value_targets - the outcome bootstrapped from the later moves' root
    values (lambda < 1) and mixed with the move's own (beta > 0); the images must then come from engines
    created with record_root_values.  ``outcomes`` and the tuples keep z.

    full_only (the playout cap): only the examples of full moves are kept.  Every array is first
    built for all moves - the value targets must see whole games - then the rows yk_examples_full_rows names
    are taken, and the last `maxlen` of those kept: maxlen counts training examples.  ``n_searched`` of the
    shard is the number of moves before the filter.

    score_utility (w) and score_scale (c), the score-margin utility (None: off): the shard's
    ``values`` come from yk_examples_utility_targets - wherever the formulas above read the outcome they read
    (1 - w) * outcome + w * g, g the squashed final margin of the game's final board in the images - also at
    (value_mix, value_lambda) = (0, 1), where no root value is needed.  ``outcomes`` and the tuples keep z."""
    beta, lam = check_value_knobs(value_mix, value_lambda)
    su, sc = check_score_knobs(score_utility, score_scale)
    if full_only:
        every = examples_from_images(images, n_envs, max_moves, sims, n_games=n_games, maxlen=None, stream=stream,
                                     value_mix=beta, value_lambda=lam, score_utility=su, score_scale=sc)
        idx = examples_full_rows(images, n_envs, max_moves, sims, n_games=n_games, stream=stream)
        if maxlen is not None:
            idx = idx[max(int(idx.numel()) - max(int(maxlen), 0), 0):].contiguous()
        return _take_rows(every, idx)
    imgs = images.reshape(images.shape[0] if images.dim() > 1 else 1, -1).contiguous()
    R = imgs.shape[0]
    cnt = C.c_int64()
    sp = stream_ptr(stream)
    call("yk_examples_from_records", imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, 0, 0, None, None, None,
         C.byref(cnt), sp)
    total = int(cnt.value)
    skip = max(total - int(maxlen), 0) if maxlen is not None else 0
    n = total - skip
    states = torch.empty((max(n, 1), 8), dtype=torch.int64, device="cuda")
    targets = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    values = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    call("yk_examples_from_records", imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, skip, n,
         states.data_ptr(), targets.data_ptr(), values.data_ptr(), C.byref(cnt), sp)
    if int(cnt.value) != n:
        raise RuntimeError(f"yk_examples_from_records wrote {cnt.value} examples, expected {n}")
    indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64()
    call("yk_examples_policies", imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, skip, n, indptr.data_ptr(),
         None, None, 0, None, C.byref(nnz), sp)
    k = int(nnz.value)
    cols = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
    vals = torch.empty(max(k, 1), dtype=torch.float64, device="cuda")
    v64 = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    call("yk_examples_policies", imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, skip, n, indptr.data_ptr(),
         cols.data_ptr(), vals.data_ptr(), k, v64.data_ptr(), C.byref(nnz), sp)
    pol = dict(pi_indptr=indptr, pi_cols=cols[:k], pi_vals=vals[:k], values64=v64[:n])
    if (beta, lam) == (0.0, 1.0) and su is None:
        shard = ExampleShard(states[:n], targets[:n], values[:n], policies=pol)
        shard.n_searched = total
        return shard
    tgt = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    rootv = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    missing = C.c_int64()
    if su is None:
        fn = "yk_examples_value_targets"
        rc = lib().yk_examples_value_targets(imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, skip, n, beta, lam,
                                             tgt.data_ptr(), rootv.data_ptr(), C.byref(missing), sp)
    else:  # the same kernel reading the utility for the outcome
        fn = "yk_examples_utility_targets"
        rc = lib().yk_examples_utility_targets(imgs.data_ptr(), R, n_envs, max_moves, sims, n_games, skip, n, beta, lam,
                                               su, sc, tgt.data_ptr(), rootv.data_ptr(), C.byref(missing), sp)
    if rc == YK_ERR_STATE and missing.value > 0:
        raise ValueError(f"{missing.value} of {n} examples need a root value the record images do not hold: "
                         "value_mix / value_lambda need engines created with record_root_values=True")
    if rc != YK_OK:
        raise YkError(fn, rc)
    # (at (0, 1) the images need no root values: the shard then carries none)
    shard = ExampleShard(states[:n], targets[:n], tgt[:n], policies=pol, outcomes=values[:n],
                         root_values=None if (beta, lam) == (0.0, 1.0) else rootv[:n])
    shard.n_searched = total
    return shard


def _take_rows(shard: ExampleShard, idx: torch.Tensor) -> ExampleShard:
    """Rows idx (device int32, within the shard) of a shard with policies as a new shard: the fixed-width
    columns by torch indexing, the policy CSR by yk_policies_take.  n_searched is carried over."""
    rows = idx.to(torch.int64)
    P = shard.policies
    ip, cols, vals = policies_take((P["pi_indptr"], P["pi_cols"], P["pi_vals"]), idx)
    pol = dict(pi_indptr=ip, pi_cols=cols, pi_vals=vals, values64=P["values64"].index_select(0, rows))
    values = shard.values.index_select(0, rows)
    same = shard.outcomes is shard.values
    out = ExampleShard(shard.states.index_select(0, rows), shard.targets.index_select(0, rows), values, policies=pol,
                       outcomes=None if same else shard.outcomes.index_select(0, rows),
                       root_values=None if shard.root_values is None else shard.root_values.index_select(0, rows))
    out.n_searched = shard.n_searched
    return out


# ---------------------------------------------------------------- reanalysis
def check_reanalyse_knobs(reanalyseFraction=0.0, reanalyseSims=None, numMCTSSims=None):
    """(fraction, sims) of the reanalysis as (float, int): reanalyseFraction in [0, 1] (0: off),
    reanalyseSims an int >= 2 (default numMCTSSims; checked only when the reanalysis is on - the first
    simulation on a fresh tree only expands the root, so one simulation leaves every count zero).
    ValueError otherwise."""
    f = float(0.0 if reanalyseFraction is None else reanalyseFraction)
    if not 0.0 <= f <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"reanalyseFraction must lie in [0, 1], got {reanalyseFraction!r}")
    sims = numMCTSSims if reanalyseSims is None else reanalyseSims
    if reanalyseSims is not None or f > 0.0:
        if sims is None or isinstance(sims, bool) or int(sims) != sims or int(sims) < 2:
            raise ValueError(f"reanalyseSims must be an int >= 2, got {sims!r}")
    return f, (int(sims) if sims is not None else 0)


def reanalyse(shard: ExampleShard, idx, *, net=None, prior: str = "net", sims: int, cpuct: float, seed: int,
              env_base: int = 0, chunk: int = 4096, env_ids=None, ctr=None, fpu_reduction=None,
              fpu_root_reduction=None, score_utility=None, score_scale=None) -> ExampleShard:
    """Examples idx of a shard searched again (MuZero's reanalyse): their boards are the roots
    of `sims` simulations of yk_mcts_search on fresh trees with `net` (a YkNet, or a wrapper with yk_net();
    prior="hash": the test prior), and their policy rows and targets become the new search's.

    idx: a device int32 tensor, strictly ascending within the shard.  The roots are searched E = min(len(idx),
    chunk) at a time on one SelfPlayEngine(E, sims, cpuct, max_moves=1), the trees reset before every chunk.
    Root j draws from the game stream (seed, env_base + j) from counter 0 - or from env_ids[j] / ctr[j] where
    given.  The last, partial chunk is padded with copies of its first root on the stream ids after the
    call's last one; their searches are dropped (they consume nothing: a stream is a function of its id).
    No root noise is ever added.  fpu_reduction / fpu_root_reduction: the searches run under first-play urgency
    (SelfPlayEngine's knobs; None: off).  score_utility / score_scale: their terminal values are the
    score-margin utility (None: off).

    A reanalysed row holds the visit distribution N / sum N of its new search and its target the most visited
    action (the lowest on ties) - also where the stored row was the one-hot of a temp-0 move, so afterwards
    the examples file no longer holds the reference's tuple for those rows.  A row whose search left no visit
    keeps its old policy and target; `reanalysis["n_empty"]` of the returned shard counts them.

    Returns a new ExampleShard (shards are immutable; host() caches): `policies` the spliced CSR with the
    same values64, `targets` a copy with the reanalysed rows replaced; states, values, outcomes and
    root_values are the input's tensors - the value targets keep the original search's numbers.  Its
    `reanalysis` is {"n": len(idx), "n_empty": ..., "chunks": ...}.  ValueError for a shard without policies,
    sims < 2 or a bad idx; an engine error raises YkError."""
    from . import kernels as K
    from .engine import SelfPlayEngine
    if shard.policies is None:
        raise ValueError("reanalyse needs the shard's policies (policies=None): build it with examples_from_images")
    if isinstance(sims, bool) or int(sims) != sims or int(sims) < 2:
        raise ValueError(f"sims must be an int >= 2 (one simulation on a fresh tree only expands the root), got {sims!r}")
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk!r}")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_cuda:
        raise TypeError("idx must be a device int32 vector")
    n, m = len(shard), int(idx.numel())
    P = shard.policies

    def result(pol, targets, n_empty, chunks):
        out = ExampleShard(shard.states, targets, shard.values, policies=pol, outcomes=shard.outcomes,
                           root_values=shard.root_values)
        out.n_searched = shard.n_searched
        out.reanalysis = dict(n=m, n_empty=n_empty, chunks=chunks)
        return out
    if m == 0:
        return result(dict(P), shard.targets.clone(), 0, 0)
    # (checked before the gather below indexes with it; yk_policies_splice checks the same on the device)
    if int(idx.min()) < 0 or int(idx.max()) >= n or (m > 1 and not bool((idx[1:] > idx[:-1]).all())):
        raise ValueError(f"idx must be strictly ascending within 0 .. {n - 1}")
    if hasattr(net, "yk_net") and prior == "net":
        prior = "hash" if getattr(net, "yk_prior", None) == "hash" else "net"
        net = None if prior == "hash" else net.yk_net()
    rows = idx.to(torch.int64)
    roots = shard.states.index_select(0, rows).contiguous()
    E = min(m, int(chunk))
    pad = (-m) % E
    if env_ids is None:
        env = np.arange(m + pad, dtype=np.uint64) + np.uint64(int(env_base) & 0xFFFFFFFF)
    else:
        env = np.asarray(torch.as_tensor(env_ids).cpu().numpy(), dtype=np.int64).astype(np.uint64).reshape(-1)
        if env.size != m:
            raise ValueError(f"env_ids has {env.size} entries for {m} roots")
        env = np.concatenate([env, (env[-1] & np.uint64(0xFFFFFFFF)) + np.uint64(1) + np.arange(pad, dtype=np.uint64)])
    env = torch.from_numpy((env & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).to("cuda")
    c0 = torch.zeros(m + pad, dtype=torch.int64, device="cuda")
    if ctr is not None:
        c_in = torch.as_tensor(ctr).to(device="cuda", dtype=torch.int64).reshape(-1)
        if c_in.numel() != m:
            raise ValueError(f"ctr has {c_in.numel()} entries for {m} roots")
        c0[:m] = c_in
    sp = stream_ptr()
    counts = torch.empty((E, K.ACTION_SIZE), dtype=torch.int32, device="cuda")
    eng = SelfPlayEngine(E, int(sims), float(cpuct), net=net, prior=prior, max_moves=1, fpu_reduction=fpu_reduction,
                         fpu_root_reduction=fpu_root_reduction, score_utility=score_utility, score_scale=score_scale)
    parts, tparts, n_empty, chunks = [], [], 0, 0
    try:
        for j0 in range(0, m, E):
            k = min(E, m - j0)
            r = roots[j0:j0 + k]
            if k < E:  # the padding: copies of the chunk's first root
                r = torch.cat([r, r[:1].expand(E - k, 8)]).contiguous()
            # the roots of a chunk are unrelated to the last chunk's, and a tree refuses a root of a lower round
            call("yk_mcts_reset", eng.handle)
            try:
                call("yk_mcts_search", eng.handle, r.data_ptr(), seed & (2**64 - 1), env[j0:j0 + E].data_ptr(),
                     c0[j0:j0 + E].data_ptr(), int(sims), counts.data_ptr(), sp)
            except YkError as e:
                st = eng.stats()
                bits = [b_name for b, b_name in eng.ERROR_BITS.items() if st["errors"] & b]
                raise YkError(f"yk_mcts_search [reanalysis chunk at root {j0}: {', '.join(bits)}; stats {st}]",
                              e.code) from None
            pol, tg, ne = K.policies_from_counts(counts[:k])
            parts.append(pol)
            tparts.append(tg)
            n_empty += ne
            chunks += 1
    finally:
        eng.close()
    new = _cat_csr(parts, torch) if len(parts) > 1 else parts[0]
    if new is None:  # (no chunk has rows: cannot happen with m > 0)
        new = parts[0]
    out_ip, out_cols, out_vals = K.policies_splice((P["pi_indptr"], P["pi_cols"], P["pi_vals"]), idx, new)
    t_new = torch.cat(tparts) if len(tparts) > 1 else tparts[0]
    targets = shard.targets.clone()
    keep = t_new >= 0
    targets[rows[keep]] = t_new[keep]
    pol = dict(P, pi_indptr=out_ip, pi_cols=out_cols, pi_vals=out_vals)
    return result(pol, targets, n_empty, chunks)


# ---------------------------------------------------------------- what NNetWrapper.train takes
def _is_example(x) -> bool:
    return isinstance(x, tuple) and len(x) == 3 and not isinstance(x[0], (ExampleShard, list, deque))


def as_device_examples(examples, outcomes=False):
    """examples: an ExampleShard, a list of (board, pi, v) tuples (Coach.py:72), or a list of
    either (trainExamplesHistory) -> device (states int64[n, 8], targets int32[n], values f32[n]).
    outcomes: a shard gives its ``outcomes`` (z) instead of its ``values`` (the training target, which
    the value knobs may have changed) - what NNetWrapper.evaluate measures against; tuples carry z anyway."""
    from .train import examples_to_device
    if isinstance(examples, ExampleShard):
        return examples.states, examples.targets, examples.outcomes if outcomes else examples.values
    items = list(examples)
    if not items or _is_example(items[0]):
        if not items:
            return (torch.zeros((0, 8), dtype=torch.int64, device="cuda"),
                    torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float32, device="cuda"))
        return examples_to_device(items)
    parts = [as_device_examples(x, outcomes) for x in items]
    parts = [p for p in parts if p[1].numel()]
    if not parts:
        return as_device_examples([])
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


# ---------------------------------------------------------------- the full policies (policy_target="visits")
def _no_policies():
    return ValueError('policy_target="visits" needs the full policies, and this ExampleShard has none '
                      "(policies=None): build it with examples_from_images, or train with policy_target=\"argmax\"")


def _tuples_csr_host(items):
    """[(board, pi, v)] with dense pi -> (indptr int64[n+1], cols int32, vals float64): the nonzero
    entries of every pi, columns ascending (what yk_examples_policies writes for the same rows)."""
    indptr = np.zeros(len(items) + 1, dtype=np.int64)
    cols, vals = [], []
    for k0 in range(0, len(items), 1024):  # (a dense row is 25 KB: a chunk at a time)
        dense = np.asarray([np.asarray(p, dtype=np.float64) for _, p, _ in items[k0:k0 + 1024]], dtype=np.float64)
        dense = dense.reshape(len(dense), -1)
        r, c = np.nonzero(dense)  # row-major: ascending columns within a row
        indptr[k0 + 1:k0 + 1 + len(dense)] = np.bincount(r, minlength=len(dense))
        cols.append(c.astype(np.int32))
        vals.append(dense[r, c])
    np.cumsum(indptr, out=indptr)
    return (indptr, np.concatenate(cols) if cols else np.zeros(0, dtype=np.int32),
            np.concatenate(vals) if vals else np.zeros(0, dtype=np.float64))


def _cat_csr(parts, xp):
    """CSR row blocks -> one CSR: indptr concatenated with each block's entry offset."""
    parts = [p for p in parts if p[0].shape[0] > 1]  # (as as_device_examples drops empty blocks)
    if not parts:
        return None
    if len(parts) == 1:
        return parts[0]
    indptr, off = [parts[0][0][:1] * 0], 0
    for ip, _, _ in parts:
        indptr.append(ip[1:] + (off - int(ip[0])))
        off += int(ip[-1]) - int(ip[0])
    if xp is np:
        return np.concatenate(indptr), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    return torch.cat(indptr), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def policies_csr_host(examples):
    """The full policies of `examples` - an ExampleShard, a list of (board, pi, v) tuples (what
    load_examples / load_reference_examples return), or a list of either (trainExamplesHistory) -
    as host CSR arrays (pi_indptr int64[n+1], pi_cols int32, pi_vals float64), for the rows
    as_device_examples returns, in its order.  Tuple lists need no GPU."""
    if isinstance(examples, ExampleShard):
        if examples.policies is None:
            raise _no_policies()
        h = examples.host()
        return h["pi_indptr"], h["pi_cols"], h["pi_vals"]
    items = list(examples)
    if not items or _is_example(items[0]):
        return _tuples_csr_host(items)
    out = _cat_csr([policies_csr_host(x) for x in items], np)
    return out if out is not None else _tuples_csr_host([])


def as_device_policies(examples):
    """policies_csr_host on the device: (pi_indptr, pi_cols, pi_vals) tensors, the soft targets
    Trainer.step(..., policies=) takes.  A shard's CSR is used where it lies (no copy)."""
    if isinstance(examples, ExampleShard):
        if examples.policies is None:
            raise _no_policies()
        P = examples.policies
        return P["pi_indptr"], P["pi_cols"], P["pi_vals"]
    items = list(examples)
    if not items or _is_example(items[0]):
        return tuple(torch.from_numpy(a).to("cuda") for a in _tuples_csr_host(items))
    out = _cat_csr([as_device_policies(x) for x in items], torch)
    return out if out is not None else as_device_policies([])


__all__ = ["ExampleShard", "examples_from_images", "as_device_examples", "as_device_policies", "policies_csr_host",
           "augment_examples", "check_playout_knobs", "check_forced_knobs", "check_fpu_knobs", "fpu_knobs_of", "check_score_knobs", "score_knobs_of", "policy_prune", "examples_full_rows", "policies_take", "check_sample_knobs", "check_ema_knobs", "sample_rounds", "sample_segments", "check_reanalyse_knobs",
           "reanalyse", "reanalyse_select", "policies_from_counts", "policies_splice"]
