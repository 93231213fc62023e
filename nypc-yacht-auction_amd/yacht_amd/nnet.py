"""YachtNNet weights (torch) + NNetWrapper.predict / train on the MI355X.

``YachtNNet`` repeats the reference architecture (yacht/pytorch/YachtNNet.py:8-70) so its
``state_dict`` names and initialisation match; torch only holds the weights.  Inference
(``NNetWrapper.predict``, NNet.py:177-195) runs through ``yk_net_predict`` - featurize,
13 dense layers, both heads and exp(log_softmax) on the GPU; ``NNetWrapper.train``
(NNet.py:118-174) through the native trainer (train.py, yk_trainer_*); ``NNetWrapper.evaluate`` (not in
the reference: a forward without dropout and float64 metrics over its logits) through ``yk_net_evaluate``.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from ._lib import call, lib, ptr, stream_ptr
from .state import ACTION_SIZE, pack
from .utils import dotdict

DEFAULT_ARGS = dotdict(dict(lr=2e-3, weight_decay=1e-4, epochs=15, batch_size=512, vloss_weight=1.5,
                            cuda=True, hidden=256, nblocks=6, dropout=0.3))  # main.py:31-42


class ResidualBlock(nn.Module):  # YachtNNet.py:8-21
    def __init__(self, dim, dropout=0.2):
        super().__init__()
        self.fc1 = nn.Linear(dim, dim)
        self.ln1 = nn.LayerNorm(dim)
        self.fc2 = nn.Linear(dim, dim)
        self.ln2 = nn.LayerNorm(dim)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        h = self.ln1(F.silu(self.fc1(x)))
        h = self.dropout(h)
        h = self.ln2(F.silu(self.fc2(h)))
        return x + h


class YachtNNet(nn.Module):  # YachtNNet.py:24-70
    def __init__(self, input_len=59, action_size=ACTION_SIZE, hidden=256, nblocks=6, dropout=0.3,
                 kaiming_init=True):
        """kaiming_init=False keeps torch's default Linear init, as the submission bot's copy of
        the class does (agent.py:30-67)."""
        super().__init__()
        self.input_len, self.action_size = input_len, action_size
        self.inp = nn.Sequential(nn.Linear(input_len, hidden), nn.LayerNorm(hidden), nn.SiLU(), nn.Dropout(dropout))
        self.blocks = nn.ModuleList([ResidualBlock(hidden, dropout) for _ in range(nblocks)])
        self.pi_head = nn.Sequential(nn.LayerNorm(hidden), nn.SiLU(), nn.Linear(hidden, action_size))
        self.v_head = nn.Sequential(nn.LayerNorm(hidden), nn.SiLU(), nn.Linear(hidden, 128), nn.SiLU(),
                                    nn.Linear(128, 1))
        for m in self.modules() if kaiming_init else ():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight, nonlinearity="relu")
                nn.init.zeros_(m.bias)

    def forward(self, x):
        if x.ndim == 3:
            x = x.squeeze(1)
        h = self.inp(x)
        for blk in self.blocks:
            h = blk(h)
        return self.pi_head(h), torch.tanh(self.v_head(h))


PRECISIONS = {"f32": 0, "f16": 1}  # YK_PREDICT_F32 / YK_PREDICT_F16 (include/yacht_hip.h)
PI_LD = 3264    # row stride of the raw logits (yk_net_logits): 3226 padded to 204 tiles of 16 columns
EVAL_COLS = 16  # YK_EVAL_COLS: the per-example columns of yk_examples_metrics / yk_net_evaluate


def check_eval_args(states, targets, values, policies, idx, chunk):
    """The shapes and dtypes YkNet.evaluate takes, checked before anything touches the device
    (ValueError); returns the policies' CSR as a 3-tuple with non-empty arrays, or None."""
    N = states.shape[0]
    if states.dtype != torch.int64 or states.dim() != 2 or states.shape[1] != 8:
        raise ValueError("states must be int64[N, 8] (packed boards)")
    if targets.dtype != torch.int32 or tuple(targets.shape) != (N,):
        raise ValueError("targets must be int32[N]")
    if values.dtype != torch.float32 or tuple(values.shape) != (N,):
        raise ValueError("values must be float32[N]")
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1):
        raise ValueError("idx must be int32[n]")
    if int(chunk) != chunk or chunk >= 2 ** 31:
        raise ValueError(f"chunk must be an int (0: the default), got {chunk!r}")
    if policies is None:
        return None
    if len(policies) != 3:
        raise ValueError("policies must be (pi_indptr, pi_cols, pi_vals)")
    indptr, cols, vals = policies
    if indptr.dtype != torch.int64 or tuple(indptr.shape) != (N + 1,):
        raise ValueError("pi_indptr must be int64[N + 1]")
    if cols.dtype != torch.int32 or vals.dtype != torch.float64 or cols.shape != vals.shape or cols.dim() != 1:
        raise ValueError("pi_cols must be int32[nnz] and pi_vals float64[nnz]")
    if cols.numel() == 0:  # (no entries at all: the call still wants three pointers)
        cols, vals = cols.new_zeros(1), vals.new_zeros(1)
    return indptr, cols, vals


def eval_summary(sums, soft: bool) -> dict:
    """The 16 column sums of yk_net_evaluate (include/yacht_hip.h) -> plain numbers: every mean is
    sums[c] / n (NaN when n == 0); policy_kl = (soft cross-entropy - target entropy) / the rows' total
    target mass.  The three soft entries are None when no policies were given."""
    s = [float(x) for x in sums]
    n = int(s[15])
    nan = float("nan")

    def mean(c):
        return s[c] / n if n else nan
    out = dict(n=n, bad_targets=int(s[14]), policy_ce=mean(1), top1=mean(12), top5=mean(13), policy_entropy=mean(3),
               valid_mass=mean(4), policy_ce_soft=None, target_entropy=None, policy_kl=None,
               value_mse=mean(10), value_bias=mean(9), value_sign_acc=mean(11))
    if soft:
        out.update(policy_ce_soft=mean(6), target_entropy=mean(7), policy_kl=(s[6] - s[7]) / s[5] if s[5] else nan)
    return out


class YkNet:
    """Owns a device copy of the weights in the kernels' layout (yk_net_create).

    precision "f32" (default): f32-equivalent products, within 1e-5 of the reference's float32
    predict.  "f16": fp16 weights / GEMM inputs with f32 accumulation and f32 Linear outputs - the
    operand precision of the reference's own GPU predict under autocast('cuda') (NNet.py:186-189;
    autocast also rounds the outputs to fp16, this mode does not), an opt-in perf mode."""

    def __init__(self, state_dict, hidden: int, nblocks: int, precision: str = "f32"):
        arrs = [np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy() if torch.is_tensor(t)
                                     else np.asarray(t, dtype=np.float32)) for t in state_dict.values()]
        if len(arrs) != 14 + 8 * nblocks:
            raise ValueError(f"state_dict has {len(arrs)} tensors, expected {14 + 8 * nblocks}")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        h = C.c_void_p()
        call("yk_net_create", C.byref(h), hidden, nblocks, ptrs, len(arrs))
        self.handle = h.value
        self.hidden, self.nblocks = hidden, nblocks
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        call("yk_net_set_precision", self.handle, PRECISIONS[precision])

    def predict_states(self, states: torch.Tensor):
        """states int64[n, 8] (device) -> pi f32[n, 3226], v f32[n]."""
        n = states.shape[0]
        pi = torch.empty((n, ACTION_SIZE), dtype=torch.float32, device="cuda")
        v = torch.empty(n, dtype=torch.float32, device="cuda")
        call("yk_net_predict", self.handle, ptr(states.contiguous()), ptr(pi), ptr(v), n, stream_ptr())
        return pi, v

    def leaf_prior(self, states: torch.Tensor):
        """The self-play engine's leaf prior before renormalisation (yk_net_leaf_prior): pi at the
        valid actions of each canonical state (softmax over them), 0 elsewhere, and v."""
        n = states.shape[0]
        pi = torch.empty((n, ACTION_SIZE), dtype=torch.float32, device="cuda")
        v = torch.empty(n, dtype=torch.float32, device="cuda")
        call("yk_net_leaf_prior", self.handle, ptr(states.contiguous()), ptr(pi), ptr(v), n, stream_ptr())
        return pi, v

    def predict_features(self, x: torch.Tensor):
        x = x.to("cuda", torch.float32).contiguous()
        n = x.shape[0]
        pi = torch.empty((n, ACTION_SIZE), dtype=torch.float32, device="cuda")
        v = torch.empty(n, dtype=torch.float32, device="cuda")
        call("yk_net_predict_features", self.handle, ptr(x), ptr(pi), ptr(v), n, stream_ptr())
        return pi, v

    def policy_action(self, states: torch.Tensor):
        """states int64[n, 8] canonical (device) -> (actions i32[n], probs f32[n]): the most probable
        valid action per row, as the submission bot picks it (agent.py:248-280); -1 if none."""
        n = states.shape[0]
        actions = torch.empty(n, dtype=torch.int32, device="cuda")
        probs = torch.empty(n, dtype=torch.float32, device="cuda")
        call("yk_net_policy_action", self.handle, ptr(states.contiguous()), ptr(actions), ptr(probs), n,
             stream_ptr())
        return actions, probs

    def logits(self, states: torch.Tensor):
        """states int64[n, 8] (device) -> (logits f32[n, 3264], v f32[n]): the raw pi_head output
        (yk_net_logits; columns >= 3226 are padding) and the value, in this net's precision mode."""
        n = states.shape[0]
        logits = torch.empty((n, PI_LD), dtype=torch.float32, device="cuda")
        v = torch.empty(n, dtype=torch.float32, device="cuda")
        if n:
            call("yk_net_logits", self.handle, ptr(states.contiguous()), ptr(logits), ptr(v), n, stream_ptr())
        return logits, v

    def evaluate(self, states, targets, values, policies=None, idx=None, chunk=0, per_row=False,
                 masked=False) -> dict:
        """Forward-only, dropout-free metrics of this net on examples (yk_net_evaluate):
        device states int64[N, 8], targets int32[N], values f32[N], optionally the policies' CSR
        (pi_indptr int64[N + 1], pi_cols int32, pi_vals float64) and idx int32[n], the examples to take
        (all N when None).  Returns eval_summary of the column sums; per_row adds ``rows``, the device
        float64 [n, 16] columns.  `chunk` rows per forward (0: 16384) - the result does not depend on it.
        masked: the same numbers over the logits with -inf at each example's invalid actions
        (yk_net_evaluate_legal) - what a net trained with the legal-move mask minimises;
        valid_mass is then 1."""
        from .replay import check_mask_knobs
        masked = check_mask_knobs(masked)
        csr = check_eval_args(states, targets, values, policies, idx, chunk)
        n = int(idx.numel()) if idx is not None else int(states.shape[0])
        rows = torch.empty((n, EVAL_COLS), dtype=torch.float64, device="cuda") if per_row else None
        sums = (C.c_double * EVAL_COLS)()
        if n:
            call("yk_net_evaluate_legal" if masked else "yk_net_evaluate", self.handle, ptr(states), ptr(targets),
                 ptr(values),
                 *([ptr(t) for t in csr] if csr else [None, None, None]),
                 ptr(idx) if idx is not None else None, n, int(chunk), ptr(rows) if per_row else None, sums,
                 stream_ptr())
        out = eval_summary(sums, soft=csr is not None)
        if per_row:
            out["rows"] = rows
        return out

    def errors(self) -> int:
        """The device check flags of this net's forwards since the last call (yk_net_errors; synchronises
        the device): 0, or YK_NET_ERR_SYNC when a value-head wave timed out on its v_head.2 hand-off."""
        f = C.c_uint32()
        call("yk_net_errors", self.handle, C.byref(f))
        return int(f.value)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().yk_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class NNetWrapper:
    """NeuralNet plugin (NeuralNet.py:14-50, NNet.py:91-213) with GPU inference."""

    def __init__(self, game, args=None):
        self.game = game
        self.args = args or DEFAULT_ARGS
        self.input_len = 59
        self.action_size = game.getActionSize()
        self.nnet = YachtNNet(self.input_len, self.action_size, self.args.hidden, self.args.nblocks,
                              self.args.dropout)
        self._yk = None
        self._yk_version = None
        # averaged weights (args.emaDecay > 0): self.nnet stays the raw iterate, the shadow is
        # kept as a CPU state_dict (None: none yet - the raw weights are then the average of themselves)
        self._ema_sd = None
        self.ema_updates = 0
        self._yk_raw = None
        self._yk_raw_version = None

    def _weights_version(self):
        return tuple(p._version for p in self.nnet.parameters())

    def ema_knobs(self):
        """(decay, every) of args.emaDecay / args.emaEvery (check_ema_knobs; decay 0: off)."""
        from .replay import check_ema_knobs
        return check_ema_knobs(self.args.get("emaDecay", 0.0), self.args.get("emaEvery", 1))

    def ema_on(self) -> bool:
        return self.ema_knobs()[0] > 0.0

    def ema_state_dict(self):
        """The weights that play: the shadow when there is one, else the raw weights."""
        return self._ema_sd if self._ema_sd is not None else self.nnet.state_dict()

    def _set_shadow(self, sd, updates):
        self._ema_sd = None if sd is None else OrderedDict((k, sd[k].detach().to("cpu", torch.float32).clone())
                                                          for k in self.nnet.state_dict().keys())
        self.ema_updates = int(updates)
        self._yk = None

    def yk_net(self, raw=False) -> YkNet:
        """Device weights for the kernels; rebuilt when the torch parameters change.  With averaged weights
        (args.emaDecay) this is the averaged net - what predicts, plays, gates and reanalyses - and
        raw=True the net of self.nnet, the optimiser's iterate (cached separately)."""
        v = self._weights_version()
        if raw and self._ema_sd is not None:
            if self._yk_raw is None or v != self._yk_raw_version:
                self._yk_raw = YkNet(self.nnet.state_dict(), self.args.hidden, self.args.nblocks)
                self._yk_raw_version = v
            return self._yk_raw
        if self._yk is None or v != self._yk_version:
            self._yk = YkNet(self.ema_state_dict(), self.args.hidden, self.args.nblocks)
            self._yk_version = v
        return self._yk

    def predict(self, board):  # NNet.py:177-195
        pi, v = self.yk_net().predict_states(K.states_to_device(pack(board)))
        return pi[0].cpu().numpy(), np.float32(v[0].item())

    def predict_batch(self, states: torch.Tensor):
        return self.yk_net().predict_states(states)

    # ---- held-out evaluation (not in the reference)
    def eval_target(self, target=None) -> str:
        target = self.args.get("policy_target", "argmax") if target is None else target
        if target not in ("argmax", "visits"):
            raise ValueError(f"policy_target must be argmax or visits, not {target!r}")
        return target

    def mask_on(self) -> bool:
        """args.maskIllegal (check_mask_knobs): train on the valid-only softmax."""
        from .replay import check_mask_knobs
        return check_mask_knobs(self.args.get("maskIllegal", False))

    def evaluate(self, examples, target=None, weights=None, masked=None) -> dict:
        """Forward only, dropout off: YkNet.evaluate's numbers for this net on `examples` - every form
        train takes (tuples, an ExampleShard, a list of either).  The values are always the outcome
        (a shard's ``outcomes``, never its knob-dependent ``values``), so runs with different valueMix /
        valueLambda stay comparable.  Adds ``loss`` = policy term + vloss_weight * value_mse, the policy
        term being policy_ce, or policy_ce_soft when `target` (default args.policy_target) is "visits" -
        which needs the policies, as train does; with "argmax" the soft entries are None when the
        examples carry no policies.  `weights`: "ema" (default; the weights that play - the averaged ones with
        args.emaDecay, else the raw ones) or "raw" (self.nnet, the optimiser's iterate).  `masked`: the policy
        numbers over each example's valid actions only (YkNet.evaluate's masked form); None (default) follows
        args.maskIllegal, so `loss` is the loss being trained.  The dict's ``masked`` says which form it is."""
        from .replay import as_device_examples, as_device_policies, check_mask_knobs
        target = self.eval_target(target)
        masked = self.mask_on() if masked is None else check_mask_knobs(masked)
        if weights not in (None, "ema", "raw"):
            raise ValueError(f"weights must be ema or raw, not {weights!r}")
        states, targets, values = as_device_examples(examples, outcomes=True)
        try:
            policies = as_device_policies(examples)
        except ValueError:
            if target == "visits":
                raise
            policies = None
        out = self.yk_net(raw=weights == "raw").evaluate(states, targets, values, policies=policies, masked=masked)
        term = out["policy_ce_soft"] if target == "visits" else out["policy_ce"]
        out["loss"] = term + float(self.args.get("vloss_weight", 1.0)) * out["value_mse"]
        out["masked"] = masked
        return out

    # ---- training (NNet.py:118-174) on the native trainer (yacht_amd/train.py)
    def uses_amp(self) -> bool:
        """The reference trains under autocast('cuda') + GradScaler whenever args.cuda
        (NNet.py:113-116, 141-155) and in float32 otherwise (:157-165): args.amp, when given,
        overrides that (amp=False: the float32 step on the GPU)."""
        a = self.args
        return bool(a.get("amp", a.get("cuda", True)))

    def _trainer(self):
        from .train import Trainer
        if getattr(self, "_tr", None) is None:
            a = self.args
            decay, every = self.ema_knobs()
            self._tr = Trainer(self.nnet.state_dict(), a.hidden, a.nblocks, lr=a.lr, weight_decay=a.weight_decay,
                               max_batch=a.batch_size, vloss_weight=a.get("vloss_weight", 1.0),
                               dropout=a.dropout, seed=a.get("seed", 0), amp=self.uses_amp(),
                               ema_decay=decay, ema_every=every, legal_mask=self.mask_on())
            if decay > 0.0 and self._ema_sd is not None:  # (averaged weights loaded before there was a trainer)
                self._tr.load_ema(self._ema_sd, self.ema_updates)
        return self._tr

    def _sample_cdf(self, examples, states, targets, values, soft, gamma, sigma):
        """The sampling distribution of args.trainSteps over the pooled examples: the
        device cumulative table of recency x surprise weights.  sigma > 0 evaluates this net, as it stands,
        on the pool once (the per-row table is freed after the weights are made)."""
        from .replay import as_device_policies, sample_segments
        if states.shape[0] == 0:
            raise ValueError("trainSteps > 0 needs examples to draw from, got none")
        lens, factors = sample_segments(examples, gamma)
        table = None
        if sigma > 0.0:
            policies = soft["policies"] if soft else as_device_policies(examples)  # (none: the "visits" error)
            table = self.yk_net().evaluate(states, targets, values, policies=tuple(policies), per_row=True,
                                           masked=self.mask_on())["rows"]  # (the surprise of the loss being trained)
        w, _ = K.sample_weights(table, lens, factors, sigma)
        del table
        return K.sample_cdf(w)[0]

    def train(self, examples, verbose=True):
        """The reference loop: `epochs` passes over shuffled minibatches of `batch_size`
        (drop_last False), one CE(argmax pi) + vloss_weight * MSE step each, clip 5.0, AdamW -
        as the reference's GPU path when args.cuda (autocast('cuda') + GradScaler,
        NNet.py:113-116, 141-155) on fp16 MFMA kernels, or in float32 (the reference's CPU path)
        with args.cuda False or args.amp False (uses_amp).
        Shuffles come from a torch generator seeded per call (the reference uses the global
        torch RNG); dropout masks from the trainer's Philox stream.

        `examples`: the reference's list of (board, pi, v), an ExampleShard (device replay
        buffer), or a list of either (trainExamplesHistory).  Under torch.distributed every
        rank holds the same pooled examples and draws the same permutation, and
        args.ddp_batch picks how the ranks share a minibatch:
          "replicated" (default): every rank takes the whole minibatch's step itself - no
            collective, parameters bit-identical to one process training alone.  The step is
            latency-bound (a 16-row tile per workgroup, 32 of them at batch 512), so
            a rank's share of a split batch would not run faster, and the split adds an
            all-reduce per step;
          "split": the minibatch split across the ranks, the share-weighted gradients
            all-reduced (DDP): the single-process step up to f32 summation order;
          "per_rank": every rank its own batch_size rows (a world x batch_size global batch).

        args.policy_target: "argmax" (default; the reference's hard label, NNet.py:145-146) or
        "visits" - cross-entropy against the full MCTS visit policy pi = N / sum N (soft targets,
        F.cross_entropy(out_pi, pi); a departure from the reference), in every ddp_batch mode.
        It needs the policies: tuples, or shards built by examples_from_images.

        args.symmetries: () (default; the reference's getSymmetries is the identity) or an iterable over
        {"carry", "rolls", "groups"} - symmetry augmentation, a departure from the reference: at the top
        of every epoch each example (board, target and, for "visits", its policy row) is replaced by a
        random member of its symmetry class, drawn on the device for (args.seed, the optimiser step count
        at that moment, the example's index) - K.augment_examples, DESIGN.md 7b-sym - into buffers
        allocated once per call; the epoch's steps then run unchanged on that copy.

        args.trainSteps: 0 (default; the epochs of full permutations above) or T > 0 - weighted minibatch
        sampling, a departure from the reference: the call takes exactly T steps, each
        on batch_size examples drawn with replacement on the device (K.sample_weights / sample_cdf /
        sample_draw) for (args.seed, the optimiser step count at the call's start, the draw's number).
        An example's weight is sampleRecency ** age - when `examples` is a list of shards or lists, the
        last item has age 0; any other form is one segment - times (1 - sampleSurprise) + sampleSurprise x
        (its policy KL over the pool's mean KL), the KL of its visit policy from this net's policy as the
        call found the net (one YkNet.evaluate over the un-augmented pool; needs the policies).  The T
        steps are split over args.epochs rounds (round e: steps floor(e T / E) .. floor((e + 1) T / E) - 1;
        empty rounds are skipped), a round being what an epoch is to the loss report and the symmetries.

        args.emaDecay: 0 (default; the net that plays is the last step's iterate, as in the reference) or a decay
        in (0, 1) - averaged weights, a departure from the reference: after every
        args.emaEvery-th step (default 1) a device shadow of the parameters moves toward them,
        e <- e + w_t (p - e).  self.nnet stays the raw iterate; after the call yk_net() - predict, the engines,
        the gate, reanalysis, evaluate, the sampler's surprise - is built from the shadow.

        args.maskIllegal: False (default; the softmax of the policy loss runs over all 3226 actions, as in the
        reference) or True - the legal-move mask, a departure from the reference: softmax,
        loss and gradient over each example's valid actions only, which is what the search reads.  The examples
        must keep its contract - a valid action in every state, valid hard targets, p > 0 on valid actions only -
        which is checked once per call on the device (K.check_legal; with symmetries on the un-augmented pool:
        the augmentation keeps targets legal); a violation raises ValueError before any step runs."""
        from . import dist as D
        from .replay import as_device_examples, as_device_policies, check_sample_knobs, sample_rounds
        target = self.args.get("policy_target", "argmax")
        if target not in ("argmax", "visits"):
            raise ValueError(f"policy_target must be argmax or visits, not {target!r}")
        symmetries = self.args.get("symmetries", ()) or ()
        symmetries = (symmetries,) if isinstance(symmetries, str) else tuple(symmetries)
        K.symmetry_flags(symmetries)  # an unknown name: ValueError, before any device work
        T, gamma, sigma = check_sample_knobs(self.args.get("trainSteps", 0) or 0, self.args.get("sampleRecency", 1.0),
                                             self.args.get("sampleSurprise", 0.0))
        ema_on = self.ema_on()  # (bad emaDecay / emaEvery: ValueError, before any device work)
        mask_on = self.mask_on()  # (a non-bool maskIllegal: ValueError, before any device work)
        tr = self._trainer()
        if tr.legal_mask != mask_on:  # (the knob changed since the trainer was built)
            tr.set_legal_mask(mask_on)
        states, targets, values = as_device_examples(examples)
        # "visits": the same rows' policies as a CSR; "argmax" calls the trainer exactly as before
        soft = {"policies": as_device_policies(examples)} if target == "visits" else {}
        if mask_on and states.shape[0]:  # the mask's contract, once per call, before any step
            bad, kind = K.check_legal(states, None if soft else targets, soft.get("policies"))
            if bad >= 0:
                raise ValueError(f"maskIllegal: example {bad} of the pooled examples breaks the legal-move mask's "
                                 f"contract: {K.LEGAL_KINDS[kind]}")
        cdf = self._sample_cdf(examples, states, targets, values, soft, gamma, sigma) if T else None
        rounds, key, drawn, picks = sample_rounds(T, self.args.epochs), tr.step_count & 0xFFFFFFFF, 0, None
        pool, aug = (states, targets, soft.get("policies")), None
        if symmetries and soft:
            K.check_policy_columns(soft["policies"])
        rank, world = D.rank_world()
        n = states.shape[0]
        bs = self.args.batch_size
        mode = self.args.get("ddp_batch", "replicated") if world > 1 else "replicated"
        if mode not in ("replicated", "split", "per_rank"):
            raise ValueError(f"ddp_batch must be replicated, split or per_rank, not {mode!r}")
        rows = bs * world if mode == "per_rank" else bs
        vw = self.args.get("vloss_weight", 1.0)
        g = torch.Generator(device="cuda")
        g.manual_seed(int(self.args.get("seed", 0)) + 1000003 * tr.step_count)
        for epoch in range(self.args.epochs):
            if T and rounds[epoch][0] == rounds[epoch][1]:
                continue  # (an empty round of the sampled steps: T < epochs)
            if symmetries and n:  # this epoch's copy of the pool (every rank holds the pool: the same copy)
                aug = K.augment_examples(*pool, int(self.args.get("seed", 0)), tr.step_count & 0xFFFFFFFF,
                                         symmetries, out=aug)
                states, targets = aug[0], aug[1]
                if soft:
                    soft = {"policies": aug[2]}
            if T:  # this round's steps x rows draws (every rank holds the pool: the same draws)
                count = (rounds[epoch][1] - rounds[epoch][0]) * rows
                if picks is None:
                    picks = torch.empty(-(-T // self.args.epochs) * rows, dtype=torch.int32, device="cuda")
                perm = K.sample_draw(cdf, int(self.args.get("seed", 0)), key, drawn, count, out=picks)
                drawn += count
            else:
                perm, count = torch.randperm(n, generator=g, device="cuda").to(torch.int32), n
            report = verbose and (epoch % 5 == 0 or epoch == self.args.epochs - 1)
            if report:
                tr.epoch_loss_begin(vw)  # summed on the device, read once after the epoch
            for i in range(0, count, rows):
                idx = perm[i:i + rows]
                if mode == "replicated":
                    tr.step(states, targets, values, idx=idx, **soft)
                    b = idx.numel()
                else:
                    parts = torch.tensor_split(idx, world)
                    loc = parts[rank]
                    b = loc.numel()
                    row0 = sum(int(x.numel()) for x in parts[:rank])  # this rank's rows in the minibatch
                    if b:
                        tr.backward(states, targets, values, idx=loc, row0=row0, **soft)
                    else:
                        tr.grads().zero_()
                    D.allreduce_grads(tr, weight=b / idx.numel())
                    tr.apply()
            if report:
                total, batches = tr.epoch_loss_end()
                if rank == 0:
                    print(f"Epoch {epoch + 1}/{self.args.epochs}, Avg Loss: {total / max(batches, 1):.4f}")
        with torch.no_grad():
            self.nnet.load_state_dict(tr.state_dict())  # the torch copy feeds checkpoints and predict
        self._yk = None
        if ema_on:  # the shadow's host copy feeds predict and the checkpoints' second set
            self._set_shadow(tr.ema_state_dict(), tr.ema_state()["updates"])

    # ---- checkpoints (NNet.py:198-213): the reference's dict, loaded without unpickling code
    def save_checkpoint(self, folder="checkpoint", filename="checkpoint.pth.tar"):
        from .train import optimizer_state_dict
        os.makedirs(folder, exist_ok=True)
        if getattr(self, "_tr", None) is not None:
            opt = optimizer_state_dict(self._tr, self.nnet, self.args.lr, self.args.weight_decay)
        else:
            opt = torch.optim.AdamW(self.nnet.parameters(), lr=self.args.lr,
                                    weight_decay=self.args.weight_decay).state_dict()
        ck = {"state_dict": self.nnet.state_dict(), "optimizer": opt, "args": dict(self.args)}
        if self.ema_on():  # "state_dict" stays the raw iterate: the optimiser state belongs to it
            ck["ema_state_dict"] = OrderedDict((k, v.clone()) for k, v in self.ema_state_dict().items())
            ck["ema_updates"] = int(self.ema_updates)
        torch.save(ck, os.path.join(folder, filename))

    def export_ema(self, folder="checkpoint", filename="ema.pth.tar"):
        """The averaged weights as a plain reference-format checkpoint ({"state_dict", "args"}): the file for
        bot.py, `python -m yacht_amd.evaluate` or the reference.  Without a shadow these are the raw weights."""
        os.makedirs(folder, exist_ok=True)
        sd = OrderedDict((k, v.detach().to("cpu").clone()) for k, v in self.ema_state_dict().items())
        torch.save({"state_dict": sd, "args": dict(self.args)}, os.path.join(folder, filename))

    def load_checkpoint(self, folder="checkpoint", filename="checkpoint.pth.tar", load_optimizer=False):
        from .train import load_optimizer_state_dict
        ck = torch.load(os.path.join(folder, filename), map_location="cpu", weights_only=True)
        sd = ck["state_dict"] if "state_dict" in ck else ck
        self.nnet.load_state_dict(OrderedDict(sd))
        self._yk = None
        if getattr(self, "_tr", None) is not None:
            self._tr.load_params(self.nnet.state_dict())
        if self.ema_on():  # (off: the file's averaged weights, if any, are ignored)
            if "ema_state_dict" in ck:
                self._set_shadow(OrderedDict(ck["ema_state_dict"]), int(ck.get("ema_updates", 0)))
            else:  # a file without them: the loaded weights are the average of themselves
                self._set_shadow(None, 0)
            if getattr(self, "_tr", None) is not None:
                self._tr.load_ema(self._ema_sd, self.ema_updates)
        if load_optimizer and "optimizer" in ck:
            load_optimizer_state_dict(self._trainer(), self.nnet, ck["optimizer"])


class HashPriorNet:
    """Deterministic stand-in for NNetWrapper (oracle/spec.py hash_prior, computed on the
    GPU by the engine itself).  It exists so whole self-play episodes can be compared
    bit-for-bit with the reference's own Coach/MCTS code; it is not a model."""

    yk_prior = "hash"

    def __init__(self, game=None, args=None):
        self.game = game

    def predict(self, board):
        pi, v = K.hash_prior(K.states_to_device(pack(board)))
        return pi[0].cpu().numpy(), np.float32(v[0].item())
