"""SelfPlayEngine: batched Coach.executeEpisode on one GPU (yk_selfplay).

One ``run`` plays a complete episode for every one of ``n_envs`` games in lock-step:
48 real moves x ``sims`` MCTS simulations each, all on the device (include/yacht_hip.h).
Game i uses the RNG stream ``(seed, env_base + i)``; trees are fresh per episode
(Coach.py:93).  Records come back as numpy arrays or as one packed device buffer for the
multi-GPU all-gather (``yacht_amd.dist``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import YK_REC_FAST, YkEngineConfigFull, call, lib, stream_ptr

ACTION_SIZE = 3226


class SelfPlayEngine:
    def __init__(self, n_envs: int, sims: int, cpuct: float = 1.5, temp_threshold: int = 15, net=None,
                 prior: str = "net", max_moves: int = 64, record_predictions: bool = False,
                 max_expansions: int = 0, arena_entries: int = 0, record_stride: int = 1, groups: int = 0,
                 dual_trees: bool = False, opponent_net=None, dirichlet_alpha: float = 0.0,
                 dirichlet_eps: float = 0.0, record_root_values: bool = False, playout_fast_sims: int = 0,
                 playout_full_prob: float = 1.0, forced_playouts_k: float = 0.0, forced_prune: bool = True,
                 fpu_reduction=None, fpu_root_reduction=None, move_temperature=None, move_temperature_early=None,
                 root_policy_temperature=None, root_policy_temperature_early=None, temperature_halflife=None,
                 score_utility=None, score_scale=None):
        if prior not in ("net", "hash"):
            raise ValueError("prior is 'net' (YachtNNet on MFMA) or 'hash' (deterministic test prior)")
        if prior == "net" and net is None:
            raise ValueError("prior='net' needs a YkNet")
        self.cfg = YkEngineConfigFull(
            n_envs=n_envs, sims=sims, cpuct=cpuct, temp_threshold=temp_threshold,
            max_moves=max_moves, prior=0 if prior == "net" else 1,
            record_predictions=int(record_predictions),
            max_expansions=max_expansions or (max_moves * sims + 8),
            arena_entries=arena_entries, record_stride=max(int(record_stride), 1),
            groups=int(groups), dual_trees=int(bool(dual_trees)),
            # AlphaZero's root noise in run() (never in arena()); on when both are > 0
            dirichlet_alpha=float(dirichlet_alpha), dirichlet_eps=float(dirichlet_eps),
            # the search's own value of each real move of run(), in info[..., 7] (DESIGN.md 7b-val;
            # never in arena())
            record_root_values=int(bool(record_root_values)))
        self.net = net  # keep the weights alive
        h = C.c_void_p()
        call("yk_engine_create", C.byref(h), C.byref(self.cfg), C.c_void_p(net.handle if net is not None else None))
        self.handle = h.value
        self.n_envs, self.sims, self.max_moves = n_envs, sims, max_moves
        # playout cap randomization in run() (never in arena()): each move of a batch is searched
        # in full with probability playout_full_prob, else with playout_fast_sims simulations; 0 is off
        self.playout_fast_sims, self.playout_full_prob = int(playout_fast_sims), float(playout_full_prob)
        if self.playout_fast_sims != 0:
            try:
                call("yk_engine_set_playout_cap", self.handle, self.playout_fast_sims, self.playout_full_prob)
            except Exception:
                self.close()
                raise
        # forced playouts and policy target pruning at the roots of run()'s full moves (never in arena(); DESIGN.md
        # 6f): a visited root child is searched until N^2 >= k P Ns, and the visits that the search's own PUCT
        # values did not justify are taken off the recorded counts (forced_prune=False: forcing alone); 0 is off
        self.forced_playouts_k, self.forced_prune = float(forced_playouts_k), bool(forced_prune)
        if self.forced_playouts_k != 0.0:
            try:
                call("yk_engine_set_forced_playouts", self.handle, self.forced_playouts_k, int(self.forced_prune))
            except Exception:
                self.close()
                raise
        # first-play urgency in every search of this engine - run(), arena() (both trees) and yk_mcts_search
        # (DESIGN.md 6g): an unvisited edge starts from the visited children's visit-weighted mean less
        # fpu_reduction * sqrt(prior mass tried) - fpu_root_reduction at depth 0, by default the same - instead
        # of from 0.  None is off; 0 is legal and is not off
        if fpu_reduction is None and fpu_root_reduction is not None:
            self.close()
            raise ValueError("fpu_root_reduction needs fpu_reduction: alone it would silently do nothing")
        self.fpu_reduction = None if fpu_reduction is None else float(fpu_reduction)
        self.fpu_root_reduction = (self.fpu_reduction if fpu_root_reduction is None or fpu_reduction is None
                                   else float(fpu_root_reduction))
        if self.fpu_reduction is not None:
            try:
                call("yk_engine_set_fpu", self.handle, 1, self.fpu_reduction, self.fpu_root_reduction)
            except Exception:
                self.close()
                raise
        # the self-play temperatures in run() (never in arena()), each on the schedule T(m) = final +
        # (early - final) * 2 ** (-m / temperature_halflife) over the real move m: move_temperature draws a temp-1
        # move from N ** (1 / T) (temp_threshold still decides where argmax begins), root_policy_temperature
        # searches the root with P ** (1 / T) renormalised, applied before the Dirichlet mix.  None is off
        try:
            from .replay import check_temperature_knobs
            tk = check_temperature_knobs(move_temperature, move_temperature_early, root_policy_temperature,
                                         root_policy_temperature_early, temperature_halflife)
            self.move_temperature, self.move_temperature_early = tk["move_temperature"], tk["move_temperature_early"]
            self.root_policy_temperature = tk["root_policy_temperature"]
            self.root_policy_temperature_early = tk["root_policy_temperature_early"]
            self.temperature_halflife = tk["temperature_halflife"]
            if self.move_temperature is not None or self.root_policy_temperature is not None:
                call("yk_engine_set_temperatures", self.handle, self.move_temperature_early or 0.0,
                     self.move_temperature or 0.0, self.root_policy_temperature_early or 0.0,
                     self.root_policy_temperature or 0.0, self.temperature_halflife or 0.0)
        except Exception:
            self.close()
            raise
        # the score-margin utility at the terminal states of every search of this engine - run() (full and fast
        # moves), arena() (both trees) and yk_mcts_search: a terminal descent returns
        # (1 - score_utility) * z + score_utility * x / (1 + |x|), x = the final margin / score_scale, in place of
        # the outcome z.  The records and the arena results stay the game's own.  None is off; a weight of 0 is legal,
        # is not off and searches as off does
        if score_utility is None and score_scale is not None:
            self.close()
            raise ValueError("score_scale needs score_utility: alone it would silently do nothing")
        if score_utility is not None and score_scale is None:
            self.close()
            raise ValueError("score_utility needs score_scale (game points, > 0): there is no default scale")
        self.score_utility = None if score_utility is None else float(score_utility)
        self.score_scale = None if score_scale is None else float(score_scale)
        if self.score_utility is not None:
            try:
                call("yk_engine_set_score_utility", self.handle, 1, self.score_utility, self.score_scale)
            except Exception:
                self.close()
                raise
        self.opponent_net = opponent_net
        if opponent_net is not None:
            # MCTS vs MCTS with two nets, each seat its own tree (the gating arena, Coach.py:117-139)
            call("yk_engine_set_opponent_net", self.handle, C.c_void_p(opponent_net.handle))

    ERROR_BITS = {1: "node pool", 2: "edge pool", 4: "arena", 8: "search depth", 16: "transition status",
                  32: "root round went backwards", 64: "visit records", 128: "move cap", 256: "zero visit counts",
                  512: "root not in tree", 1024: "hash index full", 2048: "forward hand-off timed out"}

    def run(self, seed: int, env_base: int = 0, stream=None):
        from ._lib import YkError
        try:
            call("yk_selfplay", self.handle, seed & (2**64 - 1), env_base & (2**32 - 1), stream_ptr(stream))
        except YkError as e:
            st = self.stats()
            bits = [n for b, n in self.ERROR_BITS.items() if st["errors"] & b]
            raise YkError(f"yk_selfplay [{', '.join(bits)}; stats {st}]", e.code) from None

    PLAYERS = {"mcts": 0, "random": 1, "greedy": 2}  # YK_PLAYER_*

    def arena(self, agent_seat, seed: int, env_base: int = 0, stream=None, agent: str = "mcts",
              opponent: str = "random"):
        """Batched Arena.playGame (yk_arena): `agent` in seat agent_seat[i] against `opponent`,
        each "mcts" (temp 0, this engine's net / prior and sims), "random" or "greedy"; game i
        uses stream (seed, env_base + i)."""
        from ._lib import YkError
        seat = np.ascontiguousarray(np.broadcast_to(np.asarray(agent_seat, dtype=np.int32), (self.n_envs,)))
        try:
            call("yk_arena", self.handle, seed & (2**64 - 1), env_base & (2**32 - 1), seat.ctypes.data,
                 self.PLAYERS[agent], self.PLAYERS[opponent], stream_ptr(stream))
        except YkError as e:
            st = self.stats()
            bits = [n for b, n in self.ERROR_BITS.items() if st["errors"] & b]
            raise YkError(f"yk_arena [{', '.join(bits)}; stats {st}]", e.code) from None

    def arena_results(self) -> dict:
        E, M = self.n_envs, self.max_moves
        result = np.zeros(E, dtype=np.float64)
        totals = np.zeros((E, 2), dtype=np.int32)
        nm = np.zeros(E, dtype=np.int32)
        actions = np.zeros((E, M), dtype=np.int32)
        final = np.zeros((E, 8), dtype=np.uint64)
        ctr = np.zeros(E, dtype=np.uint64)
        call("yk_arena_results", self.handle, result.ctypes.data, totals.ctypes.data, nm.ctypes.data,
             actions.ctypes.data, final.ctypes.data, ctr.ctypes.data)
        return dict(result=result, totals=totals, n_moves=nm, actions=actions, final=final, ctr=ctr)

    # class 0: the first descent of each move; class 3: expand + backup + the next descent
    KERNEL_CLASSES = ("select", "forward", "root_sort_select", "expand_backup_select", "move_begin", "move_end")

    def profile(self, enable: bool = True, stride: int = 1):
        """Per-kernel HIP event timing; the forward / expand pair of every `stride`-th simulation."""
        call("yk_engine_profile", self.handle, int(stride) if enable else 0)

    def kernel_times(self) -> dict:
        ms = np.zeros(8, dtype=np.float64)
        n = np.zeros(8, dtype=np.int64)
        call("yk_engine_kernel_times", self.handle, ms.ctypes.data, n.ctypes.data)
        kt = {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.KERNEL_CLASSES) if k != "unused"}
        if self.cfg.dirichlet_alpha > 0 and self.cfg.dirichlet_eps > 0:
            kt["root_noise"] = (float(ms[6]), int(n[6]))  # k_root_noise, two launches per move (class 6)
        if self.root_policy_temperature is not None:  # its tempered form: with the noise on, the same launches
            kt["root_temper"] = (float(ms[6]), int(n[6]))
        if self.cfg.record_root_values:
            kt["root_value"] = (float(ms[7]), int(n[7]))  # k_root_value, one launch per move (class 7)
        return kt

    STAT_NAMES = ("expansions", "scanned", "moves", "errors", "max_nodes", "max_edges", "max_arena", "vnew",
                  "path_edges", "sims", "node_cap", "edge_cap", "arena_cap", "visit_cap", "groups",
                  "forward_parts")
    # yk_engine_counters: the scans' edge gathers; expansions by the prior's path
    # fast_moves: the lock-step moves of the last batch that ran with the fast playout cap
    # forced_picks / pruned_visits: the last batch's root picks that took a forced edge, and the visits the
    # pruning took off its recorded counts
    # fpu_unvisited_picks / fpu_picks: the last batch's descent picks (every depth) that first-play urgency gave
    # to the unvisited candidate, and the picks its rule decided - nodes with both kinds of edge
    # utility_terminals: the last batch's descents that ended at a terminal state and returned a score-margin
    # utility (0 with it off)
    COUNTER_NAMES = ("scan_edges", "prior_window", "prior_sparse", "prior_general", "fast_moves", "forced_picks",
                     "pruned_visits", "fpu_unvisited_picks", "fpu_picks", "utility_terminals")

    def stats(self) -> dict:
        out = np.zeros(16, dtype=np.int64)
        call("yk_engine_stats", self.handle, out.ctypes.data)
        st = {k: int(out[i]) for i, k in enumerate(self.STAT_NAMES)}
        more = np.zeros(len(self.COUNTER_NAMES), dtype=np.int64)
        if hasattr(lib(), "yk_engine_counters"):  # (absent only from older diagnostic baselines)
            call("yk_engine_counters", self.handle, more.ctypes.data, len(more))
        st.update({k: int(more[i]) for i, k in enumerate(self.COUNTER_NAMES)})
        return st

    def records(self) -> dict:
        E, M = self.n_envs, self.max_moves
        states = np.zeros((E, M, 8), dtype=np.uint64)
        info = np.zeros((E, M, 8), dtype=np.int32)
        ctr = np.zeros((E, M, 2), dtype=np.uint64)
        values = np.zeros((E, M), dtype=np.float64)
        final = np.zeros((E, 8), dtype=np.uint64)
        nm = np.zeros(E, dtype=np.int32)
        nv = np.zeros(1, dtype=np.int64)
        call("yk_engine_records", self.handle, None, None, None, None, None, None, None, None, nv.ctypes.data)
        voff = np.zeros(E * M + 1, dtype=np.int64)
        visits = np.zeros((max(int(nv[0]), 1), 2), dtype=np.int32)
        call("yk_engine_records", self.handle, states.ctypes.data, info.ctypes.data, ctr.ctypes.data,
             values.ctypes.data, final.ctypes.data, nm.ctypes.data, voff.ctypes.data, visits.ctypes.data,
             nv.ctypes.data)
        rec = dict(states=states, info=info, ctr=ctr, values=values, final=final, n_moves=nm,
                   visits_off=voff.reshape(-1)[:E * M + 1], visits=visits[:int(nv[0])])
        if self.cfg.record_root_values:
            rec["root_values"] = decode_root_values(info[:, :, 7])  # float32 [n, max_moves], NaN where absent
        if self.playout_fast_sims > 0:  # bool [n, max_moves]: the played moves searched with the fast cap
            rec["fast"] = ((info[:, :, 6] & YK_REC_FAST) != 0) & (np.arange(M)[None, :] < nm[:, None])
        return rec

    def predictions(self, leaves: bool = False):
        """(pi, v, count[, leaves]) of the recorded games (every record_stride-th): pi[r, k] is
        Ps * valids of game r * record_stride's k-th expansion (MCTS.py:86-88, before the
        renormalisation), exactly what the search used; count[r] its expansions."""
        R = (self.n_envs + self.cfg.record_stride - 1) // self.cfg.record_stride
        X = self.cfg.max_expansions
        pi = np.zeros((R, X, ACTION_SIZE), dtype=np.float32)
        v = np.zeros((R, X), dtype=np.float32)
        lv = np.zeros((R, X, 8), dtype=np.uint64) if leaves else None
        cnt = np.zeros(R, dtype=np.int32)
        call("yk_engine_predictions", self.handle, pi.ctypes.data, v.ctypes.data,
             lv.ctypes.data if leaves else None, cnt.ctypes.data)
        if (cnt > X).any():
            raise RuntimeError(f"prediction record truncated: {int(cnt.max())} expansions > max_expansions {X}")
        return (pi, v, cnt, lv) if leaves else (pi, v, cnt)

    def root_priors(self):
        """(before, after), float32[R, max_moves, 3226] dense by action, of the recorded games of the last
        run(): each move's root prior as the Dirichlet noise found it and as it left it (0 at invalid
        actions and past the game's end).  Needs record_predictions and the noise on."""
        R = (self.n_envs + self.cfg.record_stride - 1) // self.cfg.record_stride
        before = np.zeros((R, self.max_moves, ACTION_SIZE), dtype=np.float32)
        after = np.zeros_like(before)
        call("yk_engine_root_priors", self.handle, before.ctypes.data, after.ctypes.data)
        return before, after

    def temperatures(self):
        """(move_t, root_t), float64[max_moves] each: the tables of T by real move this engine holds (DESIGN.md
        6h), None for a schedule that is off."""
        mt = np.zeros(self.max_moves, dtype=np.float64)
        rt = np.zeros(self.max_moves, dtype=np.float64)
        call("yk_engine_temperatures", self.handle, mt.ctypes.data, rt.ctypes.data)
        return (mt if self.move_temperature is not None else None,
                rt if self.root_policy_temperature is not None else None)

    def record_bytes(self) -> int:
        n = int(lib().yk_engine_record_bytes(self.handle))
        if n < 0:
            raise RuntimeError("yk_engine_record_bytes failed")
        return n

    def pack_records(self, out: torch.Tensor = None, stream=None) -> torch.Tensor:
        nb = self.record_bytes()
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device="cuda")
        call("yk_engine_pack_records", self.handle, out.data_ptr(), out.numel(), stream_ptr(stream))
        return out

    def close(self):
        if getattr(self, "handle", None):
            lib().yk_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def playout_schedule(seed: int, env_base: int, full_prob: float, n_moves: int) -> np.ndarray:
    """yk_playout_schedule: bool[n_moves], True where move m of a self-play batch started with (seed, env_base)
    is searched in full under full_prob.  Host only."""
    full = np.zeros(max(int(n_moves), 1), dtype=np.uint8)
    call("yk_playout_schedule", seed & (2**64 - 1), env_base & (2**32 - 1), float(full_prob), int(n_moves),
         full.ctypes.data)
    return full[:int(n_moves)].astype(bool)


def decode_root_values(words: np.ndarray) -> np.ndarray:
    """info[..., 7] words (record_root_values) -> float32 root values: the word is the value's bit pattern
    (a zero value is stored as 0x80000000, so it comes back as -0.0), and the zero word - no value
    recorded - becomes NaN."""
    w = np.ascontiguousarray(words, dtype=np.int32).view(np.uint32)
    return np.where(w == 0, np.uint32(0x7FC00000), w).astype(np.uint32).view(np.float32)


def unpack_record_image(buf: np.ndarray, n_envs: int, max_moves: int, sims: int) -> dict:
    """Inverse of yk_engine_pack_records (host bytes of one rank's image)."""
    E, M = n_envs, max_moves
    vcap = 2 * M * max(sims, 32)
    parts = [("states", np.uint64, (E, M, 8)), ("info", np.int32, (E, M, 8)), ("ctr", np.uint64, (E, M, 2)),
             ("values", np.float64, (E, M)), ("visits_raw", np.uint32, (E, vcap)), ("voff", np.int32, (E, M + 1)),
             ("n_moves", np.int32, (E,)), ("final", np.uint64, (E, 8))]
    out, off = {}, 0
    raw = np.ascontiguousarray(buf).view(np.uint8)
    for name, dt, shape in parts:
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = raw[off:off + nb].view(dt).reshape(shape)
        off += (nb + 15) & ~15
    return out
