"""Coach self-play and learning on the MI355X engine (Coach.py:17-170).

``executeEpisode`` keeps the reference's return value - a list of
``(canonicalBoard, pi, v)`` - and ``executeEpisodes(n)`` plays n games in one lock-step
batch on the GPU (``SelfPlayEngine``).  ``learn`` is the reference loop at device scale and on
any number of ranks (one process per GPU, torch.distributed):

* self-play: the iteration's numEps games are sharded over the ranks by global env id, each
  rank's trajectory records are all-gathered (RCCL) and turned into device examples
  (``replay.ExampleShard``) - the same pooled buffer a single GPU playing every game builds;
* train: ``NNetWrapper.train`` on the pooled history, each minibatch split over the ranks with
  an all-reduce of the gradients (DDP), so every rank holds the same new net;
* gating: ``arena.GatingArena`` - pmcts vs nmcts as one dual-tree device batch, games sharded,
  tallies summed - then accept / reject as Coach.py:127-139.
* reanalysis (opt-in, ``args.reanalyseFraction``; not in the reference): after the iteration's self-play, a
  Philox-chosen fraction of every older iteration's examples is searched again with the current net and
  their policy targets replaced (``replay.reanalyse``).  Every rank does all of it.
* playout cap randomization (opt-in, ``args.playoutFastSims`` / ``playoutFullProb``; not in the reference;
  DESIGN.md 6e): each move of a self-play batch is searched in full (numMCTSSims) with probability
  playoutFullProb and with playoutFastSims simulations otherwise; only the full moves become examples.
* forced playouts and policy target pruning (opt-in, ``args.forcedPlayoutsK``, ``forcedPrune``; not in the
  reference): at the roots of self-play's full moves a visited child is searched until
  N^2 >= k P Ns, and the forced visits the search's PUCT values did not justify are taken off the recorded
  counts, which the policy targets are made of.
* first-play urgency (opt-in, ``args.fpuReduction``, ``fpuRootReduction``; not in the reference):
  an unvisited edge starts from the visited children's visit-weighted mean less a reduction, not from 0 - in
  everything that searches: self-play, the held-out games, the reanalysis, the gate, ``MCTSArena``, the plugin.
* score-margin utility (opt-in, ``args.scoreUtility``, ``scoreScale``; not in the reference): a
  bounded function of the final point margin is blended into the outcome, at the terminal states of every search
  (self-play, the held-out games, the reanalysis, the gate, ``MCTSArena``, the plugin) and in the value targets;
  the records, the examples files, the gate's tallies and ``NNetWrapper.evaluate`` keep the outcome.
* self-play temperatures (opt-in, ``args.moveTemperature`` / ``moveTemperatureEarly``,
  ``rootPolicyTemperature`` / ``rootPolicyTemperatureEarly``, ``temperatureHalflife``; not in the reference;
  DESIGN.md 6h): a temp-1 move is drawn from N^(1/T) and the self-play root searched with P^(1/T) renormalised,
  T on a schedule over the game - in self-play and the held-out games only; the policy targets are untouched.
* held-out evaluation (opt-in, ``args.holdoutEps = m``; not in the reference): m more self-play games per
  iteration that never enter training, on which the previous and the new net are evaluated after
  train (``NNetWrapper.evaluate``; ``last_eval``, ``eval_history``).  The gate does not use it.

Randomness comes from per-game Philox streams ``(game seed, env id)``: the Coach hands out
consecutive env ids starting at the game's own (``_streams``), episodes first, then each
iteration's arena games, so no two games ever share a stream.  Every episode starts from a
fresh tree (Coach.py:93).
"""
from __future__ import annotations

import logging
import os

from ._lib import YK_REC_FAST
from .engine import SelfPlayEngine
from .mcts import MCTS
from .state import ACTION_SIZE, unpack

# every real game has exactly 48 moves (2 bids in round 1, 2 bids + 2 scores in rounds 2-12,
# 2 scores in round 13; YachtGame.py:266-370): the record capacity of the Coach's engines, so
# the all-gathered images carry no padding moves (a longer game would be a move-cap error)
GAME_MOVES = 48


def examples_from_records(rec: dict, n_envs: int):
    """Engine records -> per-game lists of (YachtState, pi list, v) as Coach.py:72 returns.  A fast move of the
    playout cap (info[6] & 0x100) is not an example."""
    out = []
    M = rec["states"].shape[1]
    for e in range(n_envs):
        ex = []
        for m in range(int(rec["n_moves"][e])):
            if int(rec["info"][e, m, 6]) & YK_REC_FAST:
                continue
            temp, _player, action = (int(x) for x in rec["info"][e, m, :3])
            a0, a1 = int(rec["visits_off"][e * M + m]), int(rec["visits_off"][e * M + m + 1])
            if temp == 0:
                pi = [0] * ACTION_SIZE
                pi[action] = 1
            else:
                counts = [0] * ACTION_SIZE
                for a, c in rec["visits"][a0:a1]:
                    counts[int(a)] = int(c)
                counts = [x ** 1.0 for x in counts]
                s = float(sum(counts))
                pi = [x / s for x in counts]
            ex.append((unpack(rec["states"][e, m]), pi, float(rec["values"][e, m])))
        out.append(ex)
    return out


log = logging.getLogger(__name__)


class Coach:
    def __init__(self, game, nnet, args):
        self.game, self.nnet, self.args = game, nnet, args
        # search-value targets: valueMix = beta, valueLambda = lambda; (0, 1) is off -
        # the reference's value target, the outcome.  Checked here, before anything touches the device.
        from .replay import check_value_knobs
        self.value_mix, self.value_lambda = check_value_knobs(args.get("valueMix", 0.0),
                                                              args.get("valueLambda", 1.0))
        # weighted minibatch sampling: NNetWrapper.train's knobs, checked here as well
        from .replay import check_sample_knobs
        check_sample_knobs(args.get("trainSteps", 0) or 0, args.get("sampleRecency", 1.0),
                           args.get("sampleSurprise", 0.0))
        # reanalysis: reanalyseFraction of the older iterations' examples searched again with
        # the current net every iteration, reanalyseSims simulations each (default numMCTSSims); 0 is off -
        # no engine is built and no stream id consumed
        from .replay import check_reanalyse_knobs
        self.reanalyse_fraction, self.reanalyse_sims = check_reanalyse_knobs(
            args.get("reanalyseFraction", 0.0), args.get("reanalyseSims", None), args.get("numMCTSSims", None))
        # playout cap randomization: playoutFastSims simulations for the moves that are not drawn
        # (playoutFullProb) to be searched in full; only the full moves become examples.  Unset: off
        from .replay import check_playout_knobs
        self.playout_fast_sims, self.playout_full_prob = check_playout_knobs(
            args.get("playoutFastSims", None), args.get("playoutFullProb", None), args.get("numMCTSSims", None))
        # forced playouts and policy target pruning at the self-play roots.  Unset: off
        from .replay import check_forced_knobs
        self.forced_k, self.forced_prune = check_forced_knobs(args.get("forcedPlayoutsK", None),
                                                              args.get("forcedPrune", None))
        # first-play urgency in every search made for this Coach.  Unset: off
        from .replay import check_fpu_knobs
        self.fpu_reduction, self.fpu_root_reduction = check_fpu_knobs(args.get("fpuReduction", None),
                                                                      args.get("fpuRootReduction", None))
        # the score-margin utility in every search made for this Coach and in its value targets.
        # Unset: off
        from .replay import check_score_knobs
        self.score_utility, self.score_scale = check_score_knobs(args.get("scoreUtility", None),
                                                                 args.get("scoreScale", None))
        # the self-play temperatures: self-play and the held-out games only.  Unset: off
        from .replay import temperature_knobs_of
        self.temperature_knobs = temperature_knobs_of(args)
        # averaged weights: NNetWrapper's knobs, checked here as well.  With emaDecay set the
        # net that plays, gates and reanalyses is the averaged one (NNetWrapper.yk_net); learn's flow is unchanged
        from .replay import check_ema_knobs
        self.ema_decay, self.ema_every = check_ema_knobs(args.get("emaDecay", 0.0), args.get("emaEvery", 1))
        # legal-move mask: NNetWrapper's knob, checked here as well.  With it set train minimises
        # the valid-only cross-entropy, and the held-out line compares the nets on that loss
        from .replay import check_mask_knobs
        self.mask_illegal = check_mask_knobs(args.get("maskIllegal", False))
        # {"searched", "kept", "sims"} of the last selfPlayExamples (this rank's sims); with forcedPlayoutsK also
        # {"forced_picks", "pruned_visits"}, with fpuReduction {"fpu_unvisited_picks", "fpu_picks"} and with
        # scoreUtility {"utility_terminals"} (this rank's)
        self.last_selfplay = None
        self.last_reanalysis = None  # [{"item", "n", "reanalysed", "n_empty"}] of the last iteration
        # held-out evaluation: holdoutEps more self-play games per iteration, kept out of training
        self.holdout_eps = int(args.get("holdoutEps", 0) or 0)
        if self.holdout_eps < 0:
            raise ValueError(f"holdoutEps must be >= 0, got {args.get('holdoutEps')!r}")
        self.holdoutHistory = []  # one ExampleShard per iteration, the trainExamplesHistory window
        self.last_eval = None     # {"prev": ..., "new": ...} of the last iteration (NNetWrapper.evaluate's dicts;
        #                           with emaDecay also "new_raw": the new net's raw iterate)
        self.eval_history = []
        # the competitor network with the same args (Coach.py:26-27)
        self.pnet = nnet.__class__(game, args) if hasattr(nnet, "train") else None
        self.mcts = MCTS(game, nnet, args)
        self.trainExamplesHistory = []
        self.skipFirstSelfPlay = False
        self._next_env = game.rng.env
        self.last_pit = None

    def _streams(self, n: int) -> int:
        """Allocate n consecutive env ids (game streams); returns the first."""
        base = self._next_env
        self._next_env += n
        return base

    def _engine(self, n):
        prior = "hash" if getattr(self.nnet, "yk_prior", None) == "hash" else "net"
        net = None if prior == "hash" else self.nnet.yk_net()
        return SelfPlayEngine(n, self.args.numMCTSSims, self.args.cpuct, self.args.tempThreshold, net=net,
                              prior=prior, max_moves=GAME_MOVES,
                              # root exploration noise of self-play (off unless both are set; the gating
                              # arena and the MCTS plugin never add it)
                              dirichlet_alpha=self.args.get("dirichletAlpha", 0.0),
                              dirichlet_eps=self.args.get("dirichletEpsilon", 0.0),
                              # each move's root value in the records, only when the value targets use it
                              record_root_values=self._value_targets_on(),
                              # the playout cap; the held-out games are played under the same config
                              playout_fast_sims=self.playout_fast_sims, playout_full_prob=self.playout_full_prob,
                              # forced playouts and pruning; again the same for the held-out games
                              forced_playouts_k=self.forced_k, forced_prune=self.forced_prune,
                              # first-play urgency; the same for the held-out games
                              fpu_reduction=self.fpu_reduction, fpu_root_reduction=self.fpu_root_reduction,
                              # the score-margin utility; the same for the held-out games
                              score_utility=self.score_utility, score_scale=self.score_scale,
                              # the move-selection and root policy temperatures; the same for the held-out games
                              **self.temperature_knobs)

    def _value_targets_on(self) -> bool:
        return (self.value_mix, self.value_lambda) != (0.0, 1.0)

    def executeEpisodes(self, n: int):
        """n episodes as the reference's per-game lists of (YachtState, pi, v) (this process only)."""
        eng = self._engine(n)
        eng.run(self.game.rng.seed, self._streams(n))
        rec = eng.records()
        eng.close()
        return examples_from_records(rec, n)

    def executeEpisode(self):
        return self.executeEpisodes(1)[0]

    def selfPlayExamples(self, n: int, maxlen: int = None):
        """One iteration's self-play (Coach.py:84-90) on every rank: game k of the n uses stream
        env0 + k and is played by rank k // ceil(n / world); the records are all-gathered and
        become the pooled ExampleShard (the last `maxlen` examples, the deque's maxlen)."""
        from . import dist as D
        from .replay import examples_from_images
        rank, world = D.rank_world()
        base = self._streams(n)
        c, lo, _hi = D.shard(n, rank, world)
        eng = self._engine(c)
        try:
            eng.run(self.game.rng.seed, base + lo)
            img = eng.pack_records()
            st = eng.stats()
            sims_run = st["sims"]
        finally:
            eng.close()
        gathered = D.allgather_records(img)
        shard = examples_from_images(gathered, c, GAME_MOVES, self.args.numMCTSSims, n_games=n, maxlen=maxlen,
                                     value_mix=self.value_mix, value_lambda=self.value_lambda,
                                     full_only=self.playout_fast_sims > 0, score_utility=self.score_utility,
                                     score_scale=self.score_scale)
        self.last_selfplay = dict(searched=shard.n_searched, kept=len(shard), sims=sims_run)
        forced = ""
        if self.forced_k > 0:
            self.last_selfplay.update(forced_picks=st["forced_picks"], pruned_visits=st["pruned_visits"])
            forced = ", %d forced root picks, %d visits pruned" % (st["forced_picks"], st["pruned_visits"])
        if self.fpu_reduction is not None:
            self.last_selfplay.update(fpu_unvisited_picks=st["fpu_unvisited_picks"], fpu_picks=st["fpu_picks"])
            forced += ", %d of %d first-play-urgency picks unvisited" % (st["fpu_unvisited_picks"], st["fpu_picks"])
        if self.score_utility is not None:
            self.last_selfplay.update(utility_terminals=st["utility_terminals"])
            forced += ", %d terminal descents returned a score utility" % st["utility_terminals"]
        log.info("SELF-PLAY %d moves searched, %d examples kept, %d lock-step sims run (this rank)%s"
                 % (shard.n_searched, len(shard), sims_run, forced))
        return shard

    def reanalyseWindow(self, iteration: int):
        """The reanalysis of iteration `iteration`: every item of trainExamplesHistory but the
        newest - whose targets the current net's search has just made - that is an ExampleShard with policies
        has the rows yk_reanalyse_select names for (game seed, key = iteration, index_base = the item's offset
        among the window's examples) searched again with self.nnet and is replaced in the list.  The root of
        row j of an item's selection draws from stream _streams(m) + j.  Every rank runs all of it: the ranks
        hold the same window and the same net and the search is exact, so they stay identical."""
        from .replay import ExampleShard, _count_examples, reanalyse, reanalyse_select
        prior = "hash" if getattr(self.nnet, "yk_prior", None) == "hash" else "net"
        net = None if prior == "hash" else self.nnet.yk_net()
        report, base, warned = [], 0, False
        H = self.trainExamplesHistory
        for j, item in enumerate(H[:-1]):
            n = _count_examples(item)
            if not isinstance(item, ExampleShard) or item.policies is None:
                if not warned:
                    log.warning("reanalyseFraction is set, but the window holds examples that are not device "
                                "shards with policies (a loaded examples file): they are not reanalysed")
                    warned = True
            elif n:
                idx = reanalyse_select(n, self.game.rng.seed, iteration, self.reanalyse_fraction, index_base=base)
                m = int(idx.numel())
                if m:
                    H[j] = reanalyse(item, idx, net=net, prior=prior, sims=self.reanalyse_sims,
                                     cpuct=self.args.cpuct, seed=self.game.rng.seed, env_base=self._streams(m),
                                     fpu_reduction=self.fpu_reduction, fpu_root_reduction=self.fpu_root_reduction,
                                     score_utility=self.score_utility, score_scale=self.score_scale)
                    report.append(dict(item=j, n=n, reanalysed=m, n_empty=H[j].reanalysis["n_empty"]))
            base += n
        self.last_reanalysis = report
        return report

    # ---- Coach.learn (Coach.py:74-139)
    def learn(self):
        """numIters iterations: numEps self-play episodes (sharded over the ranks), the replay
        history (numItersForTrainExamplesHistory iterations), NNetWrapper.train, then
        arenaCompare games of the previous net against the new one (MCTS temp 0 each),
        accepting the new net when it wins >= updateThreshold of the decided games.  Rank 0
        writes the files; every rank reads the checkpoints back, so all ranks stay identical."""
        from . import dist as D
        from .arena import GatingArena
        import time

        import torch
        a = self.args
        rank, _world = D.rank_world()

        def clock():
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            return time.perf_counter()
        for i in range(1, a.numIters + 1):
            log.info(f"Starting Iter #{i} ...")
            t = {"t0": clock()}  # phase wall times of this iteration (self.phase_times)
            if not self.skipFirstSelfPlay or i > 1:
                self.trainExamplesHistory.append(self.selfPlayExamples(a.numEps, maxlen=a.maxlenOfQueue))
            t["selfplay"] = clock()
            if self.holdout_eps:  # its own consecutive streams, right after the iteration's self-play games
                self.holdoutHistory.append(self.selfPlayExamples(self.holdout_eps))
                del self.holdoutHistory[:-a.numItersForTrainExamplesHistory]
                t["holdout"] = clock()
            if len(self.trainExamplesHistory) > a.numItersForTrainExamplesHistory:
                log.warning(f"Removing the oldest entry in trainExamples. len(trainExamplesHistory) = "
                            f"{len(self.trainExamplesHistory)}")
                self.trainExamplesHistory.pop(0)
            if self.reanalyse_fraction > 0.0:  # stale targets of the older iterations, before they are saved
                self.reanalyseWindow(i)
                t["reanalyse"] = clock()
            if rank == 0:
                self.saveTrainExamples(i - 1)
                self.nnet.save_checkpoint(folder=a.checkpoint, filename="temp.pth.tar")
            D.barrier()
            self.pnet.load_checkpoint(folder=a.checkpoint, filename="temp.pth.tar")
            t["save"] = clock()
            # the reference shuffles the pooled examples here (Coach.py:104-108) and its
            # DataLoader(shuffle=True) reshuffles every epoch; train's per-epoch permutation is
            # that reshuffle
            self.nnet.train(self.trainExamplesHistory)
            t["train"] = clock()
            if self.holdout_eps:  # every rank: the ranks hold the same nets and the same pooled games
                self.last_eval = {"prev": self.pnet.evaluate(self.holdoutHistory),
                                  "new": self.nnet.evaluate(self.holdoutHistory)}
                self.eval_history.append(self.last_eval)
                pe, ne = self.last_eval["prev"], self.last_eval["new"]
                raw = ""
                if self.ema_decay > 0.0:  # what the average does: the same examples under the raw iterate
                    self.last_eval["new_raw"] = self.nnet.evaluate(self.holdoutHistory, weights="raw")
                    raw = " ; NEW raw loss %.4f" % self.last_eval["new_raw"]["loss"]
                if self.mask_illegal:  # (evaluate follows args.maskIllegal: the loss being trained)
                    raw += " ; policy terms over the valid actions only (maskIllegal)"
                log.info("HELD-OUT %d examples, PREV / NEW : loss %.4f / %.4f ; policy_ce %.4f / %.4f ; top1 %.4f / "
                         "%.4f ; value_mse %.4f / %.4f%s" % (ne["n"], pe["loss"], ne["loss"], pe["policy_ce"],
                                                            ne["policy_ce"], pe["top1"], ne["top1"],
                                                            pe["value_mse"], ne["value_mse"], raw))
                t["eval"] = clock()
            log.info("PITTING AGAINST PREVIOUS VERSION")
            pwins, nwins, draws = GatingArena(self.game, self.pnet, self.nnet, a).playGames(
                a.arenaCompare, env_base=self._streams(2 * int(a.arenaCompare / 2)))
            t["arena"] = clock()
            log.info("NEW/PREV WINS : %d / %d ; DRAWS : %d" % (nwins, pwins, draws))
            D.barrier()  # every rank has read temp.pth.tar before it can be rewritten
            if pwins + nwins == 0 or float(nwins) / (pwins + nwins) < a.updateThreshold:
                log.info("REJECTING NEW MODEL")
                self.nnet.load_checkpoint(folder=a.checkpoint, filename="temp.pth.tar")
            else:
                log.info("ACCEPTING NEW MODEL")
                if rank == 0:
                    self.nnet.save_checkpoint(folder=a.checkpoint, filename=self.getCheckpointFile(i))
                    self.nnet.save_checkpoint(folder=a.checkpoint, filename="best.pth.tar")
            self.last_pit = (pwins, nwins, draws)
            D.barrier()
            t["gate"] = clock()
            keys = [k for k in ("t0", "selfplay", "holdout", "reanalyse", "save", "train", "eval", "arena", "gate")
                    if k in t]
            self.phase_times = {k + "_s": t[k] - t[p] for p, k in zip(keys, keys[1:])}
            if self.holdout_eps:  # eval_s: everything the held-out evaluation adds, its games included
                self.phase_times["eval_s"] += self.phase_times.pop("holdout_s")
            self.phase_times["iteration_s"] = t["gate"] - t["t0"]
        self.wait_saves()

    def getCheckpointFile(self, iteration):
        return "checkpoint_" + str(iteration) + ".pth.tar"

    # ---- the replay buffer on disk (Coach.py:144-170): this framework's npz and, when asked
    # for (examples_format "reference" / "both"), the reference's pickle next to it
    def saveTrainExamples(self, iteration):
        """Coach.py:144-152.  The npz's arrays are copied to the host here; the compressed write
        runs on a background thread (joined before the next write, a load, and at the end of
        learn), so the iteration's training does not wait for the disk."""
        import threading

        from .examples_io import examples_payload, save_reference_examples, write_examples
        folder = self.args.checkpoint
        os.makedirs(folder, exist_ok=True)
        base = os.path.join(folder, self.getCheckpointFile(iteration) + ".examples")
        fmt = self.args.get("examples_format", "npz")  # the dense reference pickle grows ~29 KB / example
        if fmt in ("both", "reference"):
            save_reference_examples(base, self.trainExamplesHistory)
        if fmt in ("both", "npz"):
            payload = examples_payload(self.trainExamplesHistory)
            self.wait_saves()
            self._saver = threading.Thread(target=write_examples, args=(base + ".npz", payload))
            self._saver.start()

    def wait_saves(self):
        """Join the background examples write, if one is running."""
        t = getattr(self, "_saver", None)
        if t is not None:
            t.join()
            self._saver = None

    def loadTrainExamples(self):
        from .examples_io import load_examples, load_reference_examples
        self.wait_saves()
        modelFile = os.path.join(self.args.load_folder_file[0], self.args.load_folder_file[1])
        examplesFile = modelFile + ".examples"
        if os.path.isfile(examplesFile + ".npz"):
            self.trainExamplesHistory = load_examples(examplesFile + ".npz")
        elif os.path.isfile(examplesFile):
            self.trainExamplesHistory = load_reference_examples(examplesFile)
        else:
            log.warning(f'File "{examplesFile}" with trainExamples not found!')
            return
        log.info("Loading done!")
        if self.score_utility is not None:  # (as below: the files hold the outcome only)
            log.warning("scoreUtility is set, but the examples file holds outcomes only: the "
                        f"{len(self.trainExamplesHistory)} reloaded iteration(s) train on outcomes")
        if self._value_targets_on():  # (a resumed run must still start: the files hold the outcome only)
            log.warning("valueMix / valueLambda are set, but the examples file holds outcomes only: the "
                        f"{len(self.trainExamplesHistory)} reloaded iteration(s) train on outcomes")
        if self.holdout_eps:  # (the files hold the training games only)
            log.info("holdoutEps is set: the held-out games are not stored in the examples file, the held-out "
                     "window starts empty")
        self.skipFirstSelfPlay = True  # examples based on the model were already collected
