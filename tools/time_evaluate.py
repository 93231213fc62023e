"""Diagnostic (GPU box): what the held-out evaluation costs.  One batch of `--envs` self-play
games gives the examples (48 per game); over them, with HIP events around each of `--calls` calls after one
warm-up call, the median of:

* yk_net_evaluate at the default chunk (16384 rows), with and without the policies' CSR;
* yk_net_predict over the same rows in the same 16384-row chunks - the yardstick: the same forward, then
  predict reads every logit and writes 3226 floats per row where evaluate reads every logit and writes 128 B;
* the parts of one chunk: yk_net_logits alone and yk_examples_metrics alone (with / without the CSR).

Then what args.holdoutEps = `--holdout` adds to one Coach iteration (phase_times["eval_s"]) at config 5's
per-GPU arguments (bench.py's coach_iter_leg: 25 sims, hidden 256 x 6): the held-out games' self-play through
Coach.selfPlayExamples plus the evaluation of the previous and the new net on a full window of
numItersForTrainExamplesHistory = 5 such shards, host wall time ending synchronised, the second of two runs.

    python tools/time_evaluate.py [--envs 4096] [--sims 100] [--calls 5] [--holdout 64] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
from yacht_amd._lib import call  # noqa: E402
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402
from yacht_amd.replay import examples_from_images  # noqa: E402

CHUNK = 16384


def timed(f, calls):
    """ms of each of `calls` calls of f (HIP events around each), after one warm-up call."""
    f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "calls_ms": ms}


def holdout_cost(a):
    from yacht_amd.coach import Coach
    from yacht_amd.game import YachtGame
    from yacht_amd.nnet import NNetWrapper
    from yacht_amd.utils import dotdict
    args = dotdict(numIters=1, numEps=8192, tempThreshold=15, updateThreshold=0.55, maxlenOfQueue=200000,
                   numMCTSSims=25, arenaCompare=10, cpuct=1.5, numItersForTrainExamplesHistory=5, lr=2e-3,
                   weight_decay=1e-4, epochs=15, batch_size=512, vloss_weight=1.5, cuda=True, hidden=a.hidden,
                   nblocks=a.nblocks, dropout=0.3, holdoutEps=a.holdout, seed=0)
    game = YachtGame(seed=99, env_id=2 * 10**6)
    torch.manual_seed(1)
    c = Coach(game, NNetWrapper(game, args), args)
    c.pnet.nnet.load_state_dict(c.nnet.nnet.state_dict())
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shard = c.selfPlayExamples(a.holdout)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        window = [shard] * args.numItersForTrainExamplesHistory
        ev = {"prev": c.pnet.evaluate(window), "new": c.nnet.evaluate(window)}
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        runs.append({"selfplay_s": t1 - t0, "evaluate_both_nets_s": t2 - t1, "eval_s": t2 - t0,
                     "window_examples": ev["new"]["n"]})
    return {"holdoutEps": a.holdout, "sims": 25, "first_run": runs[0], "second_run": runs[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--holdout", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=48)
    eng.run(0, 0)
    if eng.stats()["errors"]:
        raise SystemExit(f"engine error flags {eng.stats()['errors']}")
    shard = examples_from_images(eng.pack_records(), a.envs, 48, a.sims)
    eng.close()
    n = len(shard)
    P = shard.policies
    csr = (P["pi_indptr"], P["pi_cols"], P["pi_vals"])
    res = {"config": {"envs": a.envs, "sims": a.sims, "examples": n, "policy_entries": int(csr[1].numel()),
                      "hidden": a.hidden, "nblocks": a.nblocks, "precision": "f32", "chunk": CHUNK,
                      "calls": a.calls, "method": "HIP events around each call after one warm-up call; median",
                      "device": torch.cuda.get_device_name(0)}}
    with_csr = net.evaluate(shard.states, shard.targets, shard.outcomes, policies=csr)
    res["evaluate_result"] = with_csr
    res["evaluate_with_csr"] = timed(lambda: net.evaluate(shard.states, shard.targets, shard.outcomes, policies=csr),
                                     a.calls)
    res["evaluate_without_csr"] = timed(lambda: net.evaluate(shard.states, shard.targets, shard.outcomes), a.calls)
    pi = torch.empty((CHUNK, 3226), dtype=torch.float32, device="cuda")
    v = torch.empty(CHUNK, dtype=torch.float32, device="cuda")

    def predict_all():
        for c0 in range(0, n, CHUNK):
            m = min(CHUNK, n - c0)
            call("yk_net_predict", net.handle, shard.states[c0:c0 + m].data_ptr(), pi.data_ptr(), v.data_ptr(), m, None)
    res["predict_same_rows"] = timed(predict_all, a.calls)
    res["evaluate_over_predict"] = res["evaluate_with_csr"]["median_ms"] / res["predict_same_rows"]["median_ms"]
    # the parts, on the first chunk
    m = min(CHUNK, n)
    logits = torch.empty((m, 3264), dtype=torch.float32, device="cuda")
    sums = (C.c_double * 16)()

    def metrics(p):
        call("yk_examples_metrics", logits.data_ptr(), 3264, v.data_ptr(), shard.states.data_ptr(),
             shard.targets.data_ptr(), shard.outcomes.data_ptr(), *p, None, m, None, sums, None)
    res["one_chunk"] = {
        "rows": m,
        "logits": timed(lambda: call("yk_net_logits", net.handle, shard.states.data_ptr(), logits.data_ptr(),
                                     v.data_ptr(), m, None), a.calls),
        "metrics_with_csr": timed(lambda: metrics([t.data_ptr() for t in csr]), a.calls),
        "metrics_without_csr": timed(lambda: metrics([None] * 3), a.calls),
        "predict": timed(lambda: call("yk_net_predict", net.handle, shard.states.data_ptr(), pi.data_ptr(),
                                      v.data_ptr(), m, None), a.calls)}
    if a.holdout > 0:
        res["holdout"] = holdout_cost(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
