"""Diagnostic (GPU box): what the reanalysis costs.  With the 256 x 6 net (closed-form
weights) at the bench shape:

* one self-play batch of `--envs` games x `--sims` simulations per move, host wall time around each of
  `--calls` batches after a warm-up batch - the yardstick: its time per move of a game, which a user prices
  `reanalyseFraction` against `numEps` with (a self-played move is one search on a tree kept from the move
  before; a reanalysed root is one search on a fresh tree);
* replay.reanalyse of `--roots` examples of that batch's shard, spread evenly over it, `--chunk` roots per
  chunk, `--sims` simulations each, fresh trees: host wall time around each of `--calls` calls after a warm-up
  call, and roots per second;
* the parts of one chunk: yk_mcts_reset + yk_mcts_search (host wall time, synchronised), and the two
  conversions, yk_policies_from_counts on that chunk's counts and yk_policies_splice of its rows into the
  shard's CSR (HIP events around each whole call - both phases, allocation and synchronise included).

    python tools/time_reanalyse.py [--envs 4096] [--sims 100] [--roots 16384] [--chunk 4096] [--calls 3]
                                   [--out profiles/reanalyse.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
sys.path.insert(0, REPO)
from oracle import spec  # noqa: E402
from yacht_amd import kernels as K  # noqa: E402
from yacht_amd import replay as R  # noqa: E402
from yacht_amd._lib import call, stream_ptr  # noqa: E402
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YkNet  # noqa: E402


def wall(f, calls):
    """seconds of each of `calls` calls of f (device synchronised before and after), after one warm-up call."""
    f()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "calls_s": out}


def events(f, calls):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--roots", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reanalyse.py needs a GPU: a timing taken elsewhere says nothing")
    net = YkNet(spec.closed_form_weights(256, 6), 256, 6)
    res = {"config": {"envs": a.envs, "sims": a.sims, "roots": a.roots, "chunk": a.chunk, "calls": a.calls,
                      "net": "256 x 6, closed-form weights, f32-equivalent products", "cpuct": 1.5,
                      "method": "host wall time around synchronised calls, HIP events around the conversions; one "
                                "warm-up call each; medians and every call",
                      "device": torch.cuda.get_device_name(0)}}
    # ---- the yardstick: self-play at the same shape
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=48)
    base = [0]

    def play():
        eng.run(a.seed, base[0])
        base[0] += a.envs
    sp = wall(play, a.calls)
    st = eng.stats()
    img = eng.pack_records()
    eng.close()
    shard = R.examples_from_images(img.reshape(1, -1), a.envs, 48, a.sims)
    del img
    n = len(shard)
    moves = a.envs * 48
    sp["moves"] = moves
    sp["moves_per_s"] = moves / sp["median_s"]
    sp["us_per_move"] = 1e6 * sp["median_s"] / moves
    sp["expansions_last_batch"] = st["expansions"]
    res["selfplay_batch"] = sp
    # ---- the whole reanalysis
    m = min(a.roots, n)
    idx = torch.linspace(0, n - 1, m, dtype=torch.float64, device="cuda").round().to(torch.int32).unique()
    m = int(idx.numel())
    kw = dict(net=net, sims=a.sims, cpuct=1.5, seed=a.seed, env_base=1 << 20, chunk=a.chunk)
    last = {}

    def rean():
        last["out"] = R.reanalyse(shard, idx, **kw)
    ra = wall(rean, a.calls)
    ra["roots"] = m
    ra["roots_per_s"] = m / ra["median_s"]
    ra["us_per_root"] = 1e6 * ra["median_s"] / m
    # (a call's engine creation can dominate it - see chunk_engine below - so the fastest call is given too)
    ra["fastest_s"] = min(ra["calls_s"])
    ra["fastest_roots_per_s"] = m / ra["fastest_s"]
    ra["fastest_us_per_root"] = 1e6 * ra["fastest_s"] / m
    ra["report"] = last["out"].reanalysis
    P0, P1 = shard.policies, last["out"].policies
    ra["entries_per_row_before"] = float(P0["pi_indptr"][-1]) / n
    ra["entries_per_reanalysed_row"] = float((P1["pi_indptr"][1:] - P1["pi_indptr"][:-1])[idx.long()].double().mean())
    ra["rows_changed"] = int(((P1["pi_indptr"][1:] - P1["pi_indptr"][:-1]) !=
                              (P0["pi_indptr"][1:] - P0["pi_indptr"][:-1])).sum())
    res["reanalyse"] = ra
    res["root_over_selfplay_move"] = ra["us_per_root"] / sp["us_per_move"]
    res["fastest_root_over_selfplay_move"] = ra["fastest_us_per_root"] / sp["us_per_move"]
    # ---- the parts of one chunk
    E = min(a.chunk, m)
    cidx = idx[:E].contiguous()
    roots = shard.states.index_select(0, cidx.long()).contiguous()
    env = torch.arange(E, dtype=torch.int32, device="cuda") + (1 << 20)
    counts = torch.empty((E, K.ACTION_SIZE), dtype=torch.int32, device="cuda")
    # (what every replay.reanalyse call pays once: its engine's pools allocated and released)
    made = []

    def create():
        made.append(SelfPlayEngine(E, a.sims, 1.5, net=net, max_moves=1))

    def close():
        made.pop().close()
    tc, tx = [], []
    for _ in range(a.calls + 1):
        for f, out in ((create, tc), (close, tx)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
    res["chunk_engine"] = {"create_s": tc, "close_s": tx, "create_median_s": statistics.median(tc),
                           "close_median_s": statistics.median(tx)}
    eng = SelfPlayEngine(E, a.sims, 1.5, net=net, max_moves=1)

    def search():
        ctr = torch.zeros(E, dtype=torch.int64, device="cuda")
        call("yk_mcts_reset", eng.handle)
        call("yk_mcts_search", eng.handle, roots.data_ptr(), a.seed, env.data_ptr(), ctr.data_ptr(), a.sims,
             counts.data_ptr(), stream_ptr())
    res["chunk_search"] = wall(search, a.calls)
    res["chunk_search"]["roots"] = E
    res["chunk_search"]["us_per_root"] = 1e6 * res["chunk_search"]["median_s"] / E
    res["chunk_search"]["root_over_selfplay_move"] = res["chunk_search"]["us_per_root"] / sp["us_per_move"]
    res["chunk_search"]["expansions"] = eng.stats()["expansions"]
    eng.close()
    res["chunk_from_counts"] = events(lambda: K.policies_from_counts(counts), 5)
    new, _, n_empty = K.policies_from_counts(counts)
    old = (P0["pi_indptr"], P0["pi_cols"], P0["pi_vals"])
    res["chunk_splice"] = events(lambda: K.policies_splice(old, cidx, new), 5)
    res["chunk_splice"]["rows_of_the_csr"] = n
    res["chunk_splice"]["entries_of_the_csr"] = int(P0["pi_indptr"][-1])
    res["chunk_conversions_ms"] = res["chunk_from_counts"]["median_ms"] + res["chunk_splice"]["median_ms"]
    res["chunk_conversions_share_of_search"] = res["chunk_conversions_ms"] / (1e3 * res["chunk_search"]["median_s"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
