"""Diagnostic (GPU box): what the search-value targets (record_root_values) cost.  Two engines
on the same net and the same arena size, root values off and on, play whole episode batches in turns (off, on,
off, on, ...), each batch timed on the host around SelfPlayEngine.run (which ends synchronised); the median
batch time of each and their ratio are reported, and the two engines' records are compared (the flag must not
change them).  Then one yk_examples_value_targets pass over the flag-on batch's packed image is timed: HIP
events around back-to-back calls (each call allocates and frees its offsets and synchronises, as the replay
path uses it), beside yk_examples_from_records' pass over the same image.

    python tools/time_value_targets.py [--envs 4096] [--sims 100] [--rounds 5] [--warmup 1] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
from yacht_amd._lib import call  # noqa: E402
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5, help="timed episode batches per variant")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.9)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    entries = a.sims * 9000 + 65536  # both engines alike (the automatic size depends on the free memory)
    eng = {name: SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=48, arena_entries=entries, **kw)
           for name, kw in (("off", {}), ("on", dict(record_root_values=True)))}
    sec = {name: [] for name in eng}
    exps = {}
    for r in range(a.warmup + a.rounds):
        for name, e in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.run(r, 0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = e.stats()
            if st["errors"]:
                raise SystemExit(f"engine error flags {st['errors']} ({name})")
            if r >= a.warmup:
                sec[name].append(dt)
                exps[name] = st["expansions"]
    # the last batch of each: the same seed, so the same records but for the root-value word
    rec = {name: e.records() for name, e in eng.items()}
    same = all(np.array_equal(rec["on"][k], rec["off"][k]) for k in rec["off"] if k != "info")
    same = same and np.array_equal(rec["on"]["info"][..., :7], rec["off"]["info"][..., :7])
    words = rec["on"]["info"][..., 7]
    img = eng["on"].pack_records().reshape(1, -1)
    for e in eng.values():
        e.close()
    n = int(rec["on"]["n_moves"].sum())
    vals = torch.empty(n, dtype=torch.float32, device="cuda")
    rootv = torch.empty(n, dtype=torch.float32, device="cuda")
    states = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    targets = torch.empty(n, dtype=torch.int32, device="cuda")
    out = C.c_int64()

    def targets_pass():
        call("yk_examples_value_targets", img.data_ptr(), 1, a.envs, 48, a.sims, -1, 0, n, a.beta, a.lam,
             vals.data_ptr(), rootv.data_ptr(), C.byref(out), None)

    def examples_pass():
        call("yk_examples_from_records", img.data_ptr(), 1, a.envs, 48, a.sims, -1, 0, n, states.data_ptr(),
             targets.data_ptr(), vals.data_ptr(), C.byref(out), None)

    passes = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, f in (("value_targets", targets_pass), ("examples_from_records", examples_pass)):
        f()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            f()
        e1.record()
        e1.synchronize()
        passes[f"{name}_ms_per_call"] = e0.elapsed_time(e1) / 10
    med = {name: statistics.median(x) for name, x in sec.items()}
    res = {"config": {"envs": a.envs, "sims": a.sims, "rounds": a.rounds, "warmup": a.warmup, "beta": a.beta,
                      "lambda": a.lam, "hidden": a.hidden, "nblocks": a.nblocks, "arena_entries": entries,
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised), the two "
                                "engines taking turns batch by batch; median of the rounds",
                      "device": torch.cuda.get_device_name(0)},
           "off_s_per_batch": {"median": med["off"], "rounds": sec["off"]},
           "on_s_per_batch": {"median": med["on"], "rounds": sec["on"]},
           "expansions_per_batch": exps,
           "root_values_overhead_percent": 100.0 * (med["on"] / med["off"] - 1.0),
           "records_equal_but_for_the_word": bool(same),
           "words_recorded": int((words != 0).sum()), "moves": n,
           "targets_pass": dict(passes, examples=n,
                                note="one call over the flag-on batch's packed image, allocation of the offsets, "
                                     "the kernel and the closing synchronise included; HIP events around 10 calls")}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
