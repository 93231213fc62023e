"""Diagnostic (GPU box): what the averaged (EMA) weights cost the train step.

The shape is bench.py's train leg: YachtNNet 256 x 6, minibatches of 512, dropout 0.3, the AMP trainer and the
float32 one.  Four arms:

    parent   the parent commit's library (--parent-lib, loaded through YK_LIB_PATH), the average off
    off      this tree's library, the average off
    every1   this tree, ema_decay 0.999, ema_every 1
    every4   this tree, ema_decay 0.999, ema_every 4

Each measurement is one fresh child process (a fresh allocator, code loading and clocks), run one after the
other under its own time limit; a failed child ends the run.  A child warms up, then times `--blocks` blocks of
`--steps` back-to-back steps per mode (host wall time around a synchronised block, as bench.py takes it) and
reports every block and the median.  The arms alternate within a call, `--rounds` rounds, the order rotated from
round to round, so drift of the machine hits all alike.  Nothing is asserted: the JSON holds every child's
numbers, each arm's spread over its rounds, the paired difference of `off` against `parent` round by round
beside the parent's own spread, and what `every1` / `every4` add to `off`.

    python tools/time_ema.py --parent-lib PATH/libyacht_hip.so [--rounds 3] [--steps 1000] [--blocks 5]
                             [--out profiles/ema.json]

The kernel's own time comes from a run of its own (no counters in it):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_ema.py --child every1 --steps 200 --blocks 1
    python tools/time_ema.py --kernel-stats DIR/.../*_kernel_stats.csv [--merge profiles/ema.json]

which prints k_ema's mean duration, its 12 x nparams bytes over that time and the fraction of bench.py's
HBM peak (HBM_PEAK_GBS).
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
ARMS = ("parent", "off", "every1", "every4")
HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak (HBM3E spec)
H, NB, BATCH, DECAY = 256, 6, 512, 0.999


def nparams(h=H, nb=NB):
    return h * 59 + 3 * h + nb * (2 * h * h + 6 * h) + 2 * h + 3226 * h + 3226 + 2 * h + 128 * h + 128 + 128 + 1


def child(a):
    import numpy as np
    import torch
    from yacht_amd import kernels as K
    from yacht_amd.nnet import YachtNNet
    from yacht_amd.train import Trainer
    torch.manual_seed(0)
    sd = YachtNNet(hidden=H, nblocks=NB).state_dict()
    rng = np.random.RandomState(0)
    n = 16384
    S, _ = K.init_board(0, np.arange(n), 0)
    tg = torch.tensor(rng.randint(0, 202, n), dtype=torch.int32, device="cuda")
    vv = torch.tensor(rng.rand(n) * 2 - 1, dtype=torch.float32, device="cuda")
    idx = [torch.arange(j, j + BATCH, dtype=torch.int32, device="cuda") for j in range(0, n - BATCH, BATCH)]
    kw = {"every1": dict(ema_decay=DECAY, ema_every=1), "every4": dict(ema_decay=DECAY, ema_every=4)}.get(a.child, {})
    library = "the parent commit's (YK_LIB_PATH)" if os.environ.get("YK_LIB_PATH") else "in-tree"
    out = {"arm": a.child, "library": library, "device": torch.cuda.get_device_name(0)}
    for amp in (True, False):
        tr = Trainer(sd, H, NB, max_batch=BATCH, dropout=0.3, seed=0, amp=amp, **kw)
        out["nparams"] = tr.nparams
        for i in range(a.warmup):
            tr.step(S, tg, vv, idx=idx[i % len(idx)])
        blocks = []
        for _ in range(a.blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                tr.step(S, tg, vv, idx=idx[i % len(idx)])
            torch.cuda.synchronize()
            blocks.append(1000.0 * (time.perf_counter() - t0) / a.steps)
        key = "amp" if amp else "f32"
        out[key] = {"ms_per_step_blocks": blocks, "ms_per_step": statistics.median(blocks)}
        if kw:
            out[key]["ema_state"] = tr.ema_state()
        tr.close()
    print(json.dumps(out))


def kernel_stats(path):
    """k_ema's row of a rocprofv3 kernel_stats csv -> mean time, bytes moved and the fraction of the HBM peak."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_ema" in r["Name"]]
    if not rows:
        raise SystemExit(f"{path}: no k_ema row")
    r = rows[0]
    ns = float(r["AverageNs"])
    b = 12 * nparams()
    return {"kernel": r["Name"], "calls": int(r["Calls"]), "mean_us": ns / 1000.0, "min_us": float(r["MinNs"]) / 1000.0,
            "max_us": float(r["MaxNs"]) / 1000.0, "nparams": nparams(), "bytes": b, "gb_per_s": b / ns,
            "hbm_peak_gb_per_s": HBM_PEAK_GBS, "frac_of_hbm_peak": b / ns / HBM_PEAK_GBS,
            "source": "rocprofv3 --kernel-trace --stats of `tools/time_ema.py --child every1` (AMP and f32 steps, no "
                      "counters in the run)"}


def summary(vals):
    return {"runs": vals, "median": statistics.median(vals), "min": min(vals), "max": max(vals),
            "spread": max(vals) - min(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libyacht_hip.so (arm `parent`)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per mode and child")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--child", choices=ARMS, default=None, help="(internal) time one arm and report")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats csv: report k_ema and stop")
    ap.add_argument("--merge", default=None, help="with --kernel-stats: add the report to this JSON file")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        print(json.dumps(ks))
        if a.merge:
            with open(a.merge) as f:
                res = json.load(f)
            res["kernel"] = ks
            add = res.get("added_by_ema", {}).get("amp", {}).get("every1_minus_off_us")
            if add is not None:
                res["kernel"]["step_time_added_every1_amp_us"] = add
            with open(a.merge, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    arms = [x for x in ARMS if x != "parent" or a.parent_lib]
    if a.parent_lib and not os.path.exists(a.parent_lib):
        raise SystemExit(f"{a.parent_lib}: no such library")
    runs = {x: [] for x in arms}
    order_log = []
    fwd = ["--steps", a.steps, "--blocks", a.blocks, "--warmup", a.warmup]
    for r in range(a.rounds):
        k = r % len(arms)
        order = arms[k:] + arms[:k]  # rotated: every arm runs first, in the middle and last
        order_log.append(list(order))
        for arm in order:  # a fresh process each, one at a time: this one never opens the GPU
            env = dict(os.environ)
            env.pop("YK_LIB_PATH", None)
            if arm == "parent":
                env["YK_LIB_PATH"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm] + [str(x) for x in fwd],
                               capture_output=True, text=True, timeout=a.child_timeout, env=env)
            if p.returncode != 0:  # nothing more is started on the GPU after a failed child
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"child {arm} failed with status {p.returncode}")
            runs[arm].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"config": {"hidden": H, "nblocks": NB, "batch": BATCH, "dropout": 0.3, "ema_decay": DECAY,
                      "rounds": a.rounds, "steps": a.steps, "blocks": a.blocks, "warmup": a.warmup,
                      "nparams": runs["off"][0]["nparams"], "ema_bytes_per_update": 12 * runs["off"][0]["nparams"],
                      "device": runs["off"][0]["device"], "order": order_log,
                      "method": "host wall time around synchronised blocks of back-to-back Trainer.step calls; a "
                                "child's ms_per_step is the median of its blocks; one fresh child process per "
                                "measurement, one at a time, the arms' order rotated from round to round"},
           "ms_per_step": {}, "added_by_ema": {}, "children": runs}
    for mode in ("amp", "f32"):
        ms = {arm: summary([c[mode]["ms_per_step"] for c in runs[arm]]) for arm in arms}
        res["ms_per_step"][mode] = ms
        off = ms["off"]["runs"]
        res["added_by_ema"][mode] = {
            "every1_minus_off_us": 1000.0 * statistics.median([x - y for x, y in zip(ms["every1"]["runs"], off)]),
            "every4_minus_off_us": 1000.0 * statistics.median([x - y for x, y in zip(ms["every4"]["runs"], off)]),
            "every1_minus_off_us_rounds": [1000.0 * (x - y) for x, y in zip(ms["every1"]["runs"], off)],
            "every4_minus_off_us_rounds": [1000.0 * (x - y) for x, y in zip(ms["every4"]["runs"], off)]}
        if "parent" in ms:
            d = [1000.0 * (x - y) for x, y in zip(off, ms["parent"]["runs"])]
            res.setdefault("off_against_parent", {})[mode] = {
                "paired_difference_us_rounds": d, "paired_difference_us_median": statistics.median(d),
                "parent_spread_us": 1000.0 * ms["parent"]["spread"],
                "inside_parent_spread": abs(statistics.median(d)) <= 1000.0 * ms["parent"]["spread"]}
    print(json.dumps({k: v for k, v in res.items() if k != "children"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
