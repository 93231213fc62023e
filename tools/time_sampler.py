"""Diagnostic (GPU box): what the weighted minibatch sampling costs.  On a synthetic
per-row table of `--shards` x `--shard` examples (config 5's steady-state window: 5 x 196,608) and
`--steps` x `--batch` draws (one round), with HIP events around each of `--calls` calls after one warm-up
call, the median and every call of:

* K.sample_weights (recency 0.5 per shard, surprise 0.5), K.sample_cdf and K.sample_draw;
* the yardsticks on the same box and tensors: torch.randperm(n), which the default path pays per epoch, and
  torch.cumsum + torch.searchsorted over the same weights for as many float64 uniforms - the off-the-shelf
  form (searchsorted alone is timed too: it is what sample_draw is compared with, though sample_draw also
  makes its uniforms; torch.rand + the scaling + searchsorted is the like-for-like figure).

YK_LIB_PATH picks another build of the library to compare (an A/B); `--label` names it in the output.

    python tools/time_sampler.py [--shards 5] [--shard 196608] [--steps 400] [--batch 512] [--calls 5]
                                 [--label NAME] [--out profiles/sampler.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
from yacht_amd import kernels as K  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=5)
    ap.add_argument("--shard", type=int, default=196608)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sampler.py needs a GPU: a timing taken elsewhere says nothing")
    n, m = a.shards * a.shard, a.steps * a.batch
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rows = torch.randn((n, 16), generator=g, dtype=torch.float64, device="cuda")
    rows[:, 5] = 1.0
    rows[:, 7] = 3 * torch.rand(n, generator=g, dtype=torch.float64, device="cuda")
    rows[:, 6] = rows[:, 7] + torch.rand(n, generator=g, dtype=torch.float64, device="cuda") ** 2
    lens = [a.shard] * a.shards
    fac = [0.5 ** (a.shards - 1 - s) for s in range(a.shards)]
    res = {"config": {"examples": n, "shards": a.shards, "draws": m, "steps": a.steps, "batch": a.batch,
                      "calls": a.calls, "label": a.label, "library": os.environ.get("YK_LIB_PATH", "in-tree"),
                      "method": "HIP events around each call after one warm-up call; median",
                      "device": torch.cuda.get_device_name(0)}}
    w, ksum = K.sample_weights(rows, lens, fac, 0.5)
    cdf, total = K.sample_cdf(w)
    idx = K.sample_draw(cdf, 7, 0, 0, m)
    counts = torch.bincount(idx.long(), minlength=n).double()
    per_shard = counts.reshape(a.shards, a.shard).sum(1) / m
    res["check"] = {"K": ksum, "total": total, "drawn_share_per_shard": per_shard.tolist(),
                    "weight_share_per_shard": (w.reshape(a.shards, a.shard).sum(1) / total).tolist()}
    out = torch.empty(m, dtype=torch.int32, device="cuda")
    res["sample_weights"] = timed(lambda: K.sample_weights(rows, lens, fac, 0.5), a.calls)
    res["sample_weights_recency_only"] = timed(lambda: K.sample_weights(None, lens, fac, 0.0), a.calls)
    res["sample_cdf"] = timed(lambda: K.sample_cdf(w), a.calls)
    res["sample_draw"] = timed(lambda: K.sample_draw(cdf, 7, 0, 0, m, out=out), a.calls)
    # the yardsticks
    res["torch_randperm"] = timed(lambda: torch.randperm(n, generator=g, device="cuda"), a.calls)
    u = torch.rand(m, generator=g, dtype=torch.float64, device="cuda")
    cs = torch.cumsum(w, 0)
    t = u * cs[-1]
    res["torch_cumsum"] = timed(lambda: torch.cumsum(w, 0), a.calls)
    res["torch_searchsorted"] = timed(lambda: torch.searchsorted(cs, t, right=True), a.calls)
    res["torch_cumsum_searchsorted"] = timed(lambda: torch.searchsorted(torch.cumsum(w, 0), t, right=True), a.calls)
    res["torch_rand_scale_searchsorted"] = timed(
        lambda: torch.searchsorted(cs, torch.rand(m, generator=g, dtype=torch.float64, device="cuda") * cs[-1], right=True),
        a.calls)
    res["draw_over_searchsorted"] = res["sample_draw"]["median_ms"] / res["torch_searchsorted"]["median_ms"]
    res["cdf_plus_draw_ms"] = res["sample_cdf"]["median_ms"] + res["sample_draw"]["median_ms"]
    res["round_steps_ms_at_0.125"] = 0.125 * a.steps
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
