"""Diagnostic (GPU box): what one pass of the symmetry augmentation (yk_examples_augment, all three
symmetries) costs against the epoch it prepares.  A self-play shard, then in one process

* the augment launch over the whole shard, hard (boards and targets) and soft (with the visit-policy CSR),
  each timed with HIP events, the median of `--launches` launches after a warm-up launch;
* the same shard's one-epoch train time at `--batch`, AMP - hard and soft targets - HIP events around the
  epoch's back-to-back steps (after `--warmup` steps).

    python tools/time_augment.py [--envs 4096] [--sims 25] [--batch 512] [--launches 5] [--out FILE.json]
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
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402
from yacht_amd.replay import as_device_policies, examples_from_images  # noqa: E402
from yacht_amd.train import Trainer  # noqa: E402

NAMES = ("carry", "rolls", "groups")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096, help="self-play games behind the shard")
    ap.add_argument("--sims", type=int, default=25)
    ap.add_argument("--temp-threshold", type=int, default=15)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20, help="train steps before the timed epoch")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    sd = YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict()
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, a.temp_threshold, net=YkNet(sd, a.hidden, a.nblocks), max_moves=48)
    eng.run(0, 0)
    shard = examples_from_images(eng.pack_records(), a.envs, 48, a.sims)
    eng.close()
    S, T, V, pol = shard.states, shard.targets, shard.values, as_device_policies(shard)
    n, nnz = len(shard), int(pol[0][-1])
    K.check_policy_columns(pol)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed_augment(policies):
        out = K.augment_examples(S, T, policies, 0, 0, NAMES)  # warm-up; its tensors are reused
        ms = []
        for r in range(a.launches):
            torch.cuda.synchronize()
            e0.record()
            K.augment_examples(S, T, policies, 0, r + 1, NAMES, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, out

    aug_hard, _ = timed_augment(None)
    aug_soft, out = timed_augment(pol)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
    idx = [perm[j:j + a.batch].contiguous() for j in range(0, n, a.batch)]

    def timed_epoch(soft):
        tr = Trainer(sd, a.hidden, a.nblocks, max_batch=a.batch, dropout=0.3, amp=True)
        step = lambda i: tr.step(out[0], out[1], V, idx=i, policies=out[2] if soft else None)
        for i in idx[:a.warmup]:
            step(i)
        torch.cuda.synchronize()
        e0.record()
        for i in idx:
            step(i)
        e1.record()
        e1.synchronize()
        tr.close()
        return e0.elapsed_time(e1)

    ep_hard, ep_soft = timed_epoch(False), timed_epoch(True)
    med = statistics.median
    res = {"config": {"examples": n, "policy_entries": nnz, "batch": a.batch, "steps_per_epoch": len(idx),
                      "launches": a.launches, "hidden": a.hidden, "nblocks": a.nblocks, "amp": True, "dropout": 0.3,
                      "symmetries": list(NAMES),
                      "shard": f"{a.envs} self-play games x {a.sims} sims, {a.temp_threshold} moves at temperature 1",
                      "method": "HIP events around each augment launch over the whole shard (median of the launches, "
                                "after one warm-up launch) and around one epoch's back-to-back train steps, same process",
                      "device": torch.cuda.get_device_name(0)},
           "augment_hard_ms": {"median": med(aug_hard), "launches": aug_hard},
           "augment_soft_ms": {"median": med(aug_soft), "launches": aug_soft},
           "epoch_hard_ms": ep_hard, "epoch_soft_ms": ep_soft,
           "augment_share_of_epoch": {"hard": med(aug_hard) / ep_hard, "soft": med(aug_soft) / ep_soft}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
