"""Diagnostic (GPU box): what the legal-move mask (args.maskIllegal) costs per train step.
A self-play shard (its examples keep the mask's contract), then the native step at one batch size in four
variants - f32 / amp x unmasked / masked - each timed with HIP events around runs of back-to-back steps after
a warm-up, the median over the rounds reported with the masked / unmasked ratio per mode.  The variants take
turns round by round, so clock or thermal drift lands on all four alike; the unmasked step of the same call
is the baseline (its kernels are the ones a build without the mask launches).

    python tools/time_legal_mask.py [--batch 512] [--steps 50] [--rounds 15] [--warmup 20] [--soft] [--out FILE.json]

Where the difference goes, kernel by kernel: one variant alone under the profiler, once per variant,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_legal_mask.py --child amp_masked
and the two kernel_stats tables side by side (k_legal_bits is the extra launch, k_amp_head / k_loss the masked
instantiations).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50, help="back-to-back steps per timed run")
    ap.add_argument("--rounds", type=int, default=15, help="timed runs per variant")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=256, help="self-play games behind the shard")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--soft", action="store_true", help="train on the visit policies (policy_target visits)")
    ap.add_argument("--child", default=None, choices=["f32_unmasked", "f32_masked", "amp_unmasked", "amp_masked"],
                    help="run warmup + steps x rounds steps of this variant alone and stop (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    sd = YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict()
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 48, net=YkNet(sd, a.hidden, a.nblocks), max_moves=48)
    eng.run(0, 0)
    shard = examples_from_images(eng.pack_records(), a.envs, 48, a.sims)
    eng.close()
    S, T, V, pol = shard.states, shard.targets, shard.values, as_device_policies(shard)
    n = len(shard)
    assert K.check_legal(S, T, pol) == (-1, 0)  # the engine's records keep the contract
    nvalid = K.valid_mask(S, 1)[1].double()
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
    idx = [perm[j:j + a.batch].contiguous() for j in range(0, n - a.batch + 1, a.batch)]
    variants = [(amp, mask) for amp in (False, True) for mask in (False, True)]
    if a.child:
        variants = [(a.child.startswith("amp"), a.child.endswith("_masked"))]
    tr = {v: Trainer(sd, a.hidden, a.nblocks, max_batch=a.batch, dropout=0.3, amp=v[0], legal_mask=v[1])
          for v in variants}
    step = lambda v, i: tr[v].step(S, T, V, idx=idx[i % len(idx)], policies=pol if a.soft else None)
    for v in variants:
        for i in range(a.warmup):
            step(v, i)
    if a.child:
        for i in range(a.steps * a.rounds):
            step(variants[0], i)
        torch.cuda.synchronize()
        print("done", a.child, tr[variants[0]].losses())
        return
    ms = {v: [] for v in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds):
        for v in variants:
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.steps):
                step(v, r * a.steps + i)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / a.steps)
    res = {"config": {"batch": a.batch, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup, "hidden": a.hidden,
                      "nblocks": a.nblocks, "examples": n, "dropout": 0.3, "targets": "visits" if a.soft else "argmax",
                      "valid_actions_per_example": {"mean": float(nvalid.mean()), "median": float(nvalid.median())},
                      "shard": f"{a.envs} self-play games x {a.sims} sims",
                      "method": "HIP events around runs of `steps` back-to-back steps, the four variants taking "
                                "turns round by round; median (p10, p90) of the rounds' time per step; ratio = "
                                "masked median / unmasked median of the same mode",
                      "device": torch.cuda.get_device_name(0)}}
    for amp, mask in variants:
        x = sorted(ms[(amp, mask)])
        res[("amp" if amp else "f32") + "_" + ("masked" if mask else "unmasked") + "_ms_per_step"] = {
            "median": statistics.median(x), "p10": x[len(x) // 10], "p90": x[(9 * len(x)) // 10], "rounds": x}
    for mode in ("f32", "amp"):
        m, u = res[mode + "_masked_ms_per_step"]["median"], res[mode + "_unmasked_ms_per_step"]["median"]
        res[mode + "_masked_over_unmasked"] = m / u
        res[mode + "_masked_minus_unmasked_us"] = (m - u) * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
