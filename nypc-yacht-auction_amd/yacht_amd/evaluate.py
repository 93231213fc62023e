"""Score a checkpoint on an examples file: ``python -m yacht_amd.evaluate --model CKPT --examples FILE``.

Prints one JSON line, the dict of ``NNetWrapper.evaluate``: forward only, dropout off, the
policy against each example's target (``--target argmax``: the hard label; ``visits``: the full visit
policy) and the value against the outcome.  CKPT is a checkpoint in the reference's format
(``NNetWrapper.save_checkpoint``; its ``args`` entry gives the net's size), FILE an examples file in either
format (examples_io: this framework's ``.npz``, or the reference's pickle, read without running code from it).
``--weights ema`` scores the checkpoint's averaged weights (its ``ema_state_dict`` entry, written when the run
had ``emaDecay`` set) instead of its ``state_dict``.  ``--masked`` gives the policy numbers over each example's valid actions only
(the legal-move mask); without it they follow the checkpoint's ``maskIllegal``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def load_examples_file(path: str):
    """An examples file in either format -> list (iterations) of lists of (YachtState, pi, v)."""
    import zipfile

    from .examples_io import load_examples, load_reference_examples
    return load_examples(path) if zipfile.is_zipfile(path) else load_reference_examples(path)


def evaluate_files(model: str, examples: str, target: str = None, weights: str = "raw", masked=None) -> dict:
    import torch

    from .game import YachtGame
    from .nnet import DEFAULT_ARGS, NNetWrapper
    from .utils import dotdict
    if weights not in ("raw", "ema"):
        raise ValueError(f"weights must be raw or ema, not {weights!r}")
    ck = torch.load(model, map_location="cpu", weights_only=True)
    if weights == "ema" and "ema_state_dict" not in ck:
        raise KeyError(f"--weights ema: {model} has no 'ema_state_dict' entry (it was written without emaDecay)")
    args = dotdict(DEFAULT_ARGS)
    args.update(ck.get("args", {}) if "state_dict" in ck else {})
    net = NNetWrapper(YachtGame(0), args)
    folder, filename = os.path.split(os.path.abspath(model))
    net.load_checkpoint(folder=folder, filename=filename)
    target = net.eval_target(target)  # (a bad name fails before the file is read)
    if weights == "ema":
        net._set_shadow(ck["ema_state_dict"], int(ck.get("ema_updates", 0)))
    return net.evaluate(load_examples_file(examples), target=target, weights=weights, masked=masked)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m yacht_amd.evaluate",
                                 description="Held-out evaluation of a checkpoint on an examples file (MI355X)")
    ap.add_argument("--model", required=True, help="reference-format checkpoint (state_dict + args)")
    ap.add_argument("--examples", required=True, help="examples file: the .npz or the reference's pickle")
    ap.add_argument("--target", choices=("argmax", "visits"), default=None,
                    help="the policy term of `loss` (default: the checkpoint's policy_target, else argmax)")
    ap.add_argument("--weights", choices=("raw", "ema"), default="raw",
                    help="raw: the checkpoint's state_dict (default); ema: its averaged weights (ema_state_dict)")
    ap.add_argument("--masked", action="store_true", default=None,
                    help="policy numbers over each example's valid actions only (default: the checkpoint's "
                         "maskIllegal, else off)")
    a = ap.parse_args(argv)
    try:
        out = evaluate_files(a.model, a.examples, a.target, a.weights, a.masked)
    except KeyError as e:
        ap.error(e.args[0])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
