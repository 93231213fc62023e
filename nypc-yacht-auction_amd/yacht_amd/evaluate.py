"""Score a checkpoint on an examples file: ``python -m yacht_amd.evaluate --model CKPT --examples FILE``.

Prints one JSON line, the dict of ``NNetWrapper.evaluate``: forward only, dropout off, the
policy against each example's target (``--target argmax``: the hard label; ``visits``: the full visit
policy) and the value against the outcome.  CKPT is a checkpoint in the reference's format
(``NNetWrapper.save_checkpoint``; its ``args`` entry gives the net's size), FILE an examples file in either
format (examples_io: this framework's ``.npz``, or the reference's pickle, read without running code from it).
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


def evaluate_files(model: str, examples: str, target: str = None) -> dict:
    import torch

    from .game import YachtGame
    from .nnet import DEFAULT_ARGS, NNetWrapper
    from .utils import dotdict
    ck = torch.load(model, map_location="cpu", weights_only=True)
    args = dotdict(DEFAULT_ARGS)
    args.update(ck.get("args", {}) if "state_dict" in ck else {})
    net = NNetWrapper(YachtGame(0), args)
    folder, filename = os.path.split(os.path.abspath(model))
    net.load_checkpoint(folder=folder, filename=filename)
    target = net.eval_target(target)  # (a bad name fails before the file is read)
    return net.evaluate(load_examples_file(examples), target=target)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m yacht_amd.evaluate",
                                 description="Held-out evaluation of a checkpoint on an examples file (MI355X)")
    ap.add_argument("--model", required=True, help="reference-format checkpoint (state_dict + args)")
    ap.add_argument("--examples", required=True, help="examples file: the .npz or the reference's pickle")
    ap.add_argument("--target", choices=("argmax", "visits"), default=None,
                    help="the policy term of `loss` (default: the checkpoint's policy_target, else argmax)")
    a = ap.parse_args(argv)
    print(json.dumps(evaluate_files(a.model, a.examples, a.target)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
