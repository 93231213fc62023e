"""tools/diag_sources.py against the sources as they are: every anchor still matches exactly once (the tool
stops otherwise), the three hooked files are written, and each hook define guards text the tool inserted in
the file it belongs to.  Nothing is compiled."""
import importlib.util
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"YK_SEL_TIMING": "yk_engine.hip", "YK_XSPAN": "yk_engine.hip", "YK_TIMING": "yk_fwd.h",
         "YK_AMP_TIMING": "yk_train_amp.hip"}


def test_every_hook_lands(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("diag_sources", os.path.join(REPO, "tools", "diag_sources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["diag_sources.py", str(tmp_path)])
    tool.main()
    for define, name in HOOKS.items():
        with open(os.path.join(tool.SRC, name)) as f:
            product = f.read()
        with open(tmp_path / "csrc" / name) as f:
            hooked = f.read()
        assert define not in product  # the production sources carry no hook
        assert f"#ifdef {define}\n" in hooked
        assert len(hooked) > len(product)
    # the files the tool does not touch are plain copies
    assert sorted(os.listdir(tmp_path / "csrc")) == sorted(os.listdir(tool.SRC))
