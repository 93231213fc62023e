"""csrc/yk_optarg.h on the host: tests/optarg_host.cpp, built as plain C++17 and run once.

* with_opts over three options A, B = (B1, B2), C: for each of the 8 on/off settings the callback runs exactly once,
  with exactly the values of the options that are on, in the order A, B1, B2, C, as those types;
* opt_arg gives the pack's value when the pack has the type and the default when not; get_arg gives the pack's
  element itself (its address);
* args_in over the list (A, C) accepts (), (A), (C), (A, C) and rejects (C, A), (A, A) and a type not in the list."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO


def _compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return [shutil.which(cc)]
    hipcc = shutil.which("hipcc") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("optarg") / "optarg_host")
    src = os.path.join(REPO, "tests", "optarg_host.cpp")
    p = subprocess.run(cc + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout.splitlines()


def test_with_opts_calls_once_with_the_on_values_in_order(lines):
    got = [ln for ln in lines if ln.startswith("with_opts ")]
    want = []
    for m in range(8):
        a, b, c = (m >> 2) & 1, (m >> 1) & 1, m & 1
        on = [("A", 10 + m)] * a + [("B1", 20 + m), ("B2", 30 + m)] * b + [("C", 40 + m)] * c
        want.append("with_opts %d%d%d calls=1 types=%s values=%s" % (a, b, c, "".join(t + "," for t, _ in on),
                                                                     "".join("%d," % v for _, v in on)))
    assert got == want


def test_opt_arg_get_arg_and_the_order_check(lines):
    assert "opt_arg present=3 first=1 absent=-1 empty=-2" in lines
    assert "get_arg same=1 1" in lines
    assert "args_in ()=1 (A)=1 (C)=1 (A,C)=1 (C,A)=0 (A,A)=0 (B1)=0" in lines
    assert len(lines) == 11
