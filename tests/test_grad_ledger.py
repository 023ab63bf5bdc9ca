"""csrc/grad_ledger.h (the per-step gradient ledger of the training tape) is host-only C++: tests/grad_ledger_check.cpp,
a stand-alone program, exercises it under the host compiler's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_grad_ledger_under_sanitizers(tmp_path):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) found")
    exe = str(tmp_path / "grad_ledger_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", os.path.join(HERE, "grad_ledger_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "grad_ledger_check: ok" in run.stdout
