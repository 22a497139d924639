"""The stripe layout of the batched calls (clay_amd/csrc/stripe_layout.hpp) on the host: no GPU.

tests/host/stripe_layout_check.cpp includes the header the engine uses and checks, for families of
1..6 operands per stripe and 1..9 stripes over odd, negative and zero strides, both forms (pointer
arrays, strides): that at() equals its defining formula, that pointer arrays built from a strided
layout are reported uniform with that stride for every subset of operands, that moving one entry
of a listed operand makes them non-uniform while an entry of an operand outside the subset does
not, and the strides reported for a single stripe.  The answer selects between a single-launch
kernel and a pointer table, so it is pinned here.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stripe_layout_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_layout_forms_and_uniform_stride(tmp_path):
    exe = str(tmp_path / "stripe_layout_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("stripe layout ok:"), r.stdout[-2000:]
