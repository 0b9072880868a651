"""The lossless 57-bit tile packing of the group-aligned row pass (pymc_amd/csrc/rows_pack.h), on the host.

`tests/rows_pack_check.cpp` is a stand-alone program around the header: pack -> unpack must return every stored fp64 bit for
bit (N(0,1) values, both window edges, +-0, a denormal, +-1e300, NaN, infinities, exceptions in lane 0 / 63 and slot 0 / 13, several
in one lane, last tiles of 1, 2 and 127 rows), the window chooser must pick [-13, 3) for standard normal data, and a matrix with
a 0/1 dummy column must be declared not eligible.  The program is built with the address and undefined-behaviour sanitizers
when the system compiler has their runtimes.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rows_pack_check.cpp")
INC = os.path.join(ROOT, "pymc_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("rows_pack") / "rows_pack_check")
    base = [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + INC, SRC, "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


@pytest.mark.parametrize("section", ["roundtrip", "window", "eligible"])
def test_rows_pack(exe, section):
    r = subprocess.run([exe, section], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
