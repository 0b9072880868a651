"""The hand-counted tile loads of `k_rows_ga` (csrc/rows_ga_kernel.h) keep ONE set of registers per tile in flight.

The kernel keeps two tiles in flight; each is requested by an inline-asm statement ahead of the streaming loop and again inside
it.  The compiler does not know the loads are pending: if it gives the request inside the loop other registers than the one ahead
of it, it copies them at the loop's back-edge -- before the data has landed.  That happens when a register-only consumer of the
old tile is scheduled below the request inside the loop (csrc/rows_ga_kernel.h describes the protocol: the packed request names
the stage's sums as inputs, the raw requests rely on the scheduler).  So every instantiation that uses such loads must show
exactly two destination-register signatures among its tile-load statements.
"""

import os
import re
import shutil
import subprocess

import pytest

NEEDED = ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")


def _llvm_tools():
    """The LLVM binutils of the toolchain that builds the engine: next to the hipcc in use, else under ROCM_PATH, else on PATH."""
    import __graft_entry__ as g

    hipcc = os.path.realpath(shutil.which(g.HIPCC) or g.HIPCC)
    root = os.path.dirname(os.path.dirname(hipcc))
    dirs = [os.path.join(root, "lib", "llvm", "bin"), os.path.join(root, "llvm", "bin"), os.path.dirname(hipcc)]
    if os.environ.get("ROCM_PATH"):
        dirs.append(os.path.join(os.environ["ROCM_PATH"], "lib", "llvm", "bin"))
    for d in dirs:
        if all(os.path.exists(os.path.join(d, t)) for t in NEEDED):
            return [os.path.join(d, t) for t in NEEDED]
    found = [shutil.which(t) for t in NEEDED]
    return found if all(found) else None


def test_each_tile_in_flight_keeps_its_registers(tmp_path):
    import __graft_entry__ as g
    from pymc_amd import _lib

    need = _llvm_tools()
    if need is None:
        pytest.skip("LLVM binutils of the ROCm toolchain not found")
    g.build_engine()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([need[0], f"--dump-section=.hip_fatbin={fat}", os.environ.get("PYMC_AMD_LIB", _lib.LIB_PATH), str(tmp_path / "copy.so")])
    subprocess.check_call([need[1], "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    syms = subprocess.check_output([need[2], "-t", co], text=True)
    names = sorted(set(re.findall(r"(_Z\d+k_rows_gaILi8ELi2E\w*6GaArgs)\s*$", syms, flags=re.M)))
    assert len(names) >= 3, names   # eight stored columns, seven, seven packed
    for name in names:
        dis = subprocess.check_output([need[2], "-d", f"--disassemble-symbols={name}", co], text=True).split("\n")
        ins = [l.split("//")[0].strip() for l in dis if l.startswith("\t")]
        # a tile request: consecutive loads through a scalar base, the first of them without an immediate offset
        groups, cur = [], []
        for l in ins:
            m = re.match(r"global_load_(?:dwordx4|dword|ushort) (v\[\d+:\d+\]|v\d+), v\d+, s\[\d+:\d+\]", l)
            if m:
                cur.append(m.group(1))
            else:
                if len(cur) >= 7:
                    groups.append(tuple(cur))
                cur = []
        assert len(groups) >= 4, (name, groups)
        assert len(set(groups)) == 2, (name, sorted(set(groups)))
