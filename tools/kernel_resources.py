#!/usr/bin/env python3
"""Register, spill and scratch figures of the built sweep kernels, from the code object's metadata
(no GPU needed): the gfx950 code object is taken from the in-tree build's sweep.hip.o (or the
object given) and its amdhsa notes are read with llvm-readelf.

  python tools/kernel_resources.py [path/to/sweep.hip.o]

One line per sweep_kernel instantiation: VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch
(private segment) bytes and static LDS bytes, as the compiler recorded them.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mamba.jl_amd", "lib", "obj", "sweep.hip.o")
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj=OBJ):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin.bin"), os.path.join(tmp, "sweep.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj,
                        os.path.join(tmp, "host.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
    out = []
    # one metadata entry per kernel: "- .agpr_count: ..." up to the next entry
    for entry in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        f = dict(re.findall(r"\.(\w+):\s+'?([^'\n]+)'?", ".agpr_count:" + entry))
        out.append(f)
    return out


def factorization_scratch(obj=OBJ):
    """Static counts for sweep_kernel<2,36>: instructions and scratch_ accesses of the whole
    kernel and of the optimistic factorization pass (isa_census.py factorization_steps)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import isa_census as ic
    ic.OBJ = obj
    ins = ic.kernel_instructions(ic.disassemble())
    steps = ic.factorization_steps(ins)
    lo, hi = steps[0][0], steps[-1][1]
    sc = lambda part: sum(1 for mn, _ in part if mn.startswith("scratch_"))  # noqa: E731
    va = lambda part: sum(1 for mn, _ in part if mn.startswith("v_"))  # noqa: E731
    return {"kernel_instructions": len(ins), "kernel_valu": va(ins), "kernel_scratch": sc(ins),
            "factorization_steps": len(steps), "factorization_instructions": hi - lo,
            "factorization_valu": va(ins[lo:hi]), "factorization_scratch": sc(ins[lo:hi])}


if __name__ == "__main__":
    print("sweep_kernel<2,36> static:", factorization_scratch(sys.argv[1] if len(sys.argv) > 1 else OBJ))
    for f in kernels(sys.argv[1] if len(sys.argv) > 1 else OBJ):
        if "sweep_kernel" not in f.get("name", ""):
            continue
        # _Z12sweep_kernelILi<MODEL>ELj<KINDS>EEv9SweepArgs -> sweep_kernel<MODEL,KINDS>
        m = re.search(r"sweep_kernelILi(\d+)ELj(\d+)E", f["name"])
        name = "sweep_kernel<%s,%s>" % m.groups() if m else f["name"]
        print("%-22s vgpr %s agpr %s sgpr %s vgpr_spill %s sgpr_spill %s scratch_bytes %s static_lds_bytes %s" % (
            name, f["vgpr_count"], f["agpr_count"], f["sgpr_count"],
            f["vgpr_spill_count"], f["sgpr_spill_count"], f["private_segment_fixed_size"],
            f["group_segment_fixed_size"]))
