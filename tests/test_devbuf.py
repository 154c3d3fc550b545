"""DevBuf (csrc/devbuf.h), the owner of every device allocation of the host engine, exercised by a
stand-alone program (tests/devbuf/devbuf_test.cpp) against counting fakes of the HIP calls it makes:
move-construct, move-assign over a live buffer, reset, re-alloc, a failed allocation, pinned memory and a
growing vector of structs that hold buffers.  Built with AddressSanitizer and UBSan and run on the host:
it must end with allocations equal to frees and no sanitizer report."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mamba.jl_amd", "csrc")


def test_devbuf_ownership(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "devbuf_test")
    # the fakes' hip/hip_runtime.h is found first; devbuf.h is the engine's own
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(HERE, "devbuf"), "-I", CSRC,
           os.path.join(HERE, "devbuf", "devbuf_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed checks" in r.stdout and r.stderr == "", r.stdout + r.stderr
