"""Host builds of the kernels for the simulator tests: tests/native/sim_<stem>.cpp compiled with g++ into
tests/native/build/libsim_<stem>.so and loaded with ctypes.  A plain helper module beside the tests."""
import ctypes
import os
import subprocess

from conftest import REPO

# what the lists of dependencies are written with: paths from the repository's root
NAT, CSRC = "tests/native/", "text_alignment_amd/csrc/"
HEADER = "include/text_alignment_amd.h"
HIPSHIM = NAT + "hipshim/hip/hip_runtime.h"


def load(stem, deps, flags=(), include=()):
    """the loaded library of sim_<stem>.cpp, compiled again when it is older than its source or one of `deps` (paths
    from the repository's root, or absolute).  flags: further compiler flags, e.g. -ffp-contract=off; include:
    directories under tests/native for -I (the HIP shims)."""
    native = os.path.join(REPO, NAT)
    src = os.path.join(native, "sim_%s.cpp" % stem)
    so = os.path.join(native, "build", "libsim_%s.so" % stem)
    deps = [src] + [os.path.join(REPO, d) for d in deps]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + list(flags)
        for d in include:
            cmd += ["-I", os.path.join(native, d)]
        subprocess.check_call(cmd + ["-o", so, src])
    return ctypes.CDLL(so)
