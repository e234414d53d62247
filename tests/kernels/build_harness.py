"""TEST INFRASTRUCTURE ONLY: builds tests/kernels/libwn_kernel_harness.so, the one library of the kernel-level tests: the product's kernels
launched one at a time through their own launchers (wn_kernel_harness.hip includes csrc/wn_runtime.hip, once).  Same compiler and flags as the
product's runtime unit (pytorch-wavenet_amd/build.py), linked with an object of wn_stacked.hip.  The product package never loads it.

    python tests/kernels/build_harness.py          # build if stale
    python tests/kernels/build_harness.py --force
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "pytorch-wavenet_amd")
CSRC = os.path.join(PKG, "csrc")
OUT = os.path.join(HERE, "libwn_kernel_harness.so")
SRC = os.path.join(HERE, "wn_kernel_harness.hip")


def _deps():
    return [SRC, os.path.join(ROOT, "include", "wn_abi.h")] + sorted(
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inl")))


def build_harness(force=False, verbose=False, out=OUT):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import build as wn_build   # the product's compiler and flags
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in _deps()):
        return out
    hipcc = wn_build.hipcc_path()
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-inline-asm"]
    with tempfile.TemporaryDirectory() as tmp:
        units = [(SRC, wn_build.ALIGN_FLAGS), (os.path.join(CSRC, "wn_stacked.hip"), [])]   # (the runtime unit's flags, and the stacked unit's)
        cmds, objs = [], []
        for i, (src, extra) in enumerate(units):
            obj = os.path.join(tmp, "unit%d.o" % i)
            cmds.append(common + list(extra) + ["-c", src, "-o", obj])
            objs.append(obj)
            if verbose:
                print(" ".join(cmds[-1]))
        wn_build._compile_all(cmds)   # two compiles side by side, no more
        tmp_so = os.path.join(tmp, "lib.so")
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp_so] + objs
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link)
        _move(tmp_so, out)   # (the temporary directory may sit on another file system)
    return out


def _move(src, dst):
    part = dst + ".tmp%d" % os.getpid()
    with open(src, "rb") as f, open(part, "wb") as g:
        g.write(f.read())
    os.replace(part, dst)


if __name__ == "__main__":
    print(build_harness(force="--force" in sys.argv, verbose=True))
