"""Build libclonos_engine.so (gfx950) in-tree with hipcc.

The shared library is the product: the C-ABI in include/clonos_engine.h plus the HIP
kernels.  Every *.cpp and *.hip in csrc/ is compiled, one compile per source, and every *.h
there is a dependency of all of them.  The library is built in-tree (git-ignored), so that it
travels with a snapshot of the repository.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libclonos_engine.so")
# every source and header in csrc/ (sorted), so a new file cannot be forgotten
SOURCES = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".cpp", ".hip")))
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [
    os.path.join(ROOT, "include", "clonos_engine.h")]
ARCH = os.environ.get("CLONOS_OFFLOAD_ARCH", "gfx950")
MAX_COMPILES = 16  # hipcc processes in flight at most


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS)


def _compile_cmd(src: str, obj: str) -> list:
    return [
        hipcc(),
        "-x", "hip",
        f"--offload-arch={ARCH}",
        "-O3",
        "-std=c++17",
        "-fPIC",
        "-Wall",
        "-Wno-unused-function",
        "-Wno-unused-value",
        "-I", os.path.join(ROOT, "include"),
        "-c", src,
        "-o", obj,
    ]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every source whose object is older than it or any header (all of them with
    force), MAX_COMPILES at a time, then link."""
    if not force and not needs_build():
        return LIB
    hdr_t = max(os.path.getmtime(h) for h in HEADERS)
    objs, procs, bad = [], [], []
    for src in SOURCES:
        obj = os.path.join(CSRC, os.path.basename(src) + ".o")
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(hdr_t, os.path.getmtime(src)):
            continue
        cmd = _compile_cmd(src, obj)
        if verbose:
            print(" ".join(cmd), flush=True)
        if len(procs) == MAX_COMPILES:  # the running set is full: wait for its oldest
            done_src, p = procs.pop(0)
            if p.wait() != 0:
                bad.append(done_src)
        procs.append((src, subprocess.Popen(cmd)))
    bad += [src for src, p in procs if p.wait() != 0]
    if bad:
        raise RuntimeError(f"hipcc failed for {bad}")
    link = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
