"""CPU: the engine's host containers on their own -- clonos_amd/csrc/engine_host.h (EpochMap,
SegList, EpochAlloc, EngineLock, WorkPool) compiled with g++ into the stand-alone program
tests/engine_host_main.cpp, once with the address and undefined-behaviour sanitizers and once
with the thread sanitizer.  Each binary runs as a child process; it checks the containers
against std::map / std::vector models itself and must exit 0 with nothing on stderr.

The sanitizer runtimes are linked statically into the program, so it does not depend on the
order in which the process loads its libraries; nothing sanitised is loaded into Python.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"]
SANITIZERS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.mark.parametrize("name", sorted(SANITIZERS))
def test_engine_host_containers(name, tmp_path):
    exe = str(tmp_path / f"engine_host_{name}")
    subprocess.run(COMMON + SANITIZERS[name] + ["-o", exe, os.path.join(ROOT, "tests", "engine_host_main.cpp")],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stderr == b""
    assert r.stdout.decode().strip() == "engine_host: ok"
