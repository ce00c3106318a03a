"""CPU: the placement helper (clonos_amd/csrc/placement.h), which decides for every entry point of
the columns family whether a caller's arrays are used in place, through their registered device
address, or through engine staging.  The header is host-only; tests/placement_host.cpp drives it
with a fake registry of two adjacent ranges.  Compiled with g++ once plainly and once with
-fsanitize=address,undefined, and run directly."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "placement_host.cpp")


def test_header_functions(tmp_path):
    exe = str(tmp_path / "placement_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "placement_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


def test_the_header_is_host_only():
    """placement.h includes nothing but <cstddef> and <cstdint>."""
    text = open(os.path.join(ROOT, "clonos_amd", "csrc", "placement.h")).read()
    assert sorted(re.findall(r"^#include (.*)$", text, re.M)) == ["<cstddef>", "<cstdint>"]
