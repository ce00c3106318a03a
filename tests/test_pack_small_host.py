"""CPU: what the one-launch pack takes from pack.h and pack_wide.h, compiled with g++ into the
stand-alone program tests/pack_small_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly: the staging bounds (pack_bits_bound,
wpack_bits_bound, wpack_blocks_bound) are never below what clg_pack_columns_host /
clg_pack_wide_host produce, over random streams, all-equal streams, INT64_MIN beside INT64_MAX,
VAR_OFF = 0, 0xFFFFFFFF, 0, ... (33-bit residuals) and every stream length in {0, 1, 2, 1023, 1024,
1025, 2049}; and the in-header stream layout (wpack_layout_streams) is wpack_layout's."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pack_small_host.cpp")


def test_bounds_and_layout(tmp_path):
    exe = str(tmp_path / "pack_small_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout


def test_bounds_and_layout_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "pack_small_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout
