"""CPU: the log comparison on the host -- the header clonos_amd/csrc/diff.h compiled with g++
into a stand-alone program (tests/diff_host.cpp), and clg_lcp_host of the library.

The reference is a byte loop (os.path.commonprefix).
"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diff_host.cpp")


def build_and_run(tmp_path, extra):
    exe = str(tmp_path / "diff_host")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        return cc, None
    return cc, subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_header_program(tmp_path):
    cc, run = build_and_run(tmp_path, [])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and "diff_host: ok" in run.stdout, run.stderr


def test_header_program_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: its buffers are exactly as long as the
    strings, so a word read past an end would be reported."""
    cc, run = build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and ("asan" in cc.stderr or "ubsan" in cc.stderr):
        pytest.skip("no sanitizer runtime for g++ on this machine")
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and "diff_host: ok" in run.stdout, run.stderr


def lcp(a: bytes, b: bytes) -> int:
    return len(os.path.commonprefix([a, b]))


def test_lcp_host_every_length_and_position():
    from clonos_amd import lcp_host
    rng = random.Random(9)
    for na in range(41):
        a = bytes(rng.getrandbits(8) for _ in range(na))
        for nb in range(41):
            b = (a + bytes(rng.getrandbits(8) for _ in range(40)))[:nb]
            assert lcp_host(a, b) == min(na, nb) == lcp(a, b)
            for d in range(min(na, nb)):
                f = bytearray(b)
                f[d] ^= 0x80 if d % 2 else 0x01
                assert lcp_host(a, bytes(f)) == d == lcp(a, bytes(f)), (na, nb, d)


def test_lcp_host_cases():
    import numpy as np

    from clonos_amd import lcp_host
    assert lcp_host(b"", b"") == 0 and lcp_host(b"", b"x") == 0 and lcp_host(b"x", b"") == 0
    assert lcp_host(b"abc", b"abcd") == 3 and lcp_host(b"abcd", b"abc") == 3  # one a prefix of the other
    assert lcp_host(b"abcd", b"abcd") == 4
    rng = random.Random(10)
    a = bytes(rng.getrandbits(8) for _ in range(100_001))
    assert lcp_host(a, a) == len(a)
    cut = a[:70_000] + b"\0" * 5
    assert lcp_host(np.frombuffer(a, np.uint8), cut) == lcp(a, cut) >= 70_000
    assert lcp_host(a, a[:99_999] + bytes([a[99_999] ^ 0x80]) + a[100_000:]) == 99_999
