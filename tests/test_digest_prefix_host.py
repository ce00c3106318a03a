"""CPU: prefix digests on the host -- the header's one-pass function (clonos_amd/csrc/digest.h,
compiled with g++ into the stand-alone program tests/digest_prefix_host.cpp) against dg_bytes of
each prefix, and clg_digest_prefixes_host of the library against the definition restated here
with Python integers: p = 2^61 - 1, R = 2654435761, little-endian u32 words zero-padded past the
end, h = (h * R + w) mod p per word; the row of a cut c is {hash(b[:min(c, n)]), min(c, n)}.
"""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 61) - 1
R = 2654435761


def ref_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


def rows(d):
    return [(int(x["hash"]), int(x["len"])) for x in d]


def test_recurrence_restates_the_definition():
    """D_j = D_{j-1} R^(m(c_j) - m(c_{j-1})) + S_j with S_j the byte-linear sum over the stretch."""
    rng = random.Random(11)
    for _ in range(60):
        n = rng.randrange(0, 90)
        b = bytes(rng.getrandbits(8) for _ in range(n))
        cuts = sorted(rng.randrange(0, n + 1) for _ in range(rng.randrange(1, 9)))
        d, prev = 0, 0
        for c in cuts:
            m, m0 = (c + 3) // 4, (prev + 3) // 4
            s = sum(b[i] * (1 << (8 * (i % 4))) * pow(R, m - 1 - i // 4, P) for i in range(prev, c)) % P
            d = (d * pow(R, m - m0, P) + s) % P
            assert (d, c) == ref_digest(b[:c])
            prev = c


def test_header_one_pass_function(tmp_path):
    """(The program has its own main, so it also builds with -fsanitize=address,undefined.)"""
    exe = str(tmp_path / "digest_prefix_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "digest_prefix_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 3000, r.stdout


def test_library_prefixes_host():
    from clonos_amd import DIGEST, ClonosError, _lib, digest_host, digest_prefixes_host
    rng = random.Random(12)
    for t in range(120):
        n = rng.randrange(0, 400)
        b = bytes(rng.getrandbits(8) for _ in range(n))
        cuts = sorted(rng.randrange(0, n + 12) for _ in range(rng.randrange(0, 14)))
        if t % 9 == 0:
            cuts.append((1 << 32) - 1)
        got = digest_prefixes_host(b, cuts)
        assert got.dtype == DIGEST
        assert rows(got) == [ref_digest(b[:min(c, n)]) for c in cuts], (n, cuts)
    b = bytes(rng.getrandbits(8) for _ in range(300))
    got = rows(digest_prefixes_host(b, list(range(301))))
    assert got == [ref_digest(b[:c]) for c in range(301)]
    assert got[-1] == digest_host(b) and got[0] == (0, 0)
    assert rows(digest_prefixes_host(b"", [0, 0, 7])) == [(0, 0)] * 3
    assert len(digest_prefixes_host(b, [])) == 0
    with pytest.raises(ClonosError) as ei:
        digest_prefixes_host(b, [4, 3])
    assert ei.value.status == _lib.CLG_E_INVALID_ARG
