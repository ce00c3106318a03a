"""CPU: the log digest on the host -- clg_digest_host of the library, and the header
clonos_amd/csrc/digest.h compiled with g++ (tests/digest_host.cpp).

The reference is the definition restated here with Python integers: p = 2^61 - 1,
R = 2654435761, m = ceil(n / 4) little-endian u32 words zero-padded past the end,
hash = sum w_k R^(m-1-k) mod p, i.e. h = (h * R + w_k) mod p per word.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 61) - 1
R = 2654435761

KNOWN = [
    ("", 0x0),
    ("01", 0x1),
    ("0001020304050607", 0x1dbe37a44e1b604),
    ("000102030405060708", 0xd552ceceb23a8f8),
    ("0003" "010000000123456789" "0200000007", 0x16be1ad9309f8555),  # Order, Timestamp, RNG
    ("ff" * 4096, 0x44074c7fe928a7e),
    ("39efc63396a82399", 0x0),  # words a, b with a * R + b == p exactly
]


def ref_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


def test_reference_restates_the_sum():
    rng = random.Random(3)
    for n in (1, 5, 8, 23):
        b = bytes(rng.getrandbits(8) for _ in range(n))
        m = (n + 3) // 4
        byte_linear = sum(x * (1 << (8 * (i % 4))) * pow(R, m - 1 - i // 4, P) for i, x in enumerate(b)) % P
        assert ref_digest(b)[0] == byte_linear


@pytest.mark.parametrize("hexs,want", KNOWN)
def test_known_answers(hexs, want):
    from clonos_amd import digest_host
    b = bytes.fromhex(hexs)
    assert ref_digest(b) == (want, len(b))
    assert digest_host(b) == (want, len(b))


def test_random_lengths():
    from clonos_amd import digest_host
    rng = random.Random(4)
    for n in list(range(71)) + [4095, 4096, 4097]:
        b = bytes(rng.getrandbits(8) for _ in range(n))
        got = digest_host(b)
        assert got == ref_digest(b) and 0 <= got[0] < P


def test_flipped_byte_and_swapped_records_change_the_hash():
    from clonos_amd import digest_host
    rng = random.Random(5)
    recs = [bytes([1]) + rng.getrandbits(64).to_bytes(8, "big") for _ in range(12)]  # 9-byte Timestamp records
    b = b"".join(recs)
    base = digest_host(b)
    for i in (0, 1, 50, len(b) - 1):
        f = bytearray(b)
        f[i] ^= 0x01
        got = digest_host(bytes(f))
        assert got[1] == base[1] and got[0] != base[0] and got == ref_digest(bytes(f))
    sw = list(recs)
    sw[3], sw[4] = sw[4], sw[3]
    got = digest_host(b"".join(sw))
    assert got[1] == base[1] and got[0] != base[0] and got == ref_digest(b"".join(sw))


@pytest.fixture(scope="module")
def dgh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("digest") / "libdigest_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "digest_host.cpp")], check=True)
    lib = C.CDLL(so)
    for f, args in (("dgh_pow", [C.c_uint32]), ("dgh_pow_ladder", [C.c_uint32]), ("dgh_mul", [C.c_uint64, C.c_uint64]),
                    ("dgh_step", [C.c_uint64, C.c_uint32]), ("dgh_step_lazy", [C.c_uint64, C.c_uint32]),
                    ("dgh_reduce", [C.c_uint64]), ("dgh_bytes", [C.c_char_p, C.c_uint64])):
        getattr(lib, f).restype = C.c_uint64
        getattr(lib, f).argtypes = args
    return lib


def test_header_power_function(dgh):
    """Exponents 0, 1 and 2^k +- 1 up to 2^30: the ladder's high bits, which no GPU test of a
    few seconds reaches."""
    exps = {0, 1}
    for k in range(1, 31):
        exps |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    exps.add((1 << 32) - 1)
    for e in sorted(exps):
        want = pow(R, e, P)
        assert dgh.dgh_pow(e) == want, e
        assert dgh.dgh_pow_ladder(e) == want, e


def test_header_mul_and_step_edges(dgh):
    rng = random.Random(6)
    edge = [0, 1, 2, (1 << 29) - 1, 1 << 29, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 2, P - 1, R]
    vals = edge + [rng.randrange(P) for _ in range(300)]
    for a in vals:
        for b in edge + [rng.randrange(P) for _ in range(4)]:
            assert dgh.dgh_mul(a, b) == a * b % P, (a, b)
        for w in (0, 1, 0x9923a896, 0xFFFFFFFF, rng.getrandbits(32)):
            assert dgh.dgh_step(a, w) == (a * R + w) % P, (a, w)
    assert dgh.dgh_step(0x33c6ef39, 0x9923a896) == 0  # a * R + b == p: the last reduction


def test_header_lazy_step_chain(dgh):
    """The kernels' unreduced step: from any h below 2^63 it stays below 2^63 and congruent,
    and dg_reduce of it is the canonical value."""
    rng = random.Random(8)
    top = (1 << 63) - 1
    for h0 in [0, 1, P - 1, P, P + 1, (1 << 62) - 1, 1 << 62, top] + [rng.getrandbits(63) for _ in range(200)]:
        h, want = h0, h0 % P
        for w in [0xFFFFFFFF, 0, 0x9923a896] + [rng.getrandbits(32) for _ in range(13)]:
            h = dgh.dgh_step_lazy(h, w)
            want = (want * R + w) % P
            assert h <= top and h % P == want
        assert dgh.dgh_reduce(h) == want
    assert dgh.dgh_reduce(dgh.dgh_step_lazy(0x33c6ef39, 0x9923a896)) == 0
    assert dgh.dgh_reduce(top + (1 << 61)) == (top + (1 << 61)) % P


def test_header_bytes_matches_library(dgh):
    from clonos_amd import digest_host
    rng = random.Random(7)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 1000):
        b = bytes(rng.getrandbits(8) for _ in range(n))
        assert dgh.dgh_bytes(b, n) == digest_host(b)[0] == ref_digest(b)[0]
