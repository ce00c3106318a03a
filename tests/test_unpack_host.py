"""CPU: the whole-call unpack of packed typed columns on the host.  The header's functions
(clonos_amd/csrc/pack.h, compiled with g++ into the stand-alone program tests/unpack_host.cpp, once
plainly and once with -fsanitize=address,undefined, and run directly), and
clg_unpack_columns_all_host of the library through unpack_packed_host over the oracle's columns:
the round trip gives the columns back, array for array what PackedColumns.unpack() gives."""
import os
import re
import subprocess

import numpy as np
import pytest

from _columns_util import assert_columns_equal
from _pack_util import STREAMS, Narrow, values_of_width
from test_pack_host import SPANS, columns_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "unpack_host.cpp")


def test_header_functions(tmp_path):
    exe = str(tmp_path / "unpack_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 3000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "unpack_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


@pytest.mark.parametrize("name", sorted(SPANS))
def test_round_trip_is_the_input_and_equals_the_stream_unpack(name):
    from clonos_amd import pack_columns_host, unpack_packed_host
    cols, _ = columns_of(name)
    packed = pack_columns_host(cols)
    got = unpack_packed_host(packed)
    assert_columns_equal(got, cols)
    want = packed.unpack()
    for f, dt, _ in STREAMS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype == dt and a.shape == b.shape and (a == b).all(), f
    for f in ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0", "var", "var_pos", "error"):
        assert getattr(got, f) is getattr(want, f), f  # passed through
    assert (got.span_base == want.span_base).all()


def test_every_width_round_trips():
    from clonos_amd import pack_columns_host, unpack_packed_host
    rng = np.random.default_rng(0x51DF)
    for w in range(65):
        cols = Narrow(tag=values_of_width(rng, np.uint8, min(w, 3), 1025, vmin=0, vmax=7),
                      order=values_of_width(rng, np.int8, min(w, 8), 1023),
                      timestamp=values_of_width(rng, np.int64, w, 1024, delta=True),
                      rng=values_of_width(rng, np.int32, min(w, 32), 2049),
                      buffer_built=values_of_width(rng, np.int32, min(w, 32), 3))
        back = unpack_packed_host(pack_columns_host(cols))
        for name, _, _ in STREAMS:
            assert (getattr(back, name) == getattr(cols, name)).all(), (w, name)


def test_errors_carry_what_stream_and_block():
    from clonos_amd import ClonosError, _lib, pack_columns_host, unpack_packed_host
    cols, _ = columns_of("config3")
    packed = pack_columns_host(cols)
    good = packed.desc
    b3 = packed.blk_base[3]

    def raises(desc, what, stream, block):
        packed.desc = desc
        with pytest.raises(ClonosError) as ei:
            unpack_packed_host(packed)
        e = ei.value
        assert (e.status, e.bad_what, e.bad_stream, e.bad_block) == (_lib.CLG_E_INVALID_ARG, what, stream, block)
        packed.desc = good

    d = good.copy()
    d["pos"][b3] += 8  # the format's own rule, which clg_unpack_columns_host does not test
    raises(d, _lib.UNPACK_BAD_BLOCK, 3, 0)
    packed.desc = d
    if d["width"][b3] and d["pos"][b3] + 8 + (int(d["count"][b3]) * int(d["width"][b3]) + 7) // 8 <= packed.bits.size:
        packed.unpack_stream(3, 0, 1)  # the per-stream unpack keeps accepting it
    packed.desc = good
    d = good.copy()
    d["ref"][b3] = (1 << 31) - 1
    d["width"][1] = 65
    raises(d, _lib.UNPACK_BAD_BLOCK, 0, 1)  # a block and a value: the block
    d["width"][1] = good["width"][1]
    raises(d, _lib.UNPACK_BAD_VALUE, 3, 0)
    packed.blk_base[1] += 1
    raises(good, _lib.UNPACK_BAD_LAYOUT, 0, 0)
    packed.blk_base[1] -= 1
    assert_columns_equal(unpack_packed_host(packed), cols)
