"""CPU: the packed payload column on the host.  The header's functions (clonos_amd/csrc/ppay.h,
compiled with g++ into the stand-alone program tests/ppay_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_pack_payloads_host /
clg_unpack_payloads_host of the library through ctypes: the bytes are an independent numpy packer's
(tests/_ppay_util.py) and the round trip gives the column back, over the payload columns of
test_pack_host.py's span sets.  Two size conditions hold for the numpy packer alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _ppay_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ppay_host.cpp")


def test_header_functions(tmp_path):
    exe = str(tmp_path / "ppay_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "ppay_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


_COLUMNS = {}


def column_of(name):
    """The payload column of one of test_pack_host.py's span sets, computed once."""
    from test_pack_host import SPANS
    if name not in _COLUMNS:
        _COLUMNS[name] = U.payload_column_of(SPANS[name])
    return _COLUMNS[name]


@pytest.mark.parametrize("name", ["all_empty", "config2", "config3", "empty_first_middle_last", "random_log"])
def test_bytes_are_the_numpy_packers_and_the_round_trip_is_the_column(name):
    from clonos_amd import pack_payloads_host, unpack_payloads_host
    var, pos = column_of(name)
    packed = pack_payloads_host(var, pos)
    U.assert_packed_equals_numpy(packed, var, pos)
    assert packed.tail.size <= var.size
    back = unpack_payloads_host(packed, pos)
    assert back.dtype == np.uint8 and back.tobytes() == var.tobytes()
    assert packed.unpack(pos).tobytes() == var.tobytes()
    assert U.unpack_numpy(packed.desc, packed.bits, packed.tail, pos).tobytes() == var.tobytes()


def test_seeded_rows_across_the_tile_seams():
    from clonos_amd import pack_payloads_host, unpack_payloads_host
    rng = np.random.default_rng(0x77)
    for n in (1, 1023, 1024, 1025, 2049):
        var, pos = U.column(U.seeded_rows(rng, n, [0, 1, 2, 15, 16, 17, 63, 64, 65, 300]))
        packed = pack_payloads_host(var, pos)
        U.assert_packed_equals_numpy(packed, var, pos)
        assert unpack_payloads_host(packed, pos).tobytes() == var.tobytes()


@pytest.mark.parametrize("m,L", [(1, 47), (2, 1), (700, 47), (1024, 47), (1024, 200)])
def test_identical_rows_leave_one_row_of_tail(m, L):
    """The reference packer alone: a column of m <= 1024 identical rows of L bytes has n_tail == L."""
    var, pos = U.column([bytes((7 * i + 3) % 251 for i in range(L))] * m)
    desc, bits, tail = U.pack_numpy(var, pos)
    assert tail.size == L
    from clonos_amd import pack_payloads_host
    assert pack_payloads_host(var, pos).tail.size == L


def test_config3_packs_to_at_most_half():
    """The reference packer alone: the payload column of synth.config3_epoch(3000,
    default_rng(0x9AC)) packs to at most half its n_var, desc, bits and tail counted together."""
    var, pos = U.config3_column()
    desc, bits, tail = U.pack_numpy(var, pos)
    total = desc.nbytes + bits.size + tail.size
    print(f"config 3, 3000 records: {len(pos) - 1} rows, n_var {var.size} B, packed {total} B "
          f"(desc {desc.nbytes}, bits {bits.size}, tail {tail.size}), ratio {total / var.size:.4f}")
    assert var.size > 0 and 2 * total <= var.size
    from clonos_amd import pack_payloads_host
    assert pack_payloads_host(var, pos).n_bytes == total


def test_sizes_only_capacity_and_rejections_through_ctypes():
    from clonos_amd import ClonosError, _lib, pack_payloads_host, unpack_payloads_host
    from clonos_amd.engine import PACK_BLOCK, _packed_payloads_struct, _payloads_struct
    var, pos = column_of("random_log")
    n = pos.size - 1
    want = pack_payloads_host(var, pos)
    p = _lib.PackedPayloadsC()
    assert _lib.lib.clg_pack_payloads_host(var.ctypes.data, pos.ctypes.data, n, C.byref(p)) == _lib.CLG_OK
    assert (p.n_rows, p.n_var, p.n_bits, p.n_tail, p.bad_row) == (n, var.size, want.bits.size, want.tail.size, U.NO_ROW)
    for short in ("desc", "bits", "tail"):
        desc = np.full((want.desc.size - (short == "desc")) * 32, 0xA5, np.uint8)
        bits = np.full(want.bits.size - (short == "bits"), 0xA5, np.uint8)
        tail = np.full(want.tail.size - (short == "tail"), 0xA5, np.uint8)
        p = _packed_payloads_struct(desc.view(PACK_BLOCK), bits, tail)
        assert _lib.lib.clg_pack_payloads_host(var.ctypes.data, pos.ctypes.data, n, C.byref(p)) == _lib.CLG_E_CAPACITY
        assert (p.n_rows, p.n_var, p.n_bits, p.n_tail) == (n, var.size, want.bits.size, want.tail.size)
        assert (desc == 0xA5).all() and (bits == 0xA5).all() and (tail == 0xA5).all()
    # bad rows, the lowest
    for where, row in ((0, 0), (n // 2, None), (n, None)):
        q = pos.copy()
        q[where] = 1 if where == 0 else q[where - 1] - 1 if where < n else q[where - 1] + (1 << 32)
        with pytest.raises(ClonosError) as ei:
            pack_payloads_host(var, q)
        lens = np.diff(q.astype(np.int64).astype(object))
        first = 0 if where == 0 else int(next(k for k in range(n) if lens[k] < 0 or lens[k] >= 1 << 32))
        assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_row == first
    # the unpack: sizes only, capacity, a finding of each kind
    good = want._struct()
    out = _lib.Payloads()
    bad = _lib.UnpackBad()
    assert _lib.lib.clg_unpack_payloads_host(C.byref(good), pos.ctypes.data, C.byref(out), C.byref(bad)) == _lib.CLG_OK
    assert (out.n_rows, out.n_var, bad.what, bad.block) == (n, var.size, _lib.UNPACK_BAD_NONE, U.NO_ROW)
    buf = np.full(var.size - 1, 0xA5, np.uint8)
    out = _payloads_struct(buf, None)
    assert _lib.lib.clg_unpack_payloads_host(C.byref(good), pos.ctypes.data, C.byref(out), C.byref(bad)) == _lib.CLG_E_CAPACITY
    assert (buf == 0xA5).all()

    def finding(packed, q=pos):
        with pytest.raises(ClonosError) as ei:
            unpack_payloads_host(packed, q)
        assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_stream == _lib.PPAY_STREAM
        return ei.value.bad_what, ei.value.bad_block

    d = want.desc.copy()
    d["width"][0] = 65
    assert finding(type(want)(d, want.bits, want.tail, n, var.size)) == (_lib.UNPACK_BAD_BLOCK, 0)
    d = want.desc.copy()
    d["ref"][0] = 1  # row 0 is its own anchor
    assert finding(type(want)(d, want.bits, want.tail, n, var.size)) == (_lib.UNPACK_BAD_VALUE, 0)
    assert finding(type(want)(want.desc, want.bits, want.tail[:-1], n, var.size)) == (_lib.UNPACK_BAD_TOTAL, 0)
    assert finding(type(want)(want.desc, want.bits, want.tail, n, var.size + 1)) == (_lib.UNPACK_BAD_TOTAL, 0)
    assert finding(type(want)(want.desc[:0], want.bits, want.tail, n, var.size)) == (_lib.UNPACK_BAD_LAYOUT, 0)
