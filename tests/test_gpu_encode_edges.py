"""GPU: the batched encode (clg_encode_batch, encode.hip) at its edges, bit-exact against the CPU
oracle (_oracle.encode_soa: orc_encode record by record).  The records are built by hand in the
SoA layout (_encode_scenes.py; test_encode_edges_scene.py checks what the scenes hit without a
GPU), never through a decoder.

What is swept:
  1. lengths: n around the 4 records of a thread, the 256 of a wavefront and the 1024 of a block,
     as narrow records, as one wide kind, and with every kind in turn (period 13).
  2. every kind (the ten determinants, with and without payload bytes) at each of a thread's four
     slots and on both sides of the wave seam (255 | 256) and of two block seams (1023 | 1024,
     2047 | 2048), between records of another kind.
  3. the wide-row prefix: a block of 1024 wide records; wide records at the last record of a
     block and the first of a later one with blocks that hold none between; one as the very last.
  4. field extremes: min, max, -1 and 0 of every field, v0 with bits above the field's width,
     both flag states, every checkpoint type and callback ordinal.
  5. the LDS stage limit: blocks of 28 671, 28 672 (staged) and 28 673 bytes (direct stores),
     through one long record (first, in the middle, last) and through 1024 medium ones; a staged
     block at the limit, a direct block and a block of one record in a row.
  6. the second round of both scans: 1027 blocks, wide rows either side of block 1024.
  7. memory kinds and bounds: device input and output against host input and output; the output
     at byte offsets 0, 1, 3 and 15 of a buffer that held 0xFF, with cap == n_out: nothing before
     out and nothing at or after out + n_out is written; cap == n_out - 1: CLG_E_CAPACITY, the
     size, nothing written; out == NULL: the size.
  8. validation: the lowest bad record (a plain loop in the scene module) for bad tags, side rows
     that name another record, one row too few and one too many (bad_index == n), and payload
     ranges that pass var by 1 and by 8 bytes; after each error a valid batch encodes exactly.

Payload bytes are 1..254 and output buffers hold 0xFF, so a misplaced byte cannot pass for fill.
"""
import ctypes as C

import numpy as np
import pytest

import _encode_scenes as S
import _oracle as O
from _devbuf import DeviceBuf
from clonos_amd import Engine, _lib
from clonos_amd._lib import lib

pytestmark = pytest.mark.gpu

GUARD = 64  # fill bytes kept and compared before and after every output


@pytest.fixture(scope="module")
def eng():
    e = Engine(segment_bytes=16384, pool_segments=64)
    yield e
    e.close()


_want = {}


def want_of(name, soa):
    """The oracle's bytes of a scene, computed once."""
    if name not in _want:
        _want[name] = O.encode_soa(*soa)
    return _want[name]


def assert_same(got, want, what):
    """got == want; on a difference the first differing place, not two buffers."""
    got, want = bytes(got), bytes(want)
    if got == want:
        return
    assert len(got) == len(want), f"{what}: {len(got)} bytes, want {len(want)}"
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.flatnonzero(g != w)
    i = int(bad[0])
    lo = max(i - 4, 0)
    raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {i} (..{int(bad[-1])}): got "
                         f"{got[lo:i + 24].hex()} want {want[lo:i + 24].hex()} (from {lo})")


TYPES = (np.uint8, np.int64, np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8)


def host_input(soa):
    """clg_encode_in over host arrays; (struct, what it points into)."""
    arrs = [np.ascontiguousarray(a, t) for a, t in zip(soa[:8], TYPES)]
    var = np.frombuffer(soa[8], np.uint8) if len(soa[8]) else np.zeros(1, np.uint8)
    p = [a.ctypes.data if a.size else None for a in arrs]
    ein = _lib.EncodeIn(p[0], p[1], len(arrs[0]), *p[2:8], len(arrs[2]), var.ctypes.data, len(soa[8]),
                        _lib.CLG_MEM_HOST, 0)
    return ein, (arrs, var)


def device_input(soa):
    """The same arrays in one device buffer, each at a 256-byte aligned place; var's last byte is
    the buffer's last."""
    arrs = [np.ascontiguousarray(a, t) for a, t in zip(soa[:8], TYPES)] + [np.frombuffer(soa[8], np.uint8)]
    at, size = [], 0
    for a in arrs:
        at.append(size)
        size += (a.nbytes + 255) // 256 * 256 if a is not arrs[-1] else a.nbytes
    buf = DeviceBuf(max(size, 1))
    for a, o in zip(arrs, at):
        if a.nbytes:
            assert buf.hip.hipMemcpy(C.c_void_p(buf.at(o)), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    assert buf.hip.hipDeviceSynchronize() == 0
    p = [buf.at(o) if a.nbytes else None for a, o in zip(arrs, at)]
    ein = _lib.EncodeIn(p[0], p[1], len(arrs[0]), *p[2:8], len(arrs[2]), p[8], len(soa[8]), _lib.CLG_MEM_DEVICE, 0)
    return ein, buf


def call(eng, ein, out, cap, kind):
    """(status, *n_out, *bad_index)."""
    n_out, bad = C.c_uint64(12345), C.c_uint64(12345)
    st = lib.clg_encode_batch(eng.handle, C.byref(ein), out, cap, kind, C.byref(n_out), C.byref(bad))
    return st, n_out.value, bad.value


def encode_host(eng, soa, n_out):
    """Host rows to host bytes with cap == n_out, in a buffer that held FILL: the whole buffer."""
    ein, keep = host_input(soa)
    out = np.full(n_out + 2 * GUARD, S.FILL, np.uint8)
    st, n, _ = call(eng, ein, out.ctypes.data + GUARD, n_out, _lib.CLG_MEM_HOST)
    assert (st, n) == (_lib.CLG_OK, n_out), lib.clg_last_error()
    return out.tobytes()


def framed(want, lead=GUARD, size=None):
    """want behind `lead` fill bytes in a buffer of fill."""
    size = lead + len(want) + GUARD if size is None else size
    return bytes([S.FILL]) * lead + want + bytes([S.FILL]) * (size - lead - len(want))


def check_scene(eng, name, soa):
    want = want_of(name, soa)
    assert_same(encode_host(eng, soa, len(want)), framed(want), name)


# ---- 1. lengths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", S.MIXES)
def test_lengths(eng, mix):
    for m, n, soa in S.length_scenes():
        if m == mix:
            check_scene(eng, f"len_{mix}_{n}", soa)


# ---- 2. kinds at slots and seams ----------------------------------------------------------------------
def test_every_kind_at_every_slot_and_seam(eng):
    for kind, side, soa in S.place_scenes():
        check_scene(eng, f"place_{kind}_{side}", soa)


# ---- 3. the wide-row prefix ---------------------------------------------------------------------------
def test_wide_prefix(eng):
    for name, soa in S.prefix_scenes():
        check_scene(eng, f"prefix_{name}", soa)


# ---- 4. field extremes ----------------------------------------------------------------------------------
def test_field_extremes(eng):
    check_scene(eng, "extremes", S.extremes())


# ---- 5. the stage limit ---------------------------------------------------------------------------------
def test_stage_limit(eng):
    for name, soa, totals in S.stage_scenes():
        assert len(want_of(f"stage_{name}", soa)) == sum(totals)
        check_scene(eng, f"stage_{name}", soa)


# ---- 6. the second scan round ---------------------------------------------------------------------------
def test_second_scan_round(eng):
    check_scene(eng, "scan_round", S.scan_round())


# ---- 7. memory kinds and bounds -------------------------------------------------------------------------
def memory_scenes():
    stage = {name: soa for name, soa, _ in S.stage_scenes()}
    return [("extremes", S.extremes()), ("stage_staged_direct_one", stage["staged_direct_one"]),
            ("prefix_empty_blocks", dict(S.prefix_scenes())["empty_blocks"])]


@pytest.mark.parametrize("scene", range(3))
def test_memory_kinds_and_bounds(eng, scene):
    name, soa = memory_scenes()[scene]
    want = want_of(name, soa)
    n_out = len(want)
    hin, keep = host_input(soa)
    din, dbuf = device_input(soa)
    obuf = DeviceBuf(GUARD + 16 + n_out + GUARD)
    try:
        assert_same(encode_host(eng, soa, n_out), framed(want), f"{name}: host to host")
        # sizes only
        for ein in (hin, din):
            assert call(eng, ein, None, 0, _lib.CLG_MEM_HOST) == (_lib.CLG_E_CAPACITY, n_out, 2**64 - 1)
        # device input to host output
        out = np.full(n_out + 2 * GUARD, S.FILL, np.uint8)
        assert call(eng, din, out.ctypes.data + GUARD, n_out, _lib.CLG_MEM_HOST)[:2] == (_lib.CLG_OK, n_out)
        assert_same(out, framed(want), f"{name}: device to host")
        # device output at every residue, from device and from host input: cap == n_out exactly
        for d in (0, 1, 3, 15):
            for kind, ein in (("device", din), ("host", hin)):
                obuf.fill(S.FILL)
                assert call(eng, ein, obuf.at(GUARD + d), n_out, _lib.CLG_MEM_DEVICE)[:2] == (_lib.CLG_OK, n_out)
                assert_same(obuf.host(), framed(want, GUARD + d, obuf.n), f"{name}: {kind} to device at +{d}")
        # one byte short: the size, nothing written
        obuf.fill(S.FILL)
        assert call(eng, din, obuf.at(GUARD), n_out - 1, _lib.CLG_MEM_DEVICE)[:2] == (_lib.CLG_E_CAPACITY, n_out)
        assert_same(obuf.host(), framed(b"", GUARD, obuf.n), f"{name}: short device output")
        out[:] = S.FILL
        assert call(eng, hin, out.ctypes.data + GUARD, n_out - 1, _lib.CLG_MEM_HOST)[:2] == (_lib.CLG_E_CAPACITY, n_out)
        assert_same(out, framed(b"", GUARD, out.size), f"{name}: short host output")
    finally:
        dbuf.free()
        obuf.free()
    del keep


# ---- 8. validation ----------------------------------------------------------------------------------------
def expect_error(eng, name, soa, bad):
    """CLG_E_INVALID_ARG with the lowest bad record, no size, nothing written."""
    ein, keep = host_input(soa)
    out = np.full(1 << 16, S.FILL, np.uint8)
    st, n_out, got = call(eng, ein, out.ctypes.data, out.size, _lib.CLG_MEM_HOST)
    assert (st, got, n_out) == (_lib.CLG_E_INVALID_ARG, bad, 0), f"{name}: {lib.clg_last_error()}"
    assert (out == S.FILL).all(), name
    del keep


def test_validation_reports_the_lowest_bad_record(eng):
    ok = S.range_batch()
    for name, soa, bad in S.validation_scenes():
        expect_error(eng, name, soa, bad)
        check_scene(eng, "range_exact", ok)  # a valid batch on the same engine still encodes exactly
    # into device memory as well: nothing written
    name, soa, bad = S.validation_scenes()[0]
    din, dbuf = device_input(soa)
    obuf = DeviceBuf(4096, S.FILL)
    try:
        assert call(eng, din, obuf.at(0), obuf.n, _lib.CLG_MEM_DEVICE) == (_lib.CLG_E_INVALID_ARG, 0, bad)
        assert (obuf.host() == S.FILL).all()
    finally:
        dbuf.free()
        obuf.free()


def test_payload_ranges(eng):
    """A payload row whose range passes var is rejected (host input only, by 1 and by 8 bytes: the
    staged var is followed by 16 spare bytes); a range that ends on var's last byte, an empty one
    at var_len and a wild range on a row without a payload are accepted."""
    for name, soa, bad, same_as in S.range_scenes():
        if bad is None:
            want = want_of("range_exact", same_as)
            assert_same(encode_host(eng, soa, len(want)), framed(want), name)
        else:
            expect_error(eng, name, soa, bad)
            check_scene(eng, "range_exact", S.range_batch())
