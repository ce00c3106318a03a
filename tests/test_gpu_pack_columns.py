"""GPU: clg_pack_columns.  Every comparison is byte for byte against pack_columns_host (which
tests/test_pack_host.py holds against an independent numpy packer): the packed bytes are a pure
function of the columns, so there is no tolerance."""
import ctypes as C
import mmap

import numpy as np
import pytest

from _pack_util import STREAMS, Narrow, assert_packed_equals_numpy, assert_same_packed, values_of_width

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as e:
        yield e


def blocks_of_widths(rng, dtype, widths, delta=False, **kw):
    """One full block of 1024 values per width, in order (a DELTA block restarts at its own first value)."""
    return np.concatenate([values_of_width(rng, dtype, w, 1024, delta, **kw) for w in widths])


def every_width_columns():
    rng = np.random.default_rng(0x9AC4)
    return Narrow(tag=blocks_of_widths(rng, np.uint8, range(4), vmin=0, vmax=7),
                  order=blocks_of_widths(rng, np.int8, range(9)),
                  timestamp=blocks_of_widths(rng, np.int64, range(65), delta=True),
                  rng=blocks_of_widths(rng, np.int32, range(33)),
                  buffer_built=blocks_of_widths(rng, np.int32, reversed(range(33))))


def mixed_columns(n, seed, lens=None):
    """Five streams of n values (lens: per stream) with widths off the word seams."""
    rng = np.random.default_rng(seed)
    lens = lens or [n] * 5
    mk = lambda dt, w, k, **kw: values_of_width(rng, dt, w if k >= 3 else 0, k, **kw) if k else np.zeros(0, dt)
    return Narrow(tag=mk(np.uint8, 3, lens[0], vmin=0, vmax=7), order=mk(np.int8, 2, lens[1]),
                  timestamp=mk(np.int64, 3, lens[2], delta=True),
                  rng=mk(np.int32, 31, lens[3]), buffer_built=mk(np.int32, 13, lens[4]))


def test_every_width_matches_the_host_packer(eng):
    from clonos_amd import pack_columns_host
    cols = every_width_columns()
    want = pack_columns_host(cols)
    got = eng.pack_columns(cols)
    assert_same_packed(got, want)
    d = np.asarray(got.desc)
    for c, widths in enumerate((range(4), range(9), range(65), range(33), reversed(range(33)))):
        assert list(d["width"][got.blk_base[c]:got.blk_base[c + 1]]) == list(widths)
    back = got.unpack()
    for name, _, _ in STREAMS:
        assert (getattr(back, name) == getattr(cols, name)).all(), name


@pytest.mark.parametrize("width", [31, 32, 33, 63, 64])
@pytest.mark.parametrize("n", [1023, 1025])
def test_word_seams_with_a_short_last_block(eng, width, n):
    """Widths either side of the 32- and 64-bit seams, in a block that is not full and in one
    that is followed by a block of a single value."""
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(width * 4096 + n)
    cols = Narrow(timestamp=values_of_width(rng, np.int64, width, n, delta=True),
                  rng=values_of_width(rng, np.int32, min(width, 32), n))
    assert_same_packed(eng.pack_columns(cols), pack_columns_host(cols))


def test_int64_extremes_side_by_side(eng):
    from clonos_amd import pack_columns_host
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    cols = Narrow(timestamp=np.array([lo, hi, lo, 0, hi, hi, lo, -1, 1] * 150, np.int64))
    got = eng.pack_columns(cols)
    assert_same_packed(got, pack_columns_host(cols))
    assert (got.unpack().timestamp == cols.timestamp).all()


def test_order_extremes_across_a_block_seam(eng):
    """ORDER is the signed 8-bit element: 1025 values with -128 and 127 in the full block and the
    block of one value at either extreme, against the host packer and the numpy packer, and back
    through the device unpack."""
    from clonos_amd import pack_columns_host
    for last in (-128, 127):
        order = np.random.default_rng(0x0DE8).integers(-128, 127, 1025, endpoint=True).astype(np.int8)
        order[[3, 700, 1024]] = -128, 127, last
        cols = Narrow(order=order)
        got = eng.pack_columns(cols)
        assert_same_packed(got, pack_columns_host(cols))
        assert_packed_equals_numpy(got, cols)
        d = np.asarray(got.desc)[got.blk_base[1]:got.blk_base[2]]
        assert list(d["ref"]) == [-128, last] and list(d["width"]) == [8, 0] and list(d["count"]) == [1024, 1]
        back = eng.unpack_columns(got).order
        assert back.dtype == np.int8 and (back == order).all()


@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 1])
def test_stream_lengths(eng, n):
    from clonos_amd import pack_columns_host
    cols = mixed_columns(n, 100 + n)
    got = eng.pack_columns(cols)
    assert_same_packed(got, pack_columns_host(cols))
    assert got.n_val == [n] * 5 and got.blk_base[-1] == 5 * ((n + 1023) // 1024)


@pytest.mark.parametrize("lens", [[2049, 0, 0, 0, 0], [0, 0, 1500, 0, 0], [0, 700, 0, 0, 1], [5, 0, 1025, 0, 3000],
                                  [0, 0, 0, 0, 0]])
def test_some_and_all_streams_empty(eng, lens):
    from clonos_amd import pack_columns_host
    cols = mixed_columns(0, 7, lens)
    got = eng.pack_columns(cols)
    assert_same_packed(got, pack_columns_host(cols))
    assert got.n_val == lens


def test_one_block_more_than_a_scan_group(eng):
    """257 blocks of tags and a block of each other stream: the second group's offsets carry the
    first group's sum, and the last streams' blocks those of both."""
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(0x5CA9)
    cols = mixed_columns(0, 11, [0, 600, 900, 1024, 77])
    cols.tag = rng.integers(0, 8, 256 * 1024 + 1).astype(np.uint8)
    got = eng.pack_columns(cols)
    assert got.blk_base == [0, 257, 258, 259, 260, 261]
    assert_same_packed(got, pack_columns_host(cols))


# ---- where the arrays live ------------------------------------------------------------------
class Region:
    """Bytes in host, device or registered host memory, FILL everywhere to begin with."""

    def __init__(self, kind, n):
        from clonos_amd import _lib
        self.kind, self.n = kind, n
        if kind == "device":
            from _devbuf import DeviceBuf
            self.dev = DeviceBuf(n, fill=FILL)
            self.ptr = self.dev.p.value
        elif kind == "mapped":
            self.mem = np.frombuffer(mmap.mmap(-1, (n + 4095) & ~4095), np.uint8)
            self.mem[:] = FILL
            _lib.check(_lib.lib.clg_host_register(self.mem.ctypes.data, self.mem.size))
            self.ptr = self.mem.ctypes.data
        else:
            self.mem = np.full(n, FILL, np.uint8)
            self.ptr = self.mem.ctypes.data

    def put(self, off, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if not data.size:
            return
        if self.kind == "device":
            assert self.dev.hip.hipMemcpy(C.c_void_p(self.ptr + off), C.c_void_p(data.ctypes.data), C.c_size_t(data.size), 1) == 0
        else:
            self.mem[off:off + data.size] = data

    def get(self):
        return self.dev.host() if self.kind == "device" else np.array(self.mem[:self.n])

    def free(self):
        from clonos_amd import _lib
        if self.kind == "device":
            self.dev.free()
        elif self.kind == "mapped":
            _lib.check(_lib.lib.clg_host_unregister(self.mem.ctypes.data))


KIND = {"host": 0, "device": 1, "mapped": 2}


def columns_in(cols, kind):
    """clg_columns over the five arrays of `cols` placed in one region of `kind`, 64 bytes apart."""
    from clonos_amd import _lib
    arrs = [np.ascontiguousarray(getattr(cols, name), dt) for name, dt, _ in STREAMS]
    at, total = [], 0
    for a in arrs:
        at.append(total)
        total += (a.nbytes + 63 & ~63) + 64
    reg = Region(kind, max(total, 64))
    c = _lib.Columns()
    for (name, _, _), a, o in zip(STREAMS, arrs, at):
        reg.put(o, a)
        setattr(c, name, reg.ptr + o)
    c.n_rec = arrs[0].size
    for k in range(4):
        c.n_class[k] = arrs[k + 1].size
    c.out_kind = KIND[kind]
    return c, reg


def packed_out(kind, cap_desc, cap_bits):
    """clg_packed whose arrays have GUARD bytes of FILL either side."""
    from clonos_amd import _lib
    o_bits = (2 * GUARD + cap_desc * 32 + 63) & ~63
    reg = Region(kind, o_bits + cap_bits + 2 * GUARD)
    p = _lib.Packed()
    p.desc, p.cap_desc = reg.ptr + GUARD, cap_desc
    p.bits, p.cap_bits = reg.ptr + o_bits + GUARD, cap_bits
    p.out_kind = KIND[kind]
    return p, reg, o_bits


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("in_kind", ["host", "device", "mapped"])
def test_inputs_and_outputs_in_every_memory(eng, in_kind, out_kind):
    from clonos_amd import _lib, pack_columns_host
    cols = mixed_columns(0, 21, [2500, 1100, 1300, 1025, 40])
    want = pack_columns_host(cols)
    nb, nbits = want.desc.size, want.bits.size
    cin, rin = columns_in(cols, in_kind)
    p, rout, o_bits = packed_out(out_kind, nb + 3, nbits + 48)
    try:
        assert eng.pack_columns_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == nbits
        raw = rout.get()
        assert raw[GUARD:GUARD + nb * 32].tobytes() == np.asarray(want.desc).tobytes()
        assert raw[o_bits + GUARD:o_bits + GUARD + nbits].tobytes() == np.asarray(want.bits).tobytes()
        raw[GUARD:GUARD + nb * 32] = FILL
        raw[o_bits + GUARD:o_bits + GUARD + nbits] = FILL
        assert (raw == FILL).all()  # nothing outside what was asked for, the spare capacity included
    finally:
        rin.free()
        rout.free()


def test_sizes_only(eng):
    from clonos_amd import _lib, pack_columns_host
    cols = mixed_columns(1500, 31)
    want = pack_columns_host(cols)
    cin, rin = columns_in(cols, "device")
    p = _lib.Packed()
    try:
        assert eng.pack_columns_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size
    finally:
        rin.free()


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("short", ["desc", "bits"])
def test_capacity_leaves_the_outputs_untouched(eng, short, out_kind):
    from clonos_amd import _lib, pack_columns_host
    cols = mixed_columns(2100, 41)
    want = pack_columns_host(cols)
    nb, nbits = want.desc.size, want.bits.size
    cin, rin = columns_in(cols, "host")
    p, rout, _ = packed_out(out_kind, nb - (short == "desc"), nbits - (short == "bits"))
    try:
        assert eng.pack_columns_raw(cin, p) == _lib.CLG_E_CAPACITY
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == nbits
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()


def test_unaligned_device_outputs_are_rejected(eng):
    from clonos_amd import _lib
    cols = mixed_columns(100, 51)
    cin, rin = columns_in(cols, "host")
    p, rout, _ = packed_out("device", 8, 4096)
    p.bits += 8
    try:
        assert eng.pack_columns_raw(cin, p) == _lib.CLG_E_INVALID_ARG
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()


def test_the_stat_is_recorded(eng):
    eng.kernel_stats_reset()
    eng.pack_columns(mixed_columns(3000, 61))
    st = eng.kernel_stats()
    assert st["pack_columns"]["launches"] >= 2 and st["pack_columns"]["bytes"] > 0 and st["pack_columns"]["ms"] > 0
