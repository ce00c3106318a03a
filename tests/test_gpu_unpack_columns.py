"""GPU: clg_unpack_columns.  Every comparison is exact against unpack_packed_host
(clg_unpack_columns_all_host, which tests/test_unpack_host.py and tests/unpack_host.cpp hold to the
format): values, statuses and (what, stream, block) alike.  There is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from _pack_util import STREAMS, Narrow, values_of_width
from test_gpu_pack_columns import FILL, GUARD, KIND, Region, every_width_columns, mixed_columns

pytestmark = pytest.mark.gpu

ELEM = (1, 1, 8, 4, 4)
CAPS = ("cap_tag", "cap_order", "cap_timestamp", "cap_rng", "cap_buffer_built")


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as e:
        yield e


def assert_unpacks_to(eng, packed, cols=None):
    """The device unpack of host packed columns equals the CPU version's, array for array (and the
    columns they were packed from)."""
    from clonos_amd import unpack_packed_host
    want = unpack_packed_host(packed)
    got = eng.unpack_columns(packed)
    for name, dt, _ in STREAMS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype == dt and a.shape == b.shape and (a == b).all(), name
        if cols is not None:
            assert (a == np.asarray(getattr(cols, name), dt)).all(), name
    return got


def test_every_width(eng):
    from clonos_amd import pack_columns_host
    cols = every_width_columns()
    packed = pack_columns_host(cols)
    d = np.asarray(packed.desc)
    for c, widths in enumerate((range(4), range(9), range(65), range(33), reversed(range(33)))):
        assert list(d["width"][packed.blk_base[c]:packed.blk_base[c + 1]]) == list(widths)
    assert_unpacks_to(eng, packed, cols)


@pytest.mark.parametrize("width", [31, 32, 33, 63, 64])
@pytest.mark.parametrize("n", [1023, 1025])
def test_word_seams_with_a_short_last_block(eng, width, n):
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(width * 4096 + n + 1)
    cols = Narrow(timestamp=values_of_width(rng, np.int64, width, n, delta=True),
                  rng=values_of_width(rng, np.int32, min(width, 32), n))
    assert_unpacks_to(eng, pack_columns_host(cols), cols)


def test_int64_extremes_side_by_side(eng):
    from clonos_amd import pack_columns_host
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    cols = Narrow(timestamp=np.array([lo, hi, lo, 0, hi, hi, lo, -1, 1] * 150, np.int64),
                  rng=np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1] * 300, np.int32), order=np.array([-128, 127, 0] * 400, np.int8),
                  tag=np.array([0, 255, 7] * 400, np.uint8))
    assert_unpacks_to(eng, pack_columns_host(cols), cols)


@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 1])
def test_stream_lengths(eng, n):
    from clonos_amd import pack_columns_host
    cols = mixed_columns(n, 200 + n)
    got = assert_unpacks_to(eng, pack_columns_host(cols), cols)
    assert got.n_rec == n and all(len(getattr(got, name)) == n for name, _, _ in STREAMS)


@pytest.mark.parametrize("lens", [[2049, 0, 0, 0, 0], [0, 0, 1500, 0, 0], [0, 700, 0, 0, 1], [5, 0, 1025, 0, 3000],
                                  [0, 0, 0, 0, 0]])
def test_some_and_all_streams_empty(eng, lens):
    from clonos_amd import pack_columns_host
    cols = mixed_columns(0, 8, lens)
    got = assert_unpacks_to(eng, pack_columns_host(cols), cols)
    assert [len(getattr(got, name)) for name, _, _ in STREAMS] == lens


def test_the_grid_passes_a_256_block_boundary(eng):
    """257 blocks of tags and a block of each other stream."""
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(0x5CAA)
    cols = mixed_columns(0, 12, [0, 600, 900, 1024, 77])
    cols.tag = rng.integers(0, 8, 256 * 1024 + 1).astype(np.uint8)
    packed = pack_columns_host(cols)
    assert packed.blk_base == [0, 257, 258, 259, 260, 261]
    assert_unpacks_to(eng, packed, cols)


def sizes_of(packed):
    """Each block's payload bytes."""
    d = np.asarray(packed.desc)
    k = d["count"].astype(np.int64)
    k[packed.blk_base[2]:packed.blk_base[3]] -= 1
    return 16 * ((k * d["width"].astype(np.int64) + 127) // 128)


def test_payload_order_differs_from_block_order(eng):
    from clonos_amd import pack_columns_host
    cols = mixed_columns(0, 13, [2500, 1100, 3073, 1025, 40])
    packed = pack_columns_host(cols)
    size, old = sizes_of(packed), np.asarray(packed.bits)
    desc, bits, pos = packed.desc.copy(), np.empty_like(old), 0
    for b in np.random.default_rng(5).permutation(desc.size):
        bits[pos:pos + size[b]] = old[int(desc["pos"][b]):int(desc["pos"][b]) + size[b]]
        desc["pos"][b] = pos
        pos += int(size[b])
    assert pos == old.size and (np.diff(desc["pos"].astype(np.int64)) < 0).any()
    packed.desc, packed.bits = desc, bits
    assert_unpacks_to(eng, packed, cols)


def test_two_blocks_share_one_payload(eng):
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(6)
    cols = Narrow(rng=np.tile(rng.integers(-5000, 5000, 1024).astype(np.int32), 2),
                  timestamp=np.tile(np.cumsum(rng.integers(0, 50, 1024)), 2))
    packed = pack_columns_host(cols)
    desc = packed.desc.copy()
    for c in (2, 3):
        b = packed.blk_base[c]
        assert desc["width"][b] == desc["width"][b + 1] and desc["ref"][b] == desc["ref"][b + 1]
        desc["pos"][b + 1] = desc["pos"][b]
    packed.desc = desc
    assert_unpacks_to(eng, packed, cols)


# ---- where the arrays live ------------------------------------------------------------------
class PackedIn:
    """A packed input's desc and bits in memory of `kind`; exact: bits is a device allocation of
    exactly its length, so a read past it leaves the allocation."""

    def __init__(self, desc, bits, st, kind, exact=False):
        from clonos_amd import _lib
        self.regions = []
        p = _lib.Packed()
        C.memmove(C.byref(p), C.byref(st), C.sizeof(p))
        self.keep = (np.ascontiguousarray(desc), np.ascontiguousarray(bits))
        nb, nbits = self.keep[0].size, self.keep[1].size
        if kind == "host":
            ptrs = [self.keep[0].ctypes.data, self.keep[1].ctypes.data]
        elif exact:
            rd, rb = Region(kind, max(nb * 32, 16)), Region(kind, max(nbits, 16))
            rd.put(0, self.keep[0]), rb.put(0, self.keep[1])
            self.regions, ptrs = [rd, rb], [rd.ptr, rb.ptr]
        else:
            o_bits = (nb * 32 + 63) & ~63
            r = Region(kind, o_bits + max(nbits, 16) + 64)
            r.put(0, self.keep[0]), r.put(o_bits, self.keep[1])
            self.regions, ptrs = [r], [r.ptr, r.ptr + o_bits]
        p.desc = ptrs[0] if st.desc else None
        p.bits = ptrs[1] if st.bits else None
        p.out_kind = KIND[kind]
        self.p = p

    def free(self):
        for r in self.regions:
            r.free()


class ColumnsOut:
    """clg_columns whose five narrow arrays have GUARD bytes of FILL either side, in one region."""

    def __init__(self, kind, caps):
        from clonos_amd import _lib
        self.at, total = [], 0
        for cap, el in zip(caps, ELEM):
            self.at.append(total + GUARD)
            total += (2 * GUARD + cap * el + 63) & ~63
        self.reg = Region(kind, total)
        c = _lib.Columns()
        for (name, _, _), o, cap, cn in zip(STREAMS, self.at, caps, CAPS):
            setattr(c, name, self.reg.ptr + o)
            setattr(c, cn, cap)
        c.out_kind = KIND[kind]
        c.n_class[4], c.err_status, c.cap_wide = 77, -5, 9  # what the unpack leaves alone
        self.c = c

    def untouched(self):
        return bool((self.reg.get() == FILL).all()) and (self.c.n_class[4], self.c.err_status, self.c.cap_wide) == (77, -5, 9)

    def holds(self, want):
        """The arrays are want's and no byte outside [0, n) of any of them was written."""
        raw = self.reg.get()
        for (name, dt, _), o in zip(STREAMS, self.at):
            a = np.ascontiguousarray(getattr(want, name), dt)
            if raw[o:o + a.nbytes].tobytes() != a.tobytes():
                return False
            raw[o:o + a.nbytes] = FILL
        return bool((raw == FILL).all()) and (self.c.n_class[4], self.c.err_status) == (77, -5)

    def free(self):
        self.reg.free()


def sizes_match(c, packed):
    return [int(c.n_rec)] + [int(c.n_class[k]) for k in range(4)] == packed.n_val


IO_COLS = mixed_columns(0, 22, [2500, 1100, 1300, 1025, 40])


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("in_kind", ["host", "device", "mapped"])
def test_inputs_and_outputs_in_every_memory(eng, in_kind, out_kind):
    from clonos_amd import _lib, pack_columns_host, unpack_packed_host
    packed = pack_columns_host(IO_COLS)
    want = unpack_packed_host(packed)
    pin = PackedIn(packed.desc, packed.bits, packed._struct(), in_kind)
    out = ColumnsOut(out_kind, [n + 3 for n in packed.n_val])
    bad = _lib.UnpackBad(9, 9, 9)
    try:
        assert eng.unpack_columns_raw(pin.p, out.c, bad) == _lib.CLG_OK
        assert (bad.what, bad.stream, bad.block) == (0, 0, 2 ** 64 - 1) and sizes_match(out.c, packed)
        assert out.holds(want)  # nothing outside [0, n) of each array, the spare capacity included
    finally:
        pin.free()
        out.free()


def test_sizes_only(eng):
    from clonos_amd import _lib, pack_columns_host
    packed = pack_columns_host(mixed_columns(1500, 32))
    pin = PackedIn(packed.desc, packed.bits, packed._struct(), "device")
    c, bad = _lib.Columns(), _lib.UnpackBad()
    try:
        assert eng.unpack_columns_raw(pin.p, c, bad) == _lib.CLG_OK and sizes_match(c, packed)
    finally:
        pin.free()


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("short", range(5))
def test_capacity_leaves_the_outputs_untouched(eng, short, out_kind):
    from clonos_amd import _lib, pack_columns_host
    packed = pack_columns_host(mixed_columns(2100, 42))
    pin = PackedIn(packed.desc, packed.bits, packed._struct(), "host")
    out = ColumnsOut(out_kind, [n - (c == short) for c, n in enumerate(packed.n_val)])
    bad = _lib.UnpackBad()
    try:
        assert eng.unpack_columns_raw(pin.p, out.c, bad) == _lib.CLG_E_CAPACITY
        assert sizes_match(out.c, packed) and out.untouched() and bad.what == 0
    finally:
        out.free()


def test_misaligned_device_arrays_are_rejected(eng):
    from clonos_amd import _lib, pack_columns_host
    packed = pack_columns_host(mixed_columns(1100, 52))
    for shift_in, field, shift_out in ((8, None, 0), (0, "timestamp", 4), (0, "rng", 2), (0, "buffer_built", 1)):
        pin = PackedIn(packed.desc, packed.bits, packed._struct(), "device")
        out = ColumnsOut("device", [n + 8 for n in packed.n_val])
        pin.p.bits += shift_in
        if field:
            setattr(out.c, field, getattr(out.c, field) + shift_out)
        try:
            assert eng.unpack_columns_raw(pin.p, out.c, _lib.UnpackBad()) == _lib.CLG_E_INVALID_ARG
            assert out.untouched()
        finally:
            pin.free()
            out.free()


# ---- malformed input: the bytes may come from another process ---------------------------------
def malformed_columns():
    rng = np.random.default_rng(0xBAD)
    return Narrow(tag=rng.integers(0, 8, 1500).astype(np.uint8), order=rng.integers(0, 4, 1500).astype(np.int8),
                  timestamp=np.cumsum(rng.integers(0, 1000, 2500)).astype(np.int64),
                  rng=rng.integers(0, 100000, 2500).astype(np.int32))


B1, B2, B3 = 2, 4, 7  # blk_base of the order, timestamp and rng streams above


def _set(field, b, v):
    def f(d, p):
        d[field][b] = v
    return f


def _add(field, b, v):
    def f(d, p):
        d[field][b] = int(d[field][b]) + v
    return f


def _p(**kw):
    def f(d, p):
        for k, v in kw.items():
            if "[" in k:
                name, i = k[:-1].split("[")
                getattr(p, name)[int(i)] = v(p) if callable(v) else v
            else:
                setattr(p, k, v(p) if callable(v) else v)
    return f


def _both(*fs):
    def f(d, p):
        for g in fs:
            g(d, p)
    return f


# every case of tests/unpack_host.cpp::malformed, by name
MALFORMED = {
    "width_65": _set("width", B2 + 1, 65),
    "width_all_ones": _set("width", B2 + 1, 0xFFFFFFFF),
    "count_0": _set("count", B2, 0),
    "count_1025": _set("count", B2, 1025),
    "count_1023_not_last": _set("count", B2, 1023),
    "count_last_453": _set("count", B2 + 2, 453),
    "count_last_1024": _set("count", B2 + 2, 1024),
    "pos_at_n_bits": lambda d, p: d["pos"].__setitem__(B2 + 2, p.n_bits),
    "pos_wraps": _set("pos", B2 + 2, 2 ** 64 - 16),
    "width_64_passes_n_bits": _set("width", B3 + 2, 64),
    "pos_plus_8": _add("pos", B3 + 1, 8),
    "pos_minus_15": _add("pos", B2 + 1, -15),
    "two_blocks_lower_stream": _both(_set("width", B3, 65), _set("count", 1, 7)),
    "two_blocks_lower_block": _both(_set("width", B3 + 2, 65), _set("count", B3 + 1, 7)),
    "value_and_block": _both(_set("ref", 0, 250), _set("width", B3 + 2, 99)),
    "n_bits_16": _p(n_bits=16),
    "n_bits_past_cap": _p(n_bits=lambda p: p.cap_bits + 16),
    "blk_base_3_plus_1": _p(**{"blk_base[3]": lambda p: p.blk_base[3] + 1}),
    "blk_base_decreases": _p(**{"blk_base[2]": lambda p: p.blk_base[3] + 1}),
    "blk_base_0": _p(**{"blk_base[0]": 1}),
    "cap_desc_short": _p(cap_desc=lambda p: p.blk_base[5] - 1),
    "n_val_2_plus_1024": _p(**{"n_val[2]": 2500 + 1024}),
    "n_val_4": _p(**{"n_val[4]": 1}),
    "n_val_1_huge": _p(**{"n_val[1]": 2 ** 64 - 1}),
    "desc_null": _p(desc=None),
    "bits_null": _p(bits=None),
    "layout_and_block": _both(_p(**{"blk_base[3]": lambda p: p.blk_base[3] + 1}), _set("width", 0, 65)),
    "rng_above": _set("ref", B3, 2 ** 31 - 1 - 5),
    "rng_below": _set("ref", B3 + 1, -2 ** 31 - 1),
    "tag_above": _set("ref", 0, 250),
    "tag_below": _set("ref", 1, -1),
    "order_above": _set("ref", B1, 126),
    "order_below": _set("ref", B1 + 1, -131),
    "ref_int64_max": _set("ref", B3 + 2, 2 ** 63 - 1),
    "ref_int64_min": _set("ref", B3 + 2, -2 ** 63),
    "two_values_lower": _both(_set("ref", B3 + 1, 2 ** 31 - 1), _set("ref", 0, 253)),
}
# what the CPU program asserts for them, so that the table and the program cannot drift apart unseen
EXPECT = {
    "width_65": (2, 2, 1), "count_last_453": (2, 2, 2), "pos_plus_8": (2, 3, 1), "two_blocks_lower_stream": (2, 0, 1),
    "value_and_block": (2, 3, 2), "n_bits_16": (2, 0, 0), "blk_base_decreases": (1, 1, 0), "n_val_4": (1, 4, 0),
    "layout_and_block": (1, 2, 0), "rng_below": (3, 3, 1), "order_above": (3, 1, 0), "two_values_lower": (3, 0, 0),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_input_is_rejected_as_the_cpu_version_rejects_it(eng, name):
    """The input in device memory, bits an allocation of exactly n_bits bytes: a pos or a width
    that reached past it would leave the allocation."""
    from clonos_amd import _lib, pack_columns_host
    from clonos_amd.engine import _unpack_out
    packed = pack_columns_host(malformed_columns())
    assert packed.blk_base == [0, B1, B2, B3, 10, 10]
    desc, st = packed.desc.copy(), packed._struct()
    st.desc = desc.ctypes.data
    MALFORMED[name](desc, st)
    hc, keep = _unpack_out(packed.n_val)
    hbad = _lib.UnpackBad(9, 9, 9)
    hst = _lib.lib.clg_unpack_columns_all_host(C.byref(st), C.byref(hc), C.byref(hbad))
    want = (hst, hbad.what, hbad.stream, hbad.block)
    assert hst == _lib.CLG_E_INVALID_ARG and hbad.what != 0
    if name in EXPECT:
        assert want[1:] == EXPECT[name]
    pin = PackedIn(desc, packed.bits, st, "device", exact=True)
    out = ColumnsOut("device", [n + 3 for n in packed.n_val])
    bad = _lib.UnpackBad(9, 9, 9)
    try:
        got = eng.unpack_columns_raw(pin.p, out.c, bad)
        assert (got, bad.what, bad.stream, bad.block) == want
        assert out.untouched()
    finally:
        pin.free()
        out.free()


@pytest.mark.parametrize("kinds", [("host", "host"), ("mapped", "mapped"), ("host", "device")])
def test_a_rejection_writes_nothing_whatever_the_kinds(eng, kinds):
    from clonos_amd import _lib, pack_columns_host
    packed = pack_columns_host(malformed_columns())
    desc = packed.desc.copy()
    desc["ref"][B3 + 2] = 2 ** 31 - 10  # the last block of the last stream that holds values
    pin = PackedIn(desc, packed.bits, packed._struct(), kinds[0])
    out = ColumnsOut(kinds[1], packed.n_val)
    bad = _lib.UnpackBad()
    try:
        assert eng.unpack_columns_raw(pin.p, out.c, bad) == _lib.CLG_E_INVALID_ARG
        assert (bad.what, bad.stream, bad.block) == (_lib.UNPACK_BAD_VALUE, 3, 2) and out.untouched()
    finally:
        pin.free()
        out.free()


def test_errors_raise_with_what_stream_and_block(eng):
    from clonos_amd import ClonosError, _lib, pack_columns_host
    packed = pack_columns_host(malformed_columns())
    desc = packed.desc.copy()
    desc["pos"][B3] += 8
    packed.desc = desc
    with pytest.raises(ClonosError) as ei:
        eng.unpack_columns(packed)
    e = ei.value
    assert (e.status, e.bad_what, e.bad_stream, e.bad_block) == (_lib.CLG_E_INVALID_ARG, _lib.UNPACK_BAD_BLOCK, 3, 0)


def test_the_wide_rows_and_the_payload_column_are_passed_through(eng):
    from _columns_util import assert_columns_equal, oracle_batch
    from clonos_amd import columnize_host, pack_columns_host, synth
    rng = np.random.default_rng(0x9AD)
    cols = columnize_host(oracle_batch([b"", synth.random_log(700, rng, allow_serializable=True), b""]))
    packed = pack_columns_host(cols)
    got = eng.unpack_columns(packed)
    assert_columns_equal(got, cols)
    assert got.w_v0 is packed.w_v0 and got.var is packed.var and got.var_pos is packed.var_pos


def test_the_stat_is_recorded(eng):
    from clonos_amd import pack_columns_host
    eng.kernel_stats_reset()
    eng.unpack_columns(pack_columns_host(mixed_columns(3000, 62)))
    st = eng.kernel_stats()
    assert st["unpack_columns"]["launches"] >= 2 and st["unpack_columns"]["bytes"] > 0 and st["unpack_columns"]["ms"] > 0
