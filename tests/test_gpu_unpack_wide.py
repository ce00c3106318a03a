"""GPU: clg_unpack_wide.  Every comparison is exact, against unpack_wide_host (which
tests/test_wpack_host.py holds to the round trip of an independent packer): values, statuses and
(what, stream, block) alike; pos against numpy.cumsum.  The shapes are the smallest that reach each
seam: a tile of the kind and merge passes is 1024 rows, a block 1024 values, a wave 64, a
workgroup's quarter 256, a round of the one-workgroup scans 1024 tiles."""
import ctypes as C

import numpy as np
import pytest

from _wpack_util import WIDE, WIDE_DT, Wide, seeded_wide, width_scene
from test_gpu_pack_wide import FILL, GUARD, KIND, Region

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
DELTA = [False, True] + [f in (1, 2) or (f == 5 and k != 0) for k in range(4) for f in range(6)]


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as e:
        yield e


def unpacks_as_host(eng, packed, cols=None):
    from clonos_amd import unpack_wide_host
    want = unpack_wide_host(packed)
    got = eng.unpack_wide(packed, pos=True)
    for name, dt in zip(WIDE, WIDE_DT):
        assert got[name].dtype == dt and got[name].shape == want[name].shape and (got[name] == want[name]).all(), name
        if cols is not None:
            assert (got[name] == np.asarray(getattr(cols, name), dt)).all(), name
    pos = np.zeros(packed.n_wide + 1, np.uint64)
    np.cumsum(want["w_var_len"], dtype=np.uint64, out=pos[1:])
    assert got["pos"].dtype == np.uint64 and (got["pos"] == pos).all()
    plain = eng.unpack_wide(packed)
    assert "pos" not in plain and all((plain[k] == want[k]).all() for k in WIDE)
    return got


def same_as_host(eng, cols):
    from clonos_amd import pack_wide_host
    return unpacks_as_host(eng, pack_wide_host(cols), cols)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_row_counts_across_the_tile_seam(eng, n):
    kinds = np.random.default_rng(n).integers(0, 4, n)
    got = same_as_host(eng, seeded_wide(kinds, 100 + n, gap=2))
    assert got["w_idx"].size == n and got["pos"].size == n + 1


@pytest.mark.parametrize("count", [0, 1, 1024, 1025])
@pytest.mark.parametrize("kind", range(4))
def test_each_kinds_count_at_the_block_seam(eng, kind, count):
    """`count` rows of one kind spread among 700 of each other kind: a rank crosses its kind's block
    seam inside a tile."""
    rng = np.random.default_rng(17 * kind + count)
    kinds = np.concatenate([np.full(count, kind), np.repeat([k for k in range(4) if k != kind], 700)])
    rng.shuffle(kinds)
    same_as_host(eng, seeded_wide(kinds, 7 + count))


@pytest.mark.parametrize("kind", range(4))
def test_rows_of_one_kind_only(eng, kind):
    same_as_host(eng, seeded_wide(np.full(1500, kind), 31 + kind))


@pytest.mark.parametrize("run", [1, 64, 65, 256])
def test_kinds_in_runs_across_the_wave_and_workgroup_seams(eng, run):
    kinds = (np.arange(3 * 1024 + 77) // run) % 4
    same_as_host(eng, seeded_wide(kinds, 500 + run))


@pytest.mark.parametrize("width", range(65))
def test_width_scenes(eng, width):
    """A full block of every field of every kind at every width: every (element, scheme) instance of
    the decode at every width it can meet."""
    same_as_host(eng, width_scene(width))


@pytest.mark.parametrize("n", [1023, 1025])
def test_word_seams_with_a_short_last_block(eng, n):
    for width in (31, 33, 63, 64):
        same_as_host(eng, width_scene(width, n=n))


def test_int64_extremes_side_by_side_and_offsets_up_to_the_last_byte(eng):
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    n = 1350
    kinds = np.arange(n) % 4
    off = np.concatenate([np.arange(9, 9 + 13 * 450, 13), np.arange(1, 1 + 7 * 450, 7), 2 ** 32 - 1 - np.arange(450)[::-1]])
    v0 = np.resize(np.array([lo, hi, lo, 0, hi, hi, lo, -1, 1], np.int64), n)
    cols = Wide(kinds, w_var_off=off, w_v0=v0, w_v1=v0[::-1], w_var_len=np.resize([2 ** 32 - 1, 0, 5], n),
                w_rc=np.resize([-2 ** 31, 2 ** 31 - 1], n), w_sub=np.resize([255, 0, 1], n))
    got = same_as_host(eng, cols)
    assert got["w_var_off"].max() == 2 ** 32 - 1


def test_pos_carries_past_32_bits(eng):
    """w_var_len of 2^32 - 1 in consecutive rows, inside a thread's four rows, across waves and
    across the tile seam."""
    n = 2100
    length = np.full(n, 3, np.uint32)
    length[[0, 1, 2, 3, 62, 63, 64, 65, 255, 256, 1022, 1023, 1024, 1025, 2098, 2099]] = 2 ** 32 - 1
    got = same_as_host(eng, Wide(np.arange(n) % 4, w_var_len=length))
    assert int(got["pos"][4]) == 4 * (2 ** 32 - 1) and int(got["pos"][-1]) > 16 * (2 ** 32 - 2)


def payload_bytes(packed, b):
    stream = int(np.searchsorted(packed.blk_base, b, side="right")) - 1
    d = packed.desc[b]
    k = int(d["count"]) - (1 if DELTA[stream] else 0)
    return 16 * ((k * int(d["width"]) + 127) // 128)


def test_payloads_in_permuted_order(eng):
    """The blocks' payloads laid out in the reverse of block order."""
    from clonos_amd import pack_wide_host
    cols = seeded_wide(np.random.default_rng(8).integers(0, 4, 3000), 9)
    packed = pack_wide_host(cols)
    bits, desc, at = np.zeros_like(packed.bits), packed.desc.copy(), 0
    for b in reversed(range(desc.size)):
        nby, src = payload_bytes(packed, b), int(packed.desc["pos"][b])
        bits[at:at + nby] = packed.bits[src:src + nby]
        desc["pos"][b] = at
        at += nby
    assert at == bits.size and (np.diff(desc["pos"].astype(np.int64)) <= 0).all()
    packed.desc, packed.bits = desc, bits
    unpacks_as_host(eng, packed, cols)


def test_two_blocks_share_one_payload(eng):
    from clonos_amd import pack_wide_host
    n = 2048
    rc = np.tile(np.random.default_rng(4).integers(0, 1 << 20, 1024), 2)
    cols = Wide(np.zeros(n, np.uint8), w_rc=rc, w_var_len=np.arange(n) % 7)
    packed = pack_wide_host(cols)
    b0 = packed.blk_base[2]
    assert packed.blk_base[3] - b0 == 2 and packed.desc["width"][b0] == packed.desc["width"][b0 + 1] > 0
    desc = packed.desc.copy()
    desc["pos"][b0 + 1] = desc["pos"][b0]
    packed.desc = desc
    unpacks_as_host(eng, packed, cols)


def test_more_than_256_blocks(eng):
    from clonos_amd import pack_wide_host
    kinds = np.random.default_rng(5).integers(0, 4, 36 * 1024 + 9)
    packed = pack_wide_host(seeded_wide(kinds, 9))
    assert packed.blk_base[-1] > 256
    unpacks_as_host(eng, packed)


def test_one_tile_more_than_a_round_of_the_tile_scans(eng):
    """1024 x 1024 + 1 rows: the kind counts' scan and the tile sums' scan both take a second round.
    Every field but w_var_len is constant, so the host's side stays in seconds."""
    from clonos_amd import pack_wide_host
    n = 1024 * 1024 + 1
    cols = Wide((np.arange(n) // 3) % 4, gap=0, w_var_len=np.arange(n, dtype=np.uint64) % 1000 + (2 ** 32 - 1000))
    got = unpacks_as_host(eng, pack_wide_host(cols), cols)
    assert int(got["pos"][-1]) > 2 ** 51


# ---- where the arrays live ------------------------------------------------------------------
class WideIn:
    """A packed input's desc and bits in memory of `kind`; exact: bits is an allocation of exactly
    its length, so a read past it leaves the allocation."""

    def __init__(self, packed, kind, exact=False, st=None):
        from clonos_amd import _lib
        st = st or packed._struct()
        p = _lib.PackedWideC()
        C.memmove(C.byref(p), C.byref(st), C.sizeof(p))
        self.keep = (np.ascontiguousarray(packed.desc), np.ascontiguousarray(packed.bits))
        nb, nbits = self.keep[0].size, self.keep[1].size
        self.regions = []
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


OUT = tuple(zip(WIDE, WIDE_DT)) + (("pos", np.uint64),)


class WideOut:
    """clg_columns whose seven wide arrays, and pos, have GUARD bytes of FILL either side."""

    def __init__(self, kind, cap, pos=True):
        from clonos_amd import _lib
        self.at, total = {}, 0
        for name, dt in OUT:
            self.at[name] = total + GUARD
            total += (2 * GUARD + (cap + 1) * np.dtype(dt).itemsize + 63) & ~63
        self.reg = Region(kind, total)
        c = _lib.Columns()
        for name in WIDE:
            setattr(c, name, self.reg.ptr + self.at[name])
        c.cap_wide, c.out_kind = cap, KIND[kind]
        c.n_rec, c.n_class[0], c.err_status, c.cap_tag = 77, 5, -5, 9  # what the unpack leaves alone
        self.c = c
        self.pos = self.reg.ptr + self.at["pos"] if pos else None

    def alone(self):
        return (self.c.n_rec, self.c.n_class[0], self.c.err_status, self.c.cap_tag) == (77, 5, -5, 9)

    def untouched(self):
        return bool((self.reg.get() == FILL).all()) and self.alone()

    def holds(self, want, pos):
        """The arrays are want's, pos is pos, and no byte outside them was written."""
        raw = self.reg.get()
        for name, dt in OUT:
            a = np.ascontiguousarray(pos if name == "pos" else want[name], dt)
            o = self.at[name]
            if raw[o:o + a.nbytes].tobytes() != a.tobytes():
                return False
            raw[o:o + a.nbytes] = FILL
        return bool((raw == FILL).all()) and self.alone()

    def free(self):
        self.reg.free()


def scene():
    return seeded_wide(np.random.default_rng(21).integers(0, 4, 2500), 22, gap=3)


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("in_kind", ["host", "device", "mapped"])
def test_inputs_and_outputs_in_every_memory(eng, in_kind, out_kind):
    from clonos_amd import _lib, pack_wide_host, unpack_wide_host
    packed = pack_wide_host(scene())
    want = unpack_wide_host(packed)
    pos = np.concatenate([[0], np.cumsum(want["w_var_len"], dtype=np.uint64)]).astype(np.uint64)
    pin, out = WideIn(packed, in_kind), WideOut(out_kind, packed.n_wide + 3)
    bad = _lib.UnpackBad(9, 9, 9)
    try:
        assert eng.unpack_wide_raw(pin.p, out.c, out.pos, bad) == _lib.CLG_OK
        assert (bad.what, bad.stream, bad.block) == (0, 0, NONE) and out.c.n_class[4] == packed.n_wide
        assert out.holds(want, pos)  # nothing outside [0, n) of each array or [0, n] of pos, the spare capacity included
    finally:
        pin.free()
        out.free()


def test_sizes_only(eng):
    from clonos_amd import _lib, pack_wide_host
    packed = pack_wide_host(scene())
    pin = WideIn(packed, "device")
    c, bad = _lib.Columns(), _lib.UnpackBad()
    try:
        assert eng.unpack_wide_raw(pin.p, c, None, bad) == _lib.CLG_OK and c.n_class[4] == packed.n_wide
    finally:
        pin.free()


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("short", WIDE + ("cap_wide",))
def test_capacity_leaves_the_outputs_untouched(eng, short, out_kind):
    """Each of the seven arrays absent (a NULL array holds nothing), and cap_wide one short, which
    is every array's and pos's capacity (cap_wide + 1 entries)."""
    from clonos_amd import _lib, pack_wide_host
    packed = pack_wide_host(scene())
    pin = WideIn(packed, "host")
    out = WideOut(out_kind, packed.n_wide - (short == "cap_wide"))
    if short != "cap_wide":
        setattr(out.c, short, None)
    bad = _lib.UnpackBad()
    try:
        assert eng.unpack_wide_raw(pin.p, out.c, out.pos, bad) == _lib.CLG_E_CAPACITY
        assert out.c.n_class[4] == packed.n_wide and out.untouched() and bad.what == 0
    finally:
        out.free()


def test_misaligned_device_arrays_are_rejected(eng):
    from clonos_amd import _lib, pack_wide_host
    packed = pack_wide_host(scene())
    for shift_in, field, shift_out in ((8, None, 0), (0, "w_v1", 4), (0, "w_rc", 2), (0, "pos", 4)):
        pin, out = WideIn(packed, "device"), WideOut("device", packed.n_wide + 8)
        pin.p.bits += shift_in
        if field == "pos":
            out.pos += shift_out
        elif field:
            setattr(out.c, field, getattr(out.c, field) + shift_out)
        try:
            assert eng.unpack_wide_raw(pin.p, out.c, out.pos, _lib.UnpackBad()) == _lib.CLG_E_INVALID_ARG
            assert out.untouched()
        finally:
            pin.free()
            out.free()


# ---- rejections: those of tests/test_wpack_host.py's unpack test, and pos % 16 ------------------
def rejection_scene():
    from clonos_amd import pack_wide_host
    return pack_wide_host(seeded_wide(np.random.default_rng(3).integers(0, 4, 2500), 7))


def _desc(field, stream, block, value):
    def poke(packed, st):
        packed.desc[field][packed.blk_base[stream] + block] = value
    return poke


def _st(**kw):
    def poke(packed, st):
        for k, (i, d) in kw.items():
            if i is None:
                setattr(st, k, getattr(st, k) + d)
            else:
                getattr(st, k)[i] += d
    return poke


def _both(*fs):
    def poke(packed, st):
        for f in fs:
            f(packed, st)
    return poke


def _flip_first_kind(packed, st):
    packed.bits[0] = (int(packed.bits[0]) & 0xFC) | ((int(packed.bits[0]) + 1) & 3)


REJECTIONS = {
    "blk_base_0": _st(blk_base=(0, 1)),
    "blk_base_7": _st(blk_base=(7, 1)),
    "n_val_9": _st(n_val=(9, 1024)),
    "kind_and_idx_differ": _st(n_val=(1, -1)),
    "a_kinds_streams_differ": _st(n_val=(2 + 3, -1)),
    "the_last_stream_differs": _st(n_val=(2 + 18 + 5, 1)),
    "the_kinds_do_not_sum": _both(_st(n_val=(0, -1)), _st(n_val=(1, -1))),
    "cap_desc": _st(cap_desc=(None, -1)),
    "n_bits_past_cap_bits": _st(n_bits=(None, 1 << 20)),
    "width_65": _desc("width", 1, 2, 65),
    "count_1023": _desc("count", 0, 0, 1023),
    "pos_8": _desc("pos", 4, 0, 8),
    "pos_not_16": _desc("pos", 2 + 12 + 5, 0, 24),
    "pos_past_the_bits": _desc("pos", 2 + 6 + 1, 0, 1 << 40),
    "width_reaches_past_the_bits": _desc("width", 25, 0, 64),
    "block_before_a_lower_value": _both(_desc("ref", 0, 0, 3), _desc("width", 20, 0, 99)),
    "a_kind_of_4": _desc("ref", 0, 1, 1),
    "histogram": _flip_first_kind,
    "histogram_before_a_later_value": _both(_flip_first_kind, _desc("first", 2 + 6 + 2, 0, -1)),
    "var_off_high": _desc("first", 2 + 6 + 2, 0, 2 ** 32 - 4),
    "var_off_negative": _desc("first", 2 + 6 + 2, 0, -1),
    "var_len_high": _desc("ref", 2 + 12 + 3, 0, 2 ** 32 - 1),
    "var_len_negative": _desc("ref", 2 + 12 + 3, 0, -1),
    "idx_high": _desc("first", 1, 0, 2 ** 32),
    "idx_climbs_out_in_a_later_block": _desc("first", 1, 2, 2 ** 32 - 3),
    "rc_high": _desc("ref", 2 + 0, 0, 2 ** 31 - 5),
    "rc_low": _desc("ref", 2 + 0, 0, -2 ** 31 - 1),
    "sub_high": _desc("ref", 2 + 18 + 4, 0, 255),
    "the_lowest_of_two_values": _both(_desc("ref", 2 + 18 + 4, 0, 255), _desc("ref", 2 + 6 + 0, 0, 2 ** 31 - 5)),
}


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_every_rejection_is_the_host_calls_and_writes_nothing(eng, name):
    """The input is in device memory, bits an allocation of exactly n_bits bytes: a pos or a width that
    reached past it would leave the allocation."""
    from clonos_amd import _lib
    packed = rejection_scene()
    n = packed.n_wide
    assert all(x % 1024 > 1 for x in packed.n_val)  # (a length moved by one keeps its block count)
    packed.desc, packed.bits = packed.desc.copy(), packed.bits.copy()
    st = packed._struct()
    if name == "n_bits_past_cap_bits":
        st.n_bits = st.cap_bits  # (the poke adds to it)
    REJECTIONS[name](packed, st)
    # the host call's verdict over host arrays
    hc, arrs = _lib.Columns(), []
    for k, dt in zip(WIDE, WIDE_DT):
        arrs.append(np.full(n * np.dtype(dt).itemsize, FILL, np.uint8))
        setattr(hc, k, arrs[-1].ctypes.data)
    hc.cap_wide = n
    hbad = _lib.UnpackBad()
    hst = _lib.lib.clg_unpack_wide_host(C.byref(st), C.byref(hc), C.byref(hbad))
    assert hst == _lib.CLG_E_INVALID_ARG and hbad.what != 0 and all((a == FILL).all() for a in arrs)
    pin, out = WideIn(packed, "device", exact=True, st=st), WideOut("device", n)
    bad = _lib.UnpackBad()
    try:
        assert eng.unpack_wide_raw(pin.p, out.c, out.pos, bad) == hst
        assert (bad.what, bad.stream, bad.block) == (hbad.what, hbad.stream, hbad.block)
        assert out.untouched()
    finally:
        pin.free()
        out.free()


@pytest.mark.parametrize("kinds", [("host", "host"), ("mapped", "mapped"), ("host", "device")])
def test_a_rejection_writes_nothing_whatever_the_kinds(eng, kinds):
    from clonos_amd import _lib
    packed = rejection_scene()
    packed.desc = packed.desc.copy()
    packed.desc["first"][packed.blk_base[2 + 6 + 2]] = -1
    pin, out = WideIn(packed, kinds[0]), WideOut(kinds[1], packed.n_wide)
    bad = _lib.UnpackBad()
    try:
        assert eng.unpack_wide_raw(pin.p, out.c, out.pos, bad) == _lib.CLG_E_INVALID_ARG
        assert (bad.what, bad.stream, bad.block) == (_lib.UNPACK_BAD_VALUE, 2 + 6 + 2, 0) and out.untouched()
    finally:
        pin.free()
        out.free()


def test_errors_raise_with_what_stream_and_block(eng):
    from clonos_amd import ClonosError, _lib
    packed = rejection_scene()
    packed.desc = packed.desc.copy()
    packed.desc["width"][packed.blk_base[1] + 2] = 65
    with pytest.raises(ClonosError) as ei:
        eng.unpack_wide(packed, pos=True)
    assert (ei.value.status, ei.value.bad_what, ei.value.bad_stream, ei.value.bad_block) == (_lib.CLG_E_INVALID_ARG, 2, 1, 2)


def test_an_empty_input_launches_nothing(eng):
    from clonos_amd import pack_wide_host
    packed = pack_wide_host(seeded_wide(np.zeros(0, np.uint8), 1))
    eng.kernel_stats_reset()
    got = eng.unpack_wide(packed, pos=True)
    assert got["w_idx"].size == 0 and list(got["pos"]) == [0]
    assert eng.kernel_stats().get("unpack_wide", {}).get("launches", 0) == 0
    out = WideOut("device", 4)
    try:
        from clonos_amd import _lib
        assert eng.unpack_wide_raw(packed._struct(), out.c, out.pos, _lib.UnpackBad()) == _lib.CLG_OK
        raw = out.reg.get()
        assert not raw[out.at["pos"]:out.at["pos"] + 8].any()
        raw[out.at["pos"]:out.at["pos"] + 8] = FILL
        assert (raw == FILL).all()
    finally:
        out.free()
    assert eng.kernel_stats().get("unpack_wide", {}).get("launches", 0) == 0


def test_the_stat_is_recorded(eng):
    from clonos_amd import pack_wide_host
    packed = pack_wide_host(scene())
    eng.kernel_stats_reset()
    eng.unpack_wide(packed, pos=True)
    st = eng.kernel_stats()["unpack_wide"]
    assert st["launches"] >= 2 and st["bytes"] > 0 and st["ms"] > 0
