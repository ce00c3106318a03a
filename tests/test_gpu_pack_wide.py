"""GPU: clg_pack_wide.  Every comparison is byte for byte against pack_wide_host (which
tests/test_wpack_host.py holds against an independent numpy packer): the packed bytes are a pure
function of the rows, so there is no tolerance.  The shapes are the smallest that reach each seam:
a tile of the kind and split passes is 1024 rows, a wave 64, a workgroup's quarter 256."""
import ctypes as C
import mmap

import numpy as np
import pytest

from _wpack_util import WIDE, WIDE_DT, Wide, assert_round_trip, assert_same_wide, seeded_wide, width_scene, widths_of

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as e:
        yield e


def same_as_host(eng, cols):
    from clonos_amd import pack_wide_host
    want = pack_wide_host(cols)
    got = eng.pack_wide(cols)
    assert_same_wide(got, want)
    return got


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_row_counts_across_the_tile_seam(eng, n):
    kinds = np.random.default_rng(n).integers(0, 4, n)
    got = same_as_host(eng, seeded_wide(kinds, 100 + n, gap=2))
    assert got.n_val[0] == got.n_val[1] == n and sum(got.n_val[2::6]) == n
    assert_round_trip(got, seeded_wide(kinds, 100 + n, gap=2))


@pytest.mark.parametrize("count", [0, 1, 1024, 1025])
@pytest.mark.parametrize("kind", range(4))
def test_each_kinds_count_at_the_block_seam(eng, kind, count):
    """`count` rows of one kind spread among 700 of each other kind."""
    rng = np.random.default_rng(17 * kind + count)
    kinds = np.concatenate([np.full(count, kind), np.repeat([k for k in range(4) if k != kind], 700)])
    rng.shuffle(kinds)
    got = same_as_host(eng, seeded_wide(kinds, 7 + count))
    assert got.n_val[2 + 6 * kind] == count


@pytest.mark.parametrize("kind", range(4))
def test_rows_of_one_kind_only(eng, kind):
    got = same_as_host(eng, seeded_wide(np.full(1500, kind), 31 + kind))
    assert [got.n_val[2 + 6 * t] for t in range(4)] == [1500 if t == kind else 0 for t in range(4)]


@pytest.mark.parametrize("run", [1, 64, 65, 256])
def test_kinds_in_runs_across_the_wave_and_workgroup_seams(eng, run):
    """Kinds alternating every `run` rows: a row's rank inside its tile crosses lanes (1), waves
    (64, 65) and the workgroup's quarters (256)."""
    kinds = (np.arange(3 * 1024 + 77) // run) % 4
    same_as_host(eng, seeded_wide(kinds, 500 + run))


@pytest.mark.parametrize("width", range(65))
def test_width_scenes(eng, width):
    """A full block of every field of every kind at every width: 0..64 on the i64 fields, 0..32 on
    the 32-bit fields, 0..8 on SUB."""
    cols = width_scene(width)
    got = same_as_host(eng, cols)
    for t in range(4):
        assert widths_of(got, t) == [min(width, 32), width, min(width, 32), min(width, 32), min(width, 8), width]


@pytest.mark.parametrize("n", [1023, 1025])
def test_word_seams_with_a_short_last_block(eng, n):
    """Widths either side of the 32- and 64-bit seams in a block that is not full, and in one that
    is followed by a block of a single value."""
    for width in (31, 33, 63, 64):
        same_as_host(eng, width_scene(width, n=n))


def test_a_var_off_at_a_span_boundary_and_int64_extremes_side_by_side(eng):
    """Offsets that fall back to a small value where the next span begins (a negative DELTA residual
    beside positive ones) and stop at the last byte a u32 can name; INT64_MIN beside INT64_MAX in V0
    of every kind (FOR in kind 0, DELTA in the others)."""
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    n = 1350
    kinds = np.arange(n) % 4
    off = np.concatenate([np.arange(9, 9 + 13 * 450, 13), np.arange(1, 1 + 7 * 450, 7), 2 ** 32 - 1 - np.arange(450)[::-1]])
    v0 = np.resize(np.array([lo, hi, lo, 0, hi, hi, lo, -1, 1], np.int64), n)
    cols = Wide(kinds, w_var_off=off, w_v0=v0, w_v1=v0[::-1], w_var_len=np.resize([2 ** 32 - 1, 0, 5], n),
                w_rc=np.resize([-2 ** 31, 2 ** 31 - 1], n), w_sub=np.resize([255, 0, 1], n))
    got = same_as_host(eng, cols)
    assert_round_trip(got, cols)
    assert widths_of(got, 0)[5] == 64 and widths_of(got, 1)[5] == 64


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
    """clg_columns over the tags and the seven wide arrays of `cols` placed in one region of `kind`,
    GUARD bytes apart."""
    from clonos_amd import _lib
    arrs = [("tag", np.ascontiguousarray(cols.tag, np.uint8))]
    arrs += [(name, np.ascontiguousarray(getattr(cols, name), dt)) for name, dt in zip(WIDE, WIDE_DT)]
    at, total = {}, 0
    for name, a in arrs:
        at[name] = total
        total += (a.nbytes + 63 & ~63) + GUARD
    reg = Region(kind, max(total, 64))
    c = _lib.Columns()
    for name, a in arrs:
        reg.put(at[name], a)
        setattr(c, name, reg.ptr + at[name])
    c.n_rec = arrs[0][1].size
    c.n_class[4] = arrs[1][1].size
    c.out_kind = KIND[kind]
    return c, reg, at


def packed_out(kind, cap_desc, cap_bits):
    """clg_packed_wide whose arrays have GUARD bytes of FILL either side."""
    from clonos_amd import _lib
    o_bits = (2 * GUARD + cap_desc * 32 + 63) & ~63
    reg = Region(kind, o_bits + cap_bits + 2 * GUARD)
    p = _lib.PackedWideC()
    p.desc, p.cap_desc = reg.ptr + GUARD, cap_desc
    p.bits, p.cap_bits = reg.ptr + o_bits + GUARD, cap_bits
    p.out_kind = KIND[kind]
    return p, reg, o_bits


def scene():
    return seeded_wide(np.random.default_rng(21).integers(0, 4, 2500), 22, gap=3)


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("in_kind", ["host", "device", "mapped"])
def test_inputs_and_outputs_in_every_memory(eng, in_kind, out_kind):
    from clonos_amd import _lib, pack_wide_host
    cols = scene()
    want = pack_wide_host(cols)
    nb, nbits = want.desc.size, want.bits.size
    cin, rin, _ = columns_in(cols, in_kind)
    p, rout, o_bits = packed_out(out_kind, nb + 3, nbits + 48)
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == nbits
        assert p.bad_row == NONE
        raw = rout.get()
        assert raw[GUARD:GUARD + nb * 32].tobytes() == np.asarray(want.desc).tobytes()
        assert raw[o_bits + GUARD:o_bits + GUARD + nbits].tobytes() == np.asarray(want.bits).tobytes()
        raw[GUARD:GUARD + nb * 32] = FILL
        raw[o_bits + GUARD:o_bits + GUARD + nbits] = FILL
        assert (raw == FILL).all()  # nothing outside what was asked for, the spare capacity included
    finally:
        rin.free()
        rout.free()


@pytest.mark.parametrize("in_kind", ["device", "mapped"])
def test_a_misaligned_array_is_rejected(eng, in_kind):
    from clonos_amd import _lib
    cols = scene()
    cin, rin, _ = columns_in(cols, in_kind)
    p, rout, _ = packed_out("device", 64, 1 << 17)
    cin.w_v1 += 4
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_E_INVALID_ARG
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()


def test_unaligned_device_outputs_are_rejected(eng):
    from clonos_amd import _lib
    cin, rin, _ = columns_in(scene(), "host")
    p, rout, _ = packed_out("device", 64, 1 << 17)
    p.bits += 8
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_E_INVALID_ARG
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()


def test_sizes_only(eng):
    from clonos_amd import _lib, pack_wide_host
    cols = scene()
    want = pack_wide_host(cols)
    cin, rin, _ = columns_in(cols, "device")
    p = _lib.PackedWideC()
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size
        assert p.bad_row == NONE
    finally:
        rin.free()


@pytest.mark.parametrize("out_kind", ["host", "device", "mapped"])
@pytest.mark.parametrize("short", ["desc", "bits"])
def test_capacity_leaves_the_outputs_untouched(eng, short, out_kind):
    from clonos_amd import _lib, pack_wide_host
    cols = scene()
    want = pack_wide_host(cols)
    nb, nbits = want.desc.size, want.bits.size
    cin, rin, _ = columns_in(cols, "host")
    p, rout, _ = packed_out(out_kind, nb - (short == "desc"), nbits - (short == "bits"))
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_E_CAPACITY
        assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == nbits
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()


@pytest.mark.parametrize("in_kind", ["host", "device"])
def test_bad_rows_in_the_first_and_the_last_tile(eng, in_kind):
    """A w_idx == n_rec and a narrow tag, in the first tile and in the last: bad_row is the lowest,
    nothing is written, and the host packer reports the same row."""
    from clonos_amd import ClonosError, _lib, pack_wide_host
    cols = seeded_wide(np.arange(3 * 1024 + 5) % 4, 77)
    want = pack_wide_host(cols)
    cols.w_idx, cols.tag = cols.w_idx.copy(), cols.tag.copy()
    cols.w_idx[3 * 1024 + 2] = cols.tag.size     # the last tile: w_idx == n_rec
    cols.tag[cols.w_idx[3 * 1024 + 1]] = 2       # ... and a narrow tag
    cols.w_idx[900] = cols.tag.size              # the first tile
    cols.tag[cols.w_idx[333]] = 7
    with pytest.raises(ClonosError) as ei:
        pack_wide_host(cols)
    assert ei.value.bad_row == 333
    cin, rin, _ = columns_in(cols, in_kind)
    p, rout, _ = packed_out("device", want.desc.size + 4, want.bits.size + 64)
    try:
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_E_INVALID_ARG
        assert p.bad_row == 333 and p.n_bits == 0 and list(p.blk_base) == [0] * 27 and list(p.n_val) == [0] * 26
        assert (rout.get() == FILL).all()
    finally:
        rin.free()
        rout.free()
    with pytest.raises(ClonosError) as ei:
        eng.pack_wide(cols)
    assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_row == 333


def test_one_block_more_than_a_scan_group(eng):
    """Over 256 blocks in all: the second scan group's offsets carry the first group's sum."""
    kinds = np.random.default_rng(5).integers(0, 4, 36 * 1024 + 9)
    got = same_as_host(eng, seeded_wide(kinds, 9))
    assert got.blk_base[-1] > 256


def test_one_tile_more_than_a_round_of_the_kind_scan(eng):
    """1024 x 1024 + 1 rows: the kind counts' scan takes a second round, whose one tile gets the
    first round's totals as its bases.  The kinds cycle in runs of three, so every kind has rows in
    every tile of the first round; every field but w_var_len is constant, so the host's side stays
    in seconds."""
    n = 1024 * 1024 + 1
    got = same_as_host(eng, Wide((np.arange(n) // 3) % 4, gap=0, w_var_len=np.arange(n, dtype=np.uint64) % 1000))
    assert got.n_val[0] == n and all(got.n_val[2 + 6 * t] >= n // 4 - 3 for t in range(4))


def test_the_stat_is_recorded(eng):
    eng.kernel_stats_reset()
    eng.pack_wide(scene())
    st = eng.kernel_stats()
    assert st["pack_wide"]["launches"] >= 3 and st["pack_wide"]["bytes"] > 0 and st["pack_wide"]["ms"] > 0
