"""GPU: the one-launch pack (k_pack_small) against the multi-kernel forms and the CPU packers.

Two engines: one with the form on, one with it turned off by CLONOS_PACK_SMALL=0 (read when the
engine opens).  Every scene runs on both, into guarded outputs of exactly the CPU packer's sizes:
desc and bits are byte-equal to pack_columns_host / pack_wide_host (the packed bytes are a pure
function of the input, so there is no tolerance), the guards are intact, and the count-only stat
`pack_small` proves which path ran.  B = kPackSmallBlocks (pack.h), W = kWPackSmallRows
(pack_wide.h); a block and a tile of rows are 1024."""
import ctypes as C
import mmap
import os
import re

import numpy as np
import pytest

from _pack_util import Narrow, values_of_width
from _wpack_util import Wide, seeded_wide

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 64
NONE = 2 ** 64 - 1
KIND = {"host": 0, "device": 1, "mapped": 2}
BOTH = ("small", "multi")


def _constant(header, name):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", header)).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


B = _constant("pack.h", "kPackSmallBlocks")
W = _constant("pack_wide.h", "kWPackSmallRows")


@pytest.fixture(scope="module")
def engines():
    from clonos_amd import Engine
    small = Engine(segment_bytes=256, pool_segments=1 << 14, timing=True)
    old = os.environ.get("CLONOS_PACK_SMALL")
    os.environ["CLONOS_PACK_SMALL"] = "0"
    try:
        multi = Engine(segment_bytes=256, pool_segments=1 << 14, timing=True)
    finally:
        if old is None:
            del os.environ["CLONOS_PACK_SMALL"]
        else:
            os.environ["CLONOS_PACK_SMALL"] = old
    yield {"small": small, "multi": multi}
    small.close()
    multi.close()


def taken(eng):
    """Calls that took the one-launch pack so far."""
    return eng.kernel_stats().get("pack_small", {"launches": 0})["launches"]


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

    def get(self):
        return self.dev.host() if self.kind == "device" else np.array(self.mem[:self.n])

    def free(self):
        from clonos_amd import _lib
        if self.kind == "device":
            self.dev.free()
        elif self.kind == "mapped":
            _lib.check(_lib.lib.clg_host_unregister(self.mem.ctypes.data))


def guarded(struct, kind, cap_desc, cap_bits):
    """A clg_packed / clg_packed_wide whose arrays have GUARD bytes of FILL either side."""
    o_bits = (2 * GUARD + cap_desc * 32 + 63) & ~63
    reg = Region(kind, o_bits + cap_bits + 2 * GUARD)
    p = struct()
    p.desc, p.cap_desc = reg.ptr + GUARD, cap_desc
    p.bits, p.cap_bits = reg.ptr + o_bits + GUARD, cap_bits
    p.out_kind = KIND[kind]
    return p, reg, o_bits


def assert_written_exactly(p, reg, o_bits, want):
    nb, nbits = want.desc.size, want.bits.size
    assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == nbits
    raw = reg.get()
    assert raw[GUARD:GUARD + nb * 32].tobytes() == np.asarray(want.desc).tobytes()
    assert raw[o_bits + GUARD:o_bits + GUARD + nbits].tobytes() == np.asarray(want.bits).tobytes()
    raw[GUARD:GUARD + nb * 32] = FILL
    raw[o_bits + GUARD:o_bits + GUARD + nbits] = FILL
    assert (raw == FILL).all()  # the guards, and nothing else either


def check_narrow(engines, cols, small=True, kind="host"):
    """clg_pack_columns of host columns on both engines; small: the form must have been taken."""
    from clonos_amd import _lib, pack_columns_host
    from clonos_amd.engine import _pack_in
    want = pack_columns_host(cols)
    cin, keep = _pack_in(cols)
    for which in BOTH:
        eng = engines[which]
        before = taken(eng)
        p, reg, o_bits = guarded(_lib.Packed, kind, want.desc.size, want.bits.size)
        try:
            assert eng.pack_columns_raw(cin, p) == _lib.CLG_OK, which
            assert taken(eng) - before == (1 if which == "small" and small else 0), which
            assert_written_exactly(p, reg, o_bits, want)
        finally:
            reg.free()
    del keep
    return want


def check_wide(engines, cols, small=True, kind="host"):
    from clonos_amd import _lib, pack_wide_host
    from clonos_amd.engine import _pack_wide_in
    want = pack_wide_host(cols)
    cin, keep = _pack_wide_in(cols)
    for which in BOTH:
        eng = engines[which]
        before = taken(eng)
        p, reg, o_bits = guarded(_lib.PackedWideC, kind, want.desc.size, want.bits.size)
        try:
            assert eng.pack_wide_raw(cin, p) == _lib.CLG_OK, which
            assert taken(eng) - before == (1 if which == "small" and small else 0), which
            assert p.bad_row == NONE
            assert_written_exactly(p, reg, o_bits, want)
        finally:
            reg.free()
    del keep
    return want


def narrow_of(lens, seed, widths=(3, 2, 3, 31, 13)):
    rng = np.random.default_rng(seed)
    mk = lambda dt, w, k, **kw: values_of_width(rng, dt, w if k >= 3 else 0, k, **kw) if k else np.zeros(0, dt)
    return Narrow(tag=mk(np.uint8, widths[0], lens[0], vmin=0, vmax=7), order=mk(np.int8, widths[1], lens[1]),
                  timestamp=mk(np.int64, widths[2], lens[2], delta=True), rng=mk(np.int32, widths[3], lens[3]),
                  buffer_built=mk(np.int32, widths[4], lens[4]))


# ---- the narrow half ----------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[0, 0, 0, 0, 0], [1, 0, 2, 0, 1], [1023, 0, 1024, 0, 1025], [2049, 1, 0, 2, 1023],
                                  [0, 2049, 1025, 1024, 0]])
def test_stream_lengths_with_empty_streams_between(engines, lens):
    want = check_narrow(engines, narrow_of(lens, sum(lens) + 1))
    assert want.n_val == lens


@pytest.mark.parametrize("width", [0, 1, 2, 31, 63, 64])
def test_widths(engines, width):
    """Every stream at `width` (capped by its element): 1 is the ballot path of the FOR streams, 64
    the word-a-value path; a short last block behind a full one."""
    rng = np.random.default_rng(700 + width)
    n = 1024 + 77
    cols = Narrow(tag=values_of_width(rng, np.uint8, min(width, 3), n, vmin=0, vmax=7),
                  order=values_of_width(rng, np.int8, min(width, 8), n),
                  timestamp=values_of_width(rng, np.int64, width, n, delta=True),
                  rng=values_of_width(rng, np.int32, min(width, 32), n),
                  buffer_built=values_of_width(rng, np.int32, min(width, 32), n))
    want = check_narrow(engines, cols)
    d = np.asarray(want.desc)
    assert int(d["width"][want.blk_base[2]]) == width and int(d["width"][want.blk_base[3]]) == min(width, 32)


def test_the_delta_wraps(engines):
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    check_narrow(engines, Narrow(timestamp=np.array([lo, hi, lo, 0, hi, hi, lo, -1, 1] * 150, np.int64)))


@pytest.mark.parametrize("blocks", [1, 63, 64, 65, B, B + 1])
def test_total_blocks_at_the_scan_round_and_at_the_limit(engines, blocks):
    """`blocks` blocks in all, the last one short, over three streams; B + 1 takes the multi-kernel form."""
    rest = blocks - 1
    lens = [rest // 2 * 1024, 0, (rest - rest // 2) * 1024, 0, 5]
    want = check_narrow(engines, narrow_of(lens, blocks), small=blocks <= B)
    assert want.blk_base[-1] == blocks


@pytest.mark.parametrize("kind", ["device", "mapped"])
def test_narrow_outputs_in_place(engines, kind):
    check_narrow(engines, narrow_of([3000, 900, 1100, 5, 1024], 9), kind=kind)


def test_narrow_capacity_and_sizes_only(engines):
    from clonos_amd import _lib, pack_columns_host
    from clonos_amd.engine import _pack_in
    cols = narrow_of([3000, 900, 1100, 5, 1024], 10)
    want = pack_columns_host(cols)
    cin, keep = _pack_in(cols)
    for which in BOTH:
        eng = engines[which]
        for short in ("desc", "bits"):
            for kind in ("host", "device"):
                p, reg, _ = guarded(_lib.Packed, kind, want.desc.size - (short == "desc"), want.bits.size - (short == "bits"))
                try:
                    assert eng.pack_columns_raw(cin, p) == _lib.CLG_E_CAPACITY, (which, short, kind)
                    assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size
                    assert (reg.get() == FILL).all()
                finally:
                    reg.free()
        p = _lib.Packed()
        assert eng.pack_columns_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and p.n_bits == want.bits.size


# ---- the wide half ------------------------------------------------------------------------------
def test_no_rows_launch_nothing(engines):
    check_wide(engines, seeded_wide(np.zeros(0, np.uint8), 1), small=False)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, W, W + 1])
def test_row_counts_across_the_tile_seam_and_at_the_limit(engines, n):
    kinds = np.random.default_rng(n).integers(0, 4, n)
    want = check_wide(engines, seeded_wide(kinds, 100 + n, gap=2), small=n <= W)
    assert want.n_val[0] == want.n_val[1] == n and sum(want.n_val[2::6]) == n


@pytest.mark.parametrize("kind", range(4))
def test_each_kind_alone_and_absent(engines, kind):
    check_wide(engines, seeded_wide(np.full(1500, kind), 31 + kind))
    others = np.repeat([k for k in range(4) if k != kind], 400)
    np.random.default_rng(kind).shuffle(others)
    want = check_wide(engines, seeded_wide(others, 41 + kind))
    assert want.n_val[2 + 6 * kind] == 0


def test_a_kind_of_exactly_one_block(engines):
    kinds = np.concatenate([np.full(1024, 2), np.repeat([0, 1, 3], 333)])
    np.random.default_rng(5).shuffle(kinds)
    want = check_wide(engines, seeded_wide(kinds, 6))
    assert want.n_val[2 + 6 * 2] == 1024


@pytest.mark.parametrize("run", [1, 64, 65, 256])
def test_kinds_in_runs_across_the_wave_and_quarter_seams(engines, run):
    check_wide(engines, seeded_wide((np.arange(2 * 1024 + 77) // run) % 4, 500 + run))


def test_var_off_residuals_of_33_bits(engines):
    """VAR_OFF = 0, 0xFFFFFFFF, 0, ...: the DELTA of a zero-extended u32 is wider than its element."""
    n = 1300
    off = np.resize(np.array([0, 2 ** 32 - 1], np.uint64), n)
    want = check_wide(engines, Wide(np.zeros(n, np.uint8), w_var_off=off, w_var_len=np.resize([2 ** 32 - 1, 0, 5], n)))
    assert int(np.asarray(want.desc)["width"][want.blk_base[2 + 2]]) == 33


@pytest.mark.parametrize("kind", ["device", "mapped"])
def test_wide_outputs_in_place(engines, kind):
    check_wide(engines, seeded_wide(np.random.default_rng(21).integers(0, 4, 2500), 22, gap=3), kind=kind)


@pytest.mark.parametrize("row", [0, 1023, 1024, 2 * 1024 + 4])
@pytest.mark.parametrize("how", ["w_idx", "tag"])
def test_a_bad_row_writes_nothing(engines, row, how):
    """A w_idx == n_rec or a narrow tag at the first row, either side of the tile seam and the last
    row, with a later bad row behind it: bad_row is the lowest, nothing is written."""
    from clonos_amd import _lib
    from clonos_amd.engine import _pack_wide_in
    n = 2 * 1024 + 5
    cols = seeded_wide(np.arange(n) % 4, 77)
    cols.w_idx, cols.tag = cols.w_idx.copy(), cols.tag.copy()
    for r in {row, n - 1}:
        if how == "w_idx":
            cols.w_idx[r] = cols.tag.size
        else:
            cols.tag[cols.w_idx[r]] = 2
    cin, keep = _pack_wide_in(cols)
    for which in BOTH:
        for kind in ("device", "host"):
            before = taken(engines[which])
            p, reg, _ = guarded(_lib.PackedWideC, kind, 128, 1 << 17)
            try:
                assert engines[which].pack_wide_raw(cin, p) == _lib.CLG_E_INVALID_ARG, (which, kind)
                assert taken(engines[which]) - before == (1 if which == "small" else 0), (which, kind)  # k_pack_small's verdict
                assert p.bad_row == row and p.n_bits == 0 and list(p.blk_base) == [0] * 27 and list(p.n_val) == [0] * 26
                assert (reg.get() == FILL).all()
            finally:
                reg.free()
    del keep


def test_wide_capacity_and_sizes_only(engines):
    from clonos_amd import _lib, pack_wide_host
    from clonos_amd.engine import _pack_wide_in
    cols = seeded_wide(np.random.default_rng(3).integers(0, 4, 2500), 4)
    want = pack_wide_host(cols)
    cin, keep = _pack_wide_in(cols)
    for which in BOTH:
        eng = engines[which]
        for short in ("desc", "bits"):
            for kind in ("host", "device"):
                p, reg, _ = guarded(_lib.PackedWideC, kind, want.desc.size - (short == "desc"), want.bits.size - (short == "bits"))
                try:
                    assert eng.pack_wide_raw(cin, p) == _lib.CLG_E_CAPACITY, (which, short, kind)
                    assert list(p.n_val) == want.n_val and list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size
                    assert (reg.get() == FILL).all()
                finally:
                    reg.free()
        p = _lib.PackedWideC()
        assert eng.pack_wide_raw(cin, p) == _lib.CLG_OK
        assert list(p.n_val) == want.n_val and p.n_bits == want.bits.size and p.bad_row == NONE


# ---- both halves, through the packed-wide decode -----------------------------------------------------
@pytest.fixture(scope="module")
def decoded(engines):
    """Spans with wide rows of every kind and payloads, and what the multi-kernel engine delivers."""
    from clonos_amd import synth
    rng = np.random.default_rng(0xDEC0DE)
    spans = [b"", bytes(synth.config3_epoch(1200, rng)[0]), synth.random_log(600, rng, allow_serializable=True), b"",
             bytes(synth.config2_log(2500, rng)[0])]
    data = np.frombuffer(b"".join(spans), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])])
    at = [(int(o), len(s)) for o, s in zip(offs, spans)]
    want = engines["multi"].decode_host_columns(data, at, packed=True, pack_wide=True, payloads=True)
    return data, at, want


def raw_decode(eng, data, at, sizes, var, pk, wpk):
    from clonos_amd import _lib
    so = np.array([s[0] for s in at], np.uint64)
    sl = np.array([s[1] for s in at], np.uint64)
    return _lib.lib.clg_decode_host_columns_packed_wide(eng._h, data.ctypes.data, so.ctypes.data, sl.ctypes.data, len(at),
                                                        C.byref(sizes), C.byref(var) if var is not None else None,
                                                        C.byref(pk), C.byref(wpk))


def test_both_halves_in_one_launch(engines, decoded):
    from clonos_amd import pack_columns_host, pack_wide_host
    from _pack_util import assert_same_packed
    from _wpack_util import assert_same_wide
    data, at, want = decoded
    eng = engines["small"]
    before = taken(eng)
    got = eng.decode_host_columns(data, at, packed=True, pack_wide=True, payloads=True)
    assert taken(eng) - before == 1
    assert got.wide_packed.n_wide > 0 and got.var.size > 0
    plain = eng.decode_host_columns(data, at, payloads=True)
    assert_same_packed(got, want)
    assert_same_packed(got, pack_columns_host(plain))
    assert_same_wide(got.wide_packed, want.wide_packed)
    assert_same_wide(got.wide_packed, pack_wide_host(plain))
    assert got.var.tobytes() == want.var.tobytes() == plain.var.tobytes()


@pytest.mark.parametrize("short", ["desc", "bits", "wdesc", "wbits", "var", "none", "sizes"])
@pytest.mark.parametrize("kind", ["host", "device", "mapped"])
def test_capacities_short_by_one_and_every_memory(engines, decoded, short, kind):
    """Each capacity one unit short while the others are exact: CLG_E_CAPACITY, every size filled,
    the fill pattern intact everywhere.  none: exact capacities, written exactly.  sizes: all NULL."""
    from clonos_amd import _lib
    from clonos_amd.engine import _payloads_struct
    data, at, want = decoded
    wp = want.wide_packed
    nb, nbits, wnb, wnbits, nvar = want.desc.size, want.bits.size, wp.desc.size, wp.bits.size, want.var.size
    assert min(nb, nbits, wnb, wnbits, nvar) > 0
    for which in BOTH:
        eng = engines[which]
        before = taken(eng)
        sizes = _lib.Columns()
        if short == "sizes":
            pk, wpk, pv = _lib.Packed(), _lib.PackedWideC(), _lib.Payloads()
            assert raw_decode(eng, data, at, sizes, pv, pk, wpk) == _lib.CLG_OK
            regs = []
        else:
            pk, r1, o1 = guarded(_lib.Packed, kind, nb - (short == "desc"), nbits - (short == "bits"))
            wpk, r2, o2 = guarded(_lib.PackedWideC, kind, wnb - (short == "wdesc"), wnbits - (short == "wbits"))
            regs = [r1, r2]
            var = np.full(nvar - (short == "var"), FILL, np.uint8)
            pv = _payloads_struct(var, None)
            try:
                st = raw_decode(eng, data, at, sizes, pv, pk, wpk)
                if short == "none":
                    assert st == _lib.CLG_OK, which
                    assert_written_exactly(pk, r1, o1, want)
                    assert_written_exactly(wpk, r2, o2, wp)
                    assert var.tobytes() == want.var.tobytes()
                else:
                    assert st == _lib.CLG_E_CAPACITY, (which, short)
                    assert (r1.get() == FILL).all() and (r2.get() == FILL).all() and (var == FILL).all()
            finally:
                for r in regs:
                    r.free()
        assert taken(eng) - before == (1 if which == "small" else 0), which
        assert sizes.n_rec == want.n_rec and sizes.n_class[4] == wp.n_wide
        assert list(pk.n_val) == want.n_val and list(pk.blk_base) == want.blk_base and pk.n_bits == nbits
        assert list(wpk.n_val) == wp.n_val and list(wpk.blk_base) == wp.blk_base and wpk.n_bits == wnbits
        assert pv.n_rows == wp.n_wide and pv.n_var == nvar
