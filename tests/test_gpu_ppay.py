"""GPU: clg_pack_payloads and clg_unpack_payloads.  Every comparison is byte for byte against the
CPU codec (pack_payloads_host / unpack_payloads_host, which tests/test_ppay_host.py holds against an
independent numpy packer): the packed bytes are a pure function of the column, so there is no
tolerance.  Inputs and outputs lie in device, registered and plain host memory with guard bytes
either side of every output.  The shapes are the smallest that reach each seam: a tile is 1024
rows, a row of 64 bytes or more goes to a wave, the scan takes 1024 tiles a round.  No input here
can make a kernel fault: the bad ones are those the checks reject before any dependent access."""
import ctypes as C

import numpy as np
import pytest

import _ppay_util as U

pytestmark = pytest.mark.gpu

KINDS = ("device", "mapped", "host")


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as e:
        yield e


def host_packed(var, pos):
    from clonos_amd import pack_payloads_host
    return pack_payloads_host(var, pos)


class PackCall:
    """clg_pack_payloads of (var, pos) in `kind` memory into guarded outputs of the same kind, with
    the capacities given (default: the CPU codec's sizes exactly)."""

    def __init__(self, eng, var, pos, kind, caps=None, sizes_only=False, n_rows=None):
        from clonos_amd import _lib
        var, pos = np.ascontiguousarray(var, np.uint8), np.ascontiguousarray(pos, np.uint64)
        self.n = pos.size - 1 if n_rows is None else n_rows
        self.src = U.Guarded(kind, {"var": var.size, "pos": pos.nbytes})
        self.src.put("var", var)
        self.src.put("pos", pos)
        self.caps = caps
        self.p = _lib.PackedPayloadsC()
        self.p.out_kind = self.src.mem_kind
        self.dst = None
        if not sizes_only:
            cd, cb, ct = caps
            self.dst = U.Guarded(kind, {"desc": cd * 32, "bits": cb, "tail": ct})
            self.p.desc, self.p.bits, self.p.tail = self.dst.ptr("desc"), self.dst.ptr("bits"), self.dst.ptr("tail")
            self.p.cap_desc, self.p.cap_bits, self.p.cap_tail = cd, cb, ct
        self.st = eng.pack_payloads_raw(self.src.ptr("var"), self.src.ptr("pos"), self.n, self.src.mem_kind, self.p)

    def results(self):
        return int(self.p.n_rows), int(self.p.n_var), int(self.p.n_bits), int(self.p.n_tail), int(self.p.bad_row)

    def free(self):
        self.src.free()
        if self.dst:
            self.dst.free()


def sizes_of(want):
    return want.desc.size, want.bits.size, want.tail.size


def unpack_call(eng, src, p_in, pos_ptr, pos_kind, kind, cap_var, sizes_only=False, claim=None):
    """clg_unpack_payloads of the packed struct p_in into a guarded var of `kind` memory (claim: the
    capacity stated, where it is not the buffer's)."""
    from clonos_amd import _lib
    out = _lib.Payloads()
    dst = U.Guarded(kind, {"var": cap_var})
    out.out_kind = dst.mem_kind
    if not sizes_only:
        out.var, out.cap_var = dst.ptr("var"), cap_var if claim is None else claim
    bad = _lib.UnpackBad()
    st = eng.unpack_payloads_raw(p_in, pos_ptr, pos_kind, out, bad)
    return st, out, (int(bad.what), int(bad.stream), int(bad.block)), dst


def round_trip(eng, var, pos, kind="device"):
    """The device pack gives the CPU codec's bytes inside intact guards; the device unpack of those
    bytes, where the pack left them, gives the column back inside intact guards."""
    from clonos_amd import _lib
    var, pos = np.ascontiguousarray(var, np.uint8), np.ascontiguousarray(pos, np.uint64)
    want = host_packed(var, pos)
    c = PackCall(eng, var, pos, kind, caps=sizes_of(want))
    try:
        assert c.st == _lib.CLG_OK, _lib.lib.clg_last_error()
        assert c.results() == (pos.size - 1, var.size, want.bits.size, want.tail.size, U.NO_ROW)
        for name, arr in (("desc", want.desc), ("bits", want.bits), ("tail", want.tail)):
            assert c.dst.get(name, arr.nbytes).tobytes() == arr.tobytes(), name
            assert c.dst.intact_outside(name, arr.nbytes), name
        if pos.size > 1:
            p_in = c.p
            st, out, bad, dst = unpack_call(eng, c.src, p_in, c.src.ptr("pos"), c.src.mem_kind, kind, var.size)
            try:
                assert st == _lib.CLG_OK and bad == (_lib.UNPACK_BAD_NONE, 0, U.NO_ROW), (_lib.lib.clg_last_error(), bad)
                assert (int(out.n_rows), int(out.n_var)) == (pos.size - 1, var.size)
                assert dst.get("var", var.size).tobytes() == var.tobytes()
                assert dst.intact_outside("var", var.size)
            finally:
                dst.free()
    finally:
        c.free()
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_row_counts_across_the_tile_seams(eng, n, kind):
    rng = np.random.default_rng(100 + n)
    var, pos = U.column(U.seeded_rows(rng, n, [0, 1, 2, 15, 16, 17, 40, 63, 64, 65, 150]))
    round_trip(eng, var, pos, kind)


@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, 5000])
def test_row_lengths_either_side_of_the_wave_row(eng, L):
    """Every row has the one length L (one length for a whole tile, too), with lcps of every size;
    5000: rows of a few KiB, whose wave compares 1024 bytes a round."""
    rng = np.random.default_rng(L)
    n = 1500 if L < 5000 else 40
    base = rng.integers(0, 256, L, dtype=np.uint8)
    rows = []
    for k in range(n):
        r = base.copy()
        cut = [0, 1, L // 2, max(L - 1, 0), L, 1023, 1024, 1025][k % 8] if k else L
        if cut < L:
            r[cut:] = rng.integers(0, 256, L - cut, dtype=np.uint8)
            r[cut] = base[cut] ^ 0x40
        rows.append(r.tobytes())
    want = round_trip(eng, *U.column(rows))
    assert want.tail.size <= max(L, 1) * n


@pytest.mark.parametrize("L", [33, 80])
def test_first_difference_at_every_byte_and_alignment(eng, L):
    """The first difference at every byte 0 .. 16 and none at all (lcp == len), the row at every
    16-byte alignment and the anchor at every 16-byte alignment; 33: a lane compares, 80: a wave."""
    rng = np.random.default_rng(L)
    base = rng.integers(0, 256, L, dtype=np.uint8)
    for a in range(16):
        rows, at = [bytes(a), base.tobytes()], a + L
        for b in range(16):
            for d in range(18):
                pad = (b - at) % 16
                r = base.copy()
                if d < 17:
                    r[d] ^= 1 + (b + d) % 255
                rows += [bytes(pad), r.tobytes()]
                at += pad + L
        var, pos = U.column(rows)
        assert len(rows) <= 1024 and {int(pos[2 * i + 1]) % 16 for i in range(1, 289)} == set(range(16))
        round_trip(eng, var, pos)


def test_1024_distinct_lengths_fill_the_table_and_collide(eng):
    """Tile 0: 1024 distinct lengths, those that share slots of the device's table first, every row
    its own anchor.  Tile 1: half of those lengths twice, in another order, each row's second copy
    sharing a prefix with its first."""
    rng = np.random.default_rng(0x7AB)
    lens = U.colliding_lengths()
    rows = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
    half = [rows[i] for i in rng.permutation(1024)[:512]]
    second = []
    for r in half:
        s = np.frombuffer(r, np.uint8).copy()
        if s.size:
            s[int(rng.integers(0, s.size)):] ^= 0x11
        second.append(s.tobytes())
    tile1 = half + second
    tile1 = [tile1[i] for i in rng.permutation(1024)]
    var, pos = U.column(rows + tile1)
    assert var.size < 5 << 20
    want = round_trip(eng, var, pos)
    lcp = U.decode_lcps(want.desc, want.bits)
    assert not lcp[:1024].any() and lcp[1024:].any()


def test_zero_length_rows_between_others(eng):
    rng = np.random.default_rng(9)
    rows = []
    for k in range(2500):
        rows.append(b"" if k % 3 else rng.integers(0, 3, int(rng.choice([5, 70])), dtype=np.uint8).tobytes())
    round_trip(eng, *U.column(rows), kind="device")
    round_trip(eng, *U.column([b""] * 1500), kind="host")


def test_one_byte_rows_reach_the_scans_second_round(eng):
    """1024 tiles and a few rows more: the carry of tile_scan's second round, in the tail bases and
    in the blocks' payload offsets."""
    rng = np.random.default_rng(0x5CA)
    n = 1024 * 1024 + 5
    var = rng.integers(0, 2, n, dtype=np.uint8)
    pos = np.arange(n + 1, dtype=np.uint64)
    want = round_trip(eng, var, pos)
    assert want.desc.size == 1025 and int(want.desc["pos"][1024]) > 0 and want.tail.size > 0


@pytest.mark.parametrize("kind", KINDS)
def test_sizes_only_and_each_capacity_one_below_its_total(eng, kind):
    from clonos_amd import _lib
    var, pos = U.random_log_column()
    want = host_packed(var, pos)
    n = pos.size - 1
    filled = (n, var.size, want.bits.size, want.tail.size, U.NO_ROW)
    c = PackCall(eng, var, pos, kind, sizes_only=True)
    assert c.st == _lib.CLG_OK and c.results() == filled
    c.free()
    for which in range(3):
        caps = [s - (i == which) for i, s in enumerate(sizes_of(want))]
        c = PackCall(eng, var, pos, kind, caps=caps)
        assert c.st == _lib.CLG_E_CAPACITY and c.results() == filled and c.dst.untouched()
        c.free()
    # the unpack: sizes only, and var one byte short
    c = PackCall(eng, var, pos, kind, caps=sizes_of(want))
    assert c.st == _lib.CLG_OK
    st, out, bad, dst = unpack_call(eng, c.src, c.p, c.src.ptr("pos"), c.src.mem_kind, kind, var.size, sizes_only=True)
    assert st == _lib.CLG_OK and (int(out.n_rows), int(out.n_var)) == (n, var.size) and dst.untouched()
    dst.free()
    st, out, bad, dst = unpack_call(eng, c.src, c.p, c.src.ptr("pos"), c.src.mem_kind, kind, var.size - 1)
    assert st == _lib.CLG_E_CAPACITY and (int(out.n_rows), int(out.n_var)) == (n, var.size) and dst.untouched()
    assert bad[0] == _lib.UNPACK_BAD_NONE
    dst.free()
    c.free()


@pytest.mark.parametrize("kind", KINDS)
def test_each_rejection_of_the_pack(eng, kind):
    """pos[0] != 0, a decreasing pos and a row of 2^32 bytes: the lowest bad row, nothing written.
    The long row lies in the last tile, whose bytes are then never read."""
    from clonos_amd import _lib
    rng = np.random.default_rng(0xBAD)
    var, pos = U.column(U.seeded_rows(rng, 2300, [3, 20, 70]))
    want = host_packed(var, pos)
    big = [s + 64 for s in sizes_of(want)]
    scenes = []
    q = pos.copy()
    q[0] = 1
    scenes.append((q, 0))
    q = pos.copy()
    q[1100] = q[1099] - 1   # row 1099 decreases
    q[2200] = q[2199] - 1   # ... and row 2199, in another tile
    scenes.append((q, 1099))
    q = pos.copy()
    q[2100:] += np.uint64(1 << 32)  # row 2099 holds 2^32 bytes and more; the rows behind it are in its tile
    scenes.append((q, 2099))
    q = pos.copy()
    q[0], q[5] = 7, q[4] - 1
    scenes.append((q, 0))
    for q, row in scenes:
        c = PackCall(eng, var, q, kind, caps=big)
        assert c.st == _lib.CLG_E_INVALID_ARG and int(c.p.bad_row) == row and c.dst.untouched(), row
        c.free()
    # misaligned arrays in device and registered memory; unknown kinds
    if kind != "host":
        for name, by in (("bits", 8), ("desc", 4)):
            c = PackCall(eng, var, pos, kind, sizes_only=True)
            g = U.Guarded(kind, {"desc": big[0] * 32 + 16, "bits": big[1] + 16, "tail": big[2]})
            c.p.desc, c.p.bits, c.p.tail = g.ptr("desc"), g.ptr("bits"), g.ptr("tail")
            c.p.cap_desc, c.p.cap_bits, c.p.cap_tail = big
            setattr(c.p, name, g.ptr(name) + by)
            assert eng.pack_payloads_raw(c.src.ptr("var"), c.src.ptr("pos"), c.n, c.src.mem_kind, c.p) == _lib.CLG_E_INVALID_ARG
            assert g.untouched()
            g.free()
            c.free()
        c = PackCall(eng, var, pos, kind, sizes_only=True)
        assert eng.pack_payloads_raw(c.src.ptr("var"), c.src.ptr("pos") + 4, c.n, c.src.mem_kind, c.p) == _lib.CLG_E_INVALID_ARG
        c.free()
    c = PackCall(eng, var, pos, kind, sizes_only=True)
    assert eng.pack_payloads_raw(c.src.ptr("var"), c.src.ptr("pos"), c.n, 3, c.p) == _lib.CLG_E_INVALID_ARG
    c.p.out_kind = 7
    assert eng.pack_payloads_raw(c.src.ptr("var"), c.src.ptr("pos"), c.n, c.src.mem_kind, c.p) == _lib.CLG_E_INVALID_ARG
    c.free()


class PackedIn:
    """A packed column's three arrays and its pos in `kind` memory, as the unpack's input."""

    def __init__(self, kind, desc, bits, tail, pos, n_rows, n_var):
        from clonos_amd import _lib
        self.g = U.Guarded(kind, {"desc": desc.nbytes, "bits": bits.size, "tail": tail.size, "pos": pos.nbytes})
        for name, a in (("desc", desc), ("bits", bits), ("tail", tail), ("pos", pos)):
            self.g.put(name, a)
        self.p = _lib.PackedPayloadsC()
        self.p.desc, self.p.bits, self.p.tail = self.g.ptr("desc"), self.g.ptr("bits"), self.g.ptr("tail")
        self.p.cap_desc, self.p.cap_bits, self.p.cap_tail = desc.size, bits.size, tail.size
        self.p.out_kind = self.g.mem_kind
        self.p.n_rows, self.p.n_var, self.p.n_bits, self.p.n_tail = n_rows, n_var, bits.size, tail.size


def finding_like_the_host(eng, kind, desc, bits, tail, pos, n_var, mutate=None):
    """The device's (status, finding) of a packed input and the CPU codec's; nothing is written.
    cap_var is n_var as claimed; the buffer behind it holds at most 16 MiB, which a finding never
    reaches."""
    from clonos_amd import _lib
    n = pos.size - 1
    src = PackedIn(kind, desc, bits, tail, pos, n, n_var)
    if mutate:
        mutate(src.p)
    held = min(int(n_var), 1 << 24)
    st, out, bad, dst = unpack_call(eng, src.g, src.p, src.g.ptr("pos"), src.g.mem_kind, kind, held, claim=int(n_var))
    assert dst.untouched()
    dst.free()
    # the same on the CPU, over host copies
    hp = _lib.PackedPayloadsC()
    keep = [np.ascontiguousarray(desc), np.ascontiguousarray(bits), np.ascontiguousarray(tail), np.ascontiguousarray(pos)]
    hp.desc, hp.bits, hp.tail = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
    for f in ("cap_desc", "cap_bits", "cap_tail", "n_rows", "n_var", "n_bits", "n_tail"):
        setattr(hp, f, getattr(src.p, f))
    if not src.p.tail:
        hp.tail = None
    buf = np.full(held + 1, 0xA5, np.uint8)
    hout = _lib.Payloads()
    hout.var, hout.cap_var = buf.ctypes.data, int(n_var)
    hbad = _lib.UnpackBad()
    hst = _lib.lib.clg_unpack_payloads_host(C.byref(hp), keep[3].ctypes.data, C.byref(hout), C.byref(hbad))
    assert (buf == 0xA5).all()
    src.g.free()
    assert (st, bad) == (hst, (int(hbad.what), int(hbad.stream), int(hbad.block)))
    assert st == _lib.CLG_E_INVALID_ARG and bad[1] == _lib.PPAY_STREAM
    return bad[0], bad[2]


@pytest.mark.parametrize("kind", ["device", "host"])
def test_one_scene_per_finding_of_the_unpack(eng, kind):
    from clonos_amd import _lib
    L, B, V, T = _lib.UNPACK_BAD_LAYOUT, _lib.UNPACK_BAD_BLOCK, _lib.UNPACK_BAD_VALUE, _lib.UNPACK_BAD_TOTAL
    rng = np.random.default_rng(0xF1D)
    var, pos = U.column(U.seeded_rows(rng, 3100, [4, 9, 70, 130], alphabet=2))
    w = host_packed(var, pos)
    assert w.desc.size == 4 and (w.desc["width"] > 0).all()
    call = lambda desc=w.desc, bits=w.bits, tail=w.tail, q=pos, n_var=var.size, mutate=None: finding_like_the_host(  # noqa: E731
        eng, kind, desc, bits, tail, q, n_var, mutate)

    def with_desc(**kw):
        d = w.desc.copy()
        for f, (blk, val) in kw.items():
            d[f][blk] = val
        return d

    # LAYOUT: a capacity below its total, a block fewer than the rows need, a null array
    def short_desc(p):
        p.cap_desc -= 1

    def short_tail(p):
        p.cap_tail -= 1

    def null_tail(p):
        p.tail = None

    for m in (short_desc, short_tail, null_tail):
        assert call(mutate=m) == (L, 0)
    # BLOCK: the lowest, and before a value finding in a lower tile
    assert call(desc=with_desc(width=(2, 65))) == (B, 2)
    d = with_desc(count=(3, 1024), ref=(0, 1))
    d["pos"][1] += 8
    assert call(desc=d) == (B, 1)
    assert call(desc=with_desc(pos=(3, w.bits.size))) == (B, 3)
    # VALUE: an lcp above its row's length; a non-zero lcp on a row that is its own anchor
    assert call(desc=with_desc(ref=(2, 131))) == (V, 2)
    d = with_desc(ref=(1, 1))
    d["ref"][3] = 1
    assert call(desc=d) == (V, 1)
    # VALUE: the pos rules
    q = pos.copy()
    q[0] = 1
    assert call(q=q) == (V, 0)
    q = pos.copy()
    q[2100] = q[2101] + 1
    assert call(q=q) == (V, 2)
    if kind == "device":  # (in place: a host output's staging would be sized by the capacity claimed)
        q = pos.copy()
        q[3099:] += np.uint64(1 << 32)
        assert call(q=q, n_var=int(q[-1])) == (V, 3)
    # TOTAL: the tails' sum, and pos's end
    assert call(tail=np.concatenate([w.tail, [0]]).astype(np.uint8)) == (T, 0)
    assert call(tail=w.tail[:-1]) == (T, 0)
    assert call(n_var=var.size + 1) == (T, 0)


def test_a_non_maximal_lcp_unpacks_to_the_column(eng):
    """Every lcp above 1 lowered by one: more tail bytes, the same column."""
    from clonos_amd import PackedPayloads, _lib
    rng = np.random.default_rng(0x10)
    var, pos = U.column(U.seeded_rows(rng, 2500, [6, 40, 90], alphabet=2))
    lcp, _ = U.lcps_of(var, pos)
    lower = np.where(lcp > 1, lcp - 1, lcp)
    desc, bits, tail = U.pack_numpy(var, pos, lower)
    assert tail.size > host_packed(var, pos).tail.size
    assert eng.unpack_payloads(PackedPayloads(desc, bits, tail, pos.size - 1, var.size), pos).tobytes() == var.tobytes()
    src = PackedIn("device", desc, bits, tail, pos, pos.size - 1, var.size)
    st, out, bad, dst = unpack_call(eng, src.g, src.p, src.g.ptr("pos"), src.g.mem_kind, "device", var.size)
    assert st == _lib.CLG_OK and dst.get("var", var.size).tobytes() == var.tobytes() and dst.intact_outside("var", var.size)
    dst.free()
    src.g.free()


@pytest.mark.parametrize("name", ["config3", "random_log"])
def test_engine_round_trip_of_the_synthetic_columns(eng, name):
    var, pos = U.config3_column() if name == "config3" else U.random_log_column()
    want = host_packed(var, pos)
    eng.kernel_stats_reset()
    got = eng.pack_payloads(var, pos)
    U.assert_same_packed(got, want)
    assert eng.unpack_payloads(got, pos).tobytes() == var.tobytes()
    stats = eng.kernel_stats()
    assert stats["pack_payloads"]["launches"] > 0 and stats["unpack_payloads"]["launches"] > 0
    # device in, device out through the address form
    from _payload_util import upload
    dv, dp = upload(var), upload(pos)
    U.assert_same_packed(eng.pack_payloads(dv.p.value, dp.p.value, device=True, n_rows=pos.size - 1), want)
    dv.free()
    dp.free()
    # no rows: nothing is launched
    eng.kernel_stats_reset()
    empty = eng.pack_payloads(b"", [0])
    assert (empty.n_rows, empty.n_bytes) == (0, 0) and eng.unpack_payloads(empty, [0]).size == 0
    after = eng.kernel_stats()
    assert "pack_payloads" not in after and "unpack_payloads" not in after
