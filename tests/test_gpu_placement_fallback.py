"""GPU: CLG_MEM_MAPPED arrays that are not wholly inside one registered range.

Every entry point of the columns family that takes a memory kind resolves a registered array to
its device address; an array the registry does not hold whole is either staged through an engine
buffer (the outputs of the columns, the pack and the unpack, and the inputs of the pack and the
unpack) or refused (the inputs of clg_columnize and clg_encode_columns).  Two scenes reach that
branch:

  plain     every array in its own numpy allocation, nothing registered;
  straddle  one mapping of which only the leading pages are registered, the first array inside
            them and the second across their end (the rest lie past it).

A staged call must give the bytes of the same call with CLG_MEM_HOST arrays and leave the guard
bytes either side of every array alone; a refused call returns CLG_E_INVALID_ARG and writes
nothing.  Two engines, as in test_gpu_columns_small.py: the one-launch forms and (with
CLONOS_COLUMNS_SMALL=0) the multi-kernel forms both run on this input.

The straddle scene is also what holds the engine's copies to and from a staged array in pieces:
the HIP runtime refuses (hipErrorInvalidValue) one copy that crosses the end of registered
memory.  Before the copies were split at the edges of the registered ranges, every straddle case
here but the one-launch columns (which copy on the CPU) returned CLG_E_DEVICE."""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

from _columns_util import COLS, FILL, GUARD, GuardedColumns, exact_caps, oracle_batch, to_device
from _encode_util import IN_ARRAYS, arrays_of, columns_in, encoded, host_columns
from _pack_util import STREAMS
from test_gpu_pack_columns import mixed_columns

pytestmark = pytest.mark.gpu

SCENES = ("plain", "straddle")
BOTH = ("small", "multi")
WIDE = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")
DECODED = ("tag", "v0", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub")


@pytest.fixture(scope="module")
def engines():
    from clonos_amd import Engine
    small = Engine(segment_bytes=4096, pool_segments=256, timing=True)
    old = os.environ.get("CLONOS_COLUMNS_SMALL")
    os.environ["CLONOS_COLUMNS_SMALL"] = "0"
    try:
        multi = Engine(segment_bytes=4096, pool_segments=256, timing=True)
    finally:
        if old is None:
            del os.environ["CLONOS_COLUMNS_SMALL"]
        else:
            os.environ["CLONOS_COLUMNS_SMALL"] = old
    yield {"small": small, "multi": multi}
    small.close()
    multi.close()


def ok(status):
    """The call succeeded (the engine's error text otherwise)."""
    from clonos_amd import _lib
    assert status == _lib.CLG_OK, (status, _lib.lib.clg_last_error())
    return True


def taken(eng):
    return eng.kernel_stats().get("columns_small", {"launches": 0})["launches"]


class Spans:
    """Three spans, 301 records, 56 of them wide with payloads; no count is a multiple of 16."""

    def __init__(self):
        from clonos_amd import synth
        rng = np.random.default_rng(1)
        self.spans = [bytes(synth.config3_epoch(k, rng)[0]) for k in (211, 1, 89)]
        self.data = np.frombuffer(b"".join(self.spans), np.uint8)
        self.len = np.array([len(b) for b in self.spans], np.uint64)
        self.off = np.concatenate([[0], np.cumsum(self.len)[:-1]]).astype(np.uint64)
        self.batch = oracle_batch(self.spans)
        self.cols = host_columns(self.spans)   # the CPU's columns, for sizes and the encode's input
        c = self.cols
        self.n_class = [len(c.order), len(c.timestamp), len(c.rng), len(c.buffer_built), len(c.w_idx)]
        assert c.n_rec == 301 and int(c.w_var_len.sum()) > 0
        assert all(k % 16 for k in [c.n_rec] + self.n_class)


@pytest.fixture(scope="module")
def spans():
    return Spans()


class Memory:
    """GUARD | array | GUARD for each of `nbytes`, FILL everywhere, in one of the two scenes.
    ptr[i] is array i's address (16-byte aligned, arrays after the second 64-byte aligned)."""

    def __init__(self, scene, nbytes):
        from clonos_amd import _lib
        self._lib, self.nbytes, self.base = _lib, list(nbytes), None
        sizes = [2 * GUARD + n for n in nbytes]
        if scene == "plain":
            self.bufs = []
            for s in sizes:
                raw = np.empty(s + 64, np.uint8)
                o = -raw.ctypes.data % 64
                self.bufs.append(raw[o:o + s])
        else:
            assert scene == "straddle" and nbytes[1] > 16   # the second array crosses the registered end
            reg = (sizes[0] + GUARD + 16 + 4095) & ~4095
            at = [0, reg - 16 - GUARD]
            for s in sizes[1:-1]:
                at.append((at[-1] + s + 63) & ~63)
            region = np.frombuffer(mmap.mmap(-1, (at[-1] + sizes[-1] + 4095) & ~4095), np.uint8)
            assert reg % 4096 == 0 and reg < region.size
            self.bufs = [region[o:o + s] for o, s in zip(at, sizes)]
            _lib.check(_lib.lib.clg_host_register(region.ctypes.data, reg))
            self.base = region.ctypes.data
            p1 = self.bufs[1].ctypes.data + GUARD
            assert self.bufs[0].ctypes.data + sizes[0] <= self.base + reg and p1 < self.base + reg < p1 + nbytes[1]
        for b in self.bufs:
            b[:] = FILL
        self.ptr = [b.ctypes.data + GUARD for b in self.bufs]

    def put(self, arrays):
        for b, a in zip(self.bufs, arrays):
            a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            b[GUARD:GUARD + a.size] = a
        return self

    def data(self, i, n=None):
        return self.bufs[i][GUARD:GUARD + (self.nbytes[i] if n is None else n)].tobytes()

    def guards_intact(self):
        return all((b[:GUARD] == FILL).all() and (b[b.size - GUARD:] == FILL).all() for b in self.bufs)

    def untouched(self):
        return all((b == FILL).all() for b in self.bufs)

    def free(self):
        if self.base is not None:
            self._lib.check(self._lib.lib.clg_host_unregister(self.base))
            self.base = None


def guarded_columns(scene, caps, n_spans):
    """_columns_util's guarded columns, its arrays moved into a scene's memory (scene None: plain
    host arrays, CLG_MEM_HOST)."""
    from clonos_amd import _lib
    g = GuardedColumns("host", caps, n_spans)
    if scene is None:
        return g, None
    mem = Memory(scene, [caps[name] * np.dtype(dt).itemsize for name, dt, _, _ in COLS])
    for (name, _, _, _), b, p in zip(COLS, mem.bufs, mem.ptr):
        g.bufs[name] = b
        setattr(g.c, name, p)
    g.c.out_kind = _lib.CLG_MEM_MAPPED
    return g, mem


def same_columns(g, ref):
    assert int(g.c.n_rec) == int(ref.c.n_rec) and list(g.c.n_class) == list(ref.c.n_class)
    assert (g.base == ref.base).all()
    a, b = g.result(), ref.result()
    for name, _, _, _ in COLS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


# ---- staged: the outputs of the columns ------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_columnize_output(engines, spans, which, scene):
    from clonos_amd import _lib
    eng = engines[which]
    d, keep = to_device(spans.batch)
    base = np.ascontiguousarray(spans.batch.span_rec_base, np.uint64)
    caps = exact_caps(spans.cols.n_rec, spans.n_class)
    ref, _ = guarded_columns(None, caps, 3)
    g, mem = guarded_columns(scene, caps, 3)
    try:
        assert ok(_lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, 3, ref.c))
        before = taken(eng)
        assert ok(_lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, 3, g.c))
        assert taken(eng) - before == (which == "small")
        same_columns(g, ref)
        assert g.guards_intact() and ref.guards_intact()
    finally:
        mem.free()
    del keep


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_decode_host_columns(engines, spans, which, scene):
    from clonos_amd import _lib
    eng = engines[which]
    caps = exact_caps(spans.cols.n_rec, spans.n_class)
    ref, _ = guarded_columns(None, caps, 3)
    g, mem = guarded_columns(scene, caps, 3)
    call = lambda c: _lib.lib.clg_decode_host_columns(eng.handle, spans.data.ctypes.data, spans.off.ctypes.data,  # noqa: E731
                                                      spans.len.ctypes.data, 3, c)
    try:
        assert ok(call(ref.c))
        before = taken(eng)
        assert ok(call(g.c))
        assert taken(eng) - before == (which == "small")
        same_columns(g, ref)
        assert g.guards_intact() and ref.guards_intact()
        assert ref.result().tag.tobytes() == np.asarray(spans.cols.tag).tobytes()
    finally:
        mem.free()


# ---- staged: the pack and the unpack, inputs and outputs ---------------------------------------
PACK_COLS = mixed_columns(0, 23, [1025, 300, 77, 45, 33])   # 1025 tags: two blocks of one stream
SIDES = ("input", "output", "both")


def narrow_arrays(cols):
    return [np.ascontiguousarray(getattr(cols, name), dt) for name, dt, _ in STREAMS]


def columns_over(ptrs, lens, kind, caps=False):
    """clg_columns over the five narrow arrays at ptrs (None: null pointers)."""
    from clonos_amd import _lib
    c = _lib.Columns()
    for k, (name, _, _) in enumerate(STREAMS):
        setattr(c, name, ptrs[k] if ptrs else None)
    if caps:
        c.cap_tag, c.cap_order, c.cap_timestamp, c.cap_rng, c.cap_buffer_built = lens
    else:
        c.n_rec = lens[0]
        for k in range(4):
            c.n_class[k] = lens[k + 1]
    c.out_kind = kind
    return c


def packed_over(mem, cap_desc, cap_bits, kind):
    from clonos_amd import _lib
    p = _lib.Packed()
    p.desc, p.cap_desc, p.bits, p.cap_bits, p.out_kind = mem.ptr[0], cap_desc, mem.ptr[1], cap_bits, kind
    return p


def host_memory(nbytes):
    return Memory("plain", nbytes)   # (plain host arrays serve CLG_MEM_HOST too)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_pack_columns(engines, which, scene, side):
    from clonos_amd import _lib, pack_columns_host
    eng = engines[which]
    arrs = narrow_arrays(PACK_COLS)
    lens = [a.size for a in arrs]
    want = pack_columns_host(PACK_COLS)
    nb, nbits = want.desc.size, want.bits.size
    assert nb == 6 and want.blk_base[1] == 2
    H, M = _lib.CLG_MEM_HOST, _lib.CLG_MEM_MAPPED
    rin, rout = host_memory([a.nbytes for a in arrs]).put(arrs), host_memory([nb * 32, nbits])
    min_ = Memory(scene, [a.nbytes for a in arrs]).put(arrs) if side != "output" else rin
    mout = Memory(scene, [nb * 32, nbits]) if side != "input" else host_memory([nb * 32, nbits])
    try:
        ref = packed_over(rout, nb, nbits, H)
        assert ok(eng.pack_columns_raw(columns_over(rin.ptr, lens, H), ref))
        p = packed_over(mout, nb, nbits, M if side != "input" else H)
        assert ok(eng.pack_columns_raw(columns_over(min_.ptr, lens, M if side != "output" else H), p))
        assert list(p.n_val) == list(ref.n_val) == lens and list(p.blk_base) == list(ref.blk_base) and p.n_bits == ref.n_bits == nbits
        assert mout.data(0) == rout.data(0) == np.asarray(want.desc).tobytes()
        assert mout.data(1) == rout.data(1) == np.asarray(want.bits).tobytes()
        assert mout.guards_intact() and rout.guards_intact() and min_.guards_intact()
        assert all(min_.data(k) == a.tobytes() for k, a in enumerate(arrs))
    finally:
        min_.free()
        mout.free()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_unpack_columns(engines, which, scene, side):
    from clonos_amd import _lib, pack_columns_host
    eng = engines[which]
    arrs = narrow_arrays(PACK_COLS)
    lens = [a.size for a in arrs]
    packed = pack_columns_host(PACK_COLS)
    st = packed._struct()
    src = [np.asarray(packed.desc), np.asarray(packed.bits)]
    H, M = _lib.CLG_MEM_HOST, _lib.CLG_MEM_MAPPED

    def packed_in(mem, kind):
        p = _lib.Packed()
        C.memmove(C.byref(p), C.byref(st), C.sizeof(p))
        p.desc, p.bits, p.out_kind = mem.ptr[0], mem.ptr[1], kind
        return p

    rin, rout = host_memory([a.nbytes for a in src]).put(src), host_memory([a.nbytes for a in arrs])
    min_ = Memory(scene, [a.nbytes for a in src]).put(src) if side != "output" else rin
    mout = Memory(scene, [a.nbytes for a in arrs]) if side != "input" else host_memory([a.nbytes for a in arrs])
    try:
        bad = _lib.UnpackBad(9, 9, 9)
        ref = columns_over(rout.ptr, lens, H, caps=True)
        assert ok(eng.unpack_columns_raw(packed_in(rin, H), ref, bad))
        c = columns_over(mout.ptr, lens, M if side != "input" else H, caps=True)
        assert ok(eng.unpack_columns_raw(packed_in(min_, M if side != "output" else H), c, bad))
        assert (bad.what, bad.stream, bad.block) == (0, 0, 2 ** 64 - 1)
        assert [int(c.n_rec)] + [int(c.n_class[k]) for k in range(4)] == lens
        for k, a in enumerate(arrs):
            assert mout.data(k) == rout.data(k) == a.tobytes(), STREAMS[k][0]
        assert mout.guards_intact() and rout.guards_intact() and min_.guards_intact()
        assert all(min_.data(k) == a.tobytes() for k, a in enumerate(src))
    finally:
        min_.free()
        mout.free()


# The wide family has no one-launch form: the engines differ only in how the input columns are made,
# so one engine serves.  The pack reads the tags and the seven wide arrays, in this order.
WIDE_DT = {name: dt for name, dt, _, _ in COLS}
PACK_WIDE_IN = ("tag",) + WIDE
UNPACK_WIDE_OUT = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")   # then pos


def wide_columns_over(names, ptrs, spans, kind, caps=False):
    """clg_columns over the arrays `names` at ptrs, with the Spans input's counts."""
    from clonos_amd import _lib
    c = _lib.Columns()
    for name, p in zip(names, ptrs):
        setattr(c, name, p)
    if caps:
        c.cap_wide = spans.n_class[4]
    else:
        c.n_rec = spans.cols.n_rec
        c.n_class[4] = spans.n_class[4]
    c.out_kind = kind
    return c


def packed_wide_over(mem, cap_desc, cap_bits, kind):
    from clonos_amd import _lib
    p = _lib.PackedWideC()
    p.desc, p.cap_desc, p.bits, p.cap_bits, p.out_kind = mem.ptr[0], cap_desc, mem.ptr[1], cap_bits, kind
    return p


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("scene", SCENES)
def test_pack_wide(engines, spans, scene, side):
    from clonos_amd import _lib, pack_wide_host
    eng = engines["small"]
    arrs = [np.ascontiguousarray(getattr(spans.cols, name), WIDE_DT[name]) for name in PACK_WIDE_IN]
    assert arrs[0].size == 301 and all(a.size == 56 for a in arrs[1:])
    want = pack_wide_host(spans.cols)
    nb, nbits = want.desc.size, want.bits.size
    assert nb > 0 and nbits > 16
    H, M = _lib.CLG_MEM_HOST, _lib.CLG_MEM_MAPPED
    rin, rout = host_memory([a.nbytes for a in arrs]).put(arrs), host_memory([nb * 32, nbits])
    min_ = Memory(scene, [a.nbytes for a in arrs]).put(arrs) if side != "output" else rin
    mout = Memory(scene, [nb * 32, nbits]) if side != "input" else host_memory([nb * 32, nbits])
    try:
        ref = packed_wide_over(rout, nb, nbits, H)
        assert ok(eng.pack_wide_raw(wide_columns_over(PACK_WIDE_IN, rin.ptr, spans, H), ref))
        p = packed_wide_over(mout, nb, nbits, M if side != "input" else H)
        assert ok(eng.pack_wide_raw(wide_columns_over(PACK_WIDE_IN, min_.ptr, spans, M if side != "output" else H), p))
        assert list(p.n_val) == list(ref.n_val) == want.n_val and list(p.blk_base) == list(ref.blk_base) == want.blk_base
        assert p.n_bits == ref.n_bits == nbits and p.bad_row == ref.bad_row
        assert mout.data(0) == rout.data(0) == np.asarray(want.desc).tobytes()
        assert mout.data(1) == rout.data(1) == np.asarray(want.bits).tobytes()
        assert mout.guards_intact() and rout.guards_intact() and min_.guards_intact()
        assert all(min_.data(k) == a.tobytes() for k, a in enumerate(arrs))
    finally:
        min_.free()
        mout.free()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("scene", SCENES)
def test_unpack_wide(engines, spans, scene, side):
    """The packed input and the eight outputs: w_idx, the six fields and pos."""
    from clonos_amd import _lib, pack_wide_host, unpack_wide_host
    eng = engines["small"]
    packed = pack_wide_host(spans.cols)
    st = packed._struct()
    src = [np.asarray(packed.desc), np.asarray(packed.bits)]
    want = unpack_wide_host(packed)
    pos = np.concatenate([[0], np.cumsum(want["w_var_len"], dtype=np.uint64)]).astype(np.uint64)
    outs = [want[name] for name in UNPACK_WIDE_OUT] + [pos]
    assert all(want[name].tobytes() == np.ascontiguousarray(getattr(spans.cols, name), WIDE_DT[name]).tobytes()
               for name in UNPACK_WIDE_OUT)
    assert pos.size == 57 and int(pos[-1]) > 0
    H, M = _lib.CLG_MEM_HOST, _lib.CLG_MEM_MAPPED

    def packed_in(mem, kind):
        p = _lib.PackedWideC()
        C.memmove(C.byref(p), C.byref(st), C.sizeof(p))
        p.desc, p.bits, p.out_kind = mem.ptr[0], mem.ptr[1], kind
        return p

    rin, rout = host_memory([a.nbytes for a in src]).put(src), host_memory([a.nbytes for a in outs])
    min_ = Memory(scene, [a.nbytes for a in src]).put(src) if side != "output" else rin
    mout = Memory(scene, [a.nbytes for a in outs]) if side != "input" else host_memory([a.nbytes for a in outs])
    try:
        bad = _lib.UnpackBad(9, 9, 9)
        ref = wide_columns_over(UNPACK_WIDE_OUT, rout.ptr, spans, H, caps=True)
        assert ok(eng.unpack_wide_raw(packed_in(rin, H), ref, rout.ptr[7], bad))
        c = wide_columns_over(UNPACK_WIDE_OUT, mout.ptr, spans, M if side != "input" else H, caps=True)
        assert ok(eng.unpack_wide_raw(packed_in(min_, M if side != "output" else H), c, mout.ptr[7], bad))
        assert (bad.what, bad.stream, bad.block) == (0, 0, 2 ** 64 - 1)
        assert int(c.n_class[4]) == int(ref.n_class[4]) == 56
        for k, a in enumerate(outs):
            assert mout.data(k) == rout.data(k) == a.tobytes(), (UNPACK_WIDE_OUT + ("pos",))[k]
        assert mout.guards_intact() and rout.guards_intact() and min_.guards_intact()
        assert all(min_.data(k) == a.tobytes() for k, a in enumerate(src))
    finally:
        min_.free()
        mout.free()


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_decode_host_columns_packed(engines, spans, which, scene):
    """The wide rows and the packed narrow columns, both into the scene's memory."""
    from clonos_amd import _lib
    eng = engines[which]
    H, M = _lib.CLG_MEM_HOST, _lib.CLG_MEM_MAPPED
    nw = spans.n_class[4]
    wide_bytes = [nw * np.dtype(dt).itemsize for name, dt, _, _ in COLS if name in WIDE]
    sizes = _lib.Packed()   # a sizes-only call for the capacities
    assert ok(_lib.lib.clg_decode_host_columns_packed(eng.handle, spans.data.ctypes.data, spans.off.ctypes.data,
                                                      spans.len.ctypes.data, 3, _lib.Columns(), None, sizes))
    nb, nbits = int(sizes.blk_base[len(STREAMS)]), int(sizes.n_bits)
    assert nb == 5 and nbits > 0

    def run(wmem, pmem, kind):
        c = _lib.Columns()
        for name, p in zip(WIDE, wmem.ptr):
            setattr(c, name, p)
        sb = np.zeros(4 * 5, np.uint64)
        c.cap_wide, c.span_base, c.out_kind = nw, sb.ctypes.data, kind
        p = packed_over(pmem, nb, nbits, kind)
        st = _lib.lib.clg_decode_host_columns_packed(eng.handle, spans.data.ctypes.data, spans.off.ctypes.data,
                                                     spans.len.ctypes.data, 3, c, None, p)
        return st, c, p, sb

    rw, rp = host_memory(wide_bytes), host_memory([nb * 32, nbits])
    mw, mp = Memory(scene, wide_bytes), Memory(scene, [nb * 32, nbits])
    try:
        st, rc, rpk, rsb = run(rw, rp, H)
        assert ok(st)
        st, c, pk, sb = run(mw, mp, M)
        assert ok(st)
        assert int(c.n_rec) == int(rc.n_rec) == 301 and list(c.n_class) == list(rc.n_class) == spans.n_class
        assert (sb == rsb).all() and (sb.reshape(4, 5) == np.asarray(spans.cols.span_base)).all()
        assert list(pk.n_val) == list(rpk.n_val) and list(pk.blk_base) == list(rpk.blk_base) and pk.n_bits == rpk.n_bits
        for k in range(len(WIDE)):
            assert mw.data(k) == rw.data(k), WIDE[k]
        assert mw.data(0) == np.asarray(spans.cols.w_idx).tobytes()
        assert mp.data(0) == rp.data(0) and mp.data(1) == rp.data(1)
        assert mw.guards_intact() and mp.guards_intact() and rw.guards_intact() and rp.guards_intact()
    finally:
        mw.free()
        mp.free()


# ---- refused: the inputs of clg_columnize and clg_encode_columns --------------------------------
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_columnize_input_is_refused(engines, spans, which, scene):
    from clonos_amd import _lib
    eng = engines[which]
    b = spans.batch
    arrs = [np.ascontiguousarray(getattr(b, k)) for k in DECODED]
    mem = Memory(scene, [a.nbytes for a in arrs]).put(arrs)
    d = _lib.Decoded()
    for k, p in zip(DECODED, mem.ptr):
        setattr(d, k, p)
    d.n_rec, d.n_wide, d.out_kind = b.n_rec, len(b.w_idx), _lib.CLG_MEM_MAPPED
    d.cap, d.wcap = d.n_rec, d.n_wide
    base = np.ascontiguousarray(b.span_rec_base, np.uint64)
    g, _ = guarded_columns(None, exact_caps(spans.cols.n_rec, spans.n_class), 3)
    try:
        assert _lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, 3, g.c) == _lib.CLG_E_INVALID_ARG
        assert g.untouched()
        assert all(mem.data(k) == a.tobytes() for k, a in enumerate(arrs)) and mem.guards_intact()
    finally:
        mem.free()


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("which", BOTH)
def test_encode_columns_input_is_refused(engines, spans, which, scene):
    from clonos_amd import _lib
    eng = engines[which]
    arrs = arrays_of(spans.cols)
    names = [name for name, _, _ in IN_ARRAYS]
    mem = Memory(scene, [arrs[k].nbytes for k in names]).put([arrs[k] for k in names])
    total = int(spans.len.sum())
    out = np.full(total + 2 * GUARD, FILL, np.uint8)
    try:
        cin, keep = columns_in(arrs, spans.cols.span_base, _lib.CLG_MEM_MAPPED, dict(zip(names, mem.ptr)))
        enc, sbb = encoded(out.ctypes.data + GUARD, total, 3, _lib.CLG_MEM_HOST)
        assert eng.encode_columns_raw(cin, enc) == _lib.CLG_E_INVALID_ARG
        assert (out == FILL).all()
        # (the same columns as plain host arrays encode to the spans' bytes)
        cin, keep = columns_in(arrs, spans.cols.span_base, _lib.CLG_MEM_HOST)
        assert ok(eng.encode_columns_raw(cin, enc))
        assert out[GUARD:GUARD + total].tobytes() == spans.data.tobytes()
    finally:
        mem.free()
