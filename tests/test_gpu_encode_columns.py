"""GPU: typed columns back to log bytes (clg_encode_columns, encode_columns.hip).  Every expected
value is the spans' own bytes (the oracle decodes them, clg_columnize_host and
clg_gather_payloads_host make the columns on the CPU) or the CPU version's results, never the
device path's.  T is the write tile's record count and LDS its staging buffer, read from the
headers."""
import ctypes as C
import mmap
import os
import re

import numpy as np
import pytest

from _encode_util import (FILL, GUARD, NONE, GuardedDevice, arrays_of, columns_in, encoded, host_columns, placed_spans,
                          span_lengths)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_const(path, name):
    text = open(os.path.join(ROOT, "clonos_amd", "csrc", path)).read()
    m = re.search(r"constexpr uint32_t %s = ([^;]+);" % name, text)
    return m.group(1).strip()


assert header_const("encode_columns.h", "kEcolTile") == "kColTile"
T = int(header_const("columns.h", "kColTile"))
LDS = eval(header_const("encode_columns.h", "kEcolLds"))
WAVE_ROW = int(header_const("encode_columns.h", "kEcolWaveRow"))
assert T == 4096 and LDS == 65536 and WAVE_ROW == 64

MIXES = {
    "order": ["order"],
    "timestamp": ["timestamp"],
    "order_timestamp": ["order", "timestamp"],
    "wide": ["timer_pts", "timer_87", "source_cp", "ignore_cp", "ser_string", "ser_boolean", "ser_integer"],
}


def mix_bytes(names, n, rng):
    """(bytes, record offsets with the end) of n records drawn evenly from the named synth kinds."""
    from clonos_amd import synth
    if names == "config3":
        b, offs = synth.config3_epoch(n, rng)
        return bytes(b), np.append(offs, len(b))
    kinds = [synth.KINDS[k] for k in names]
    idx = rng.integers(0, len(kinds), n)
    fields = {}
    for ki, kd in enumerate(kinds):
        cnt = int((idx == ki).sum())
        fields[ki] = [rng.integers(0, 2 if kd.name == "ser_boolean" else 1 << min(8 * w - 1, 62), cnt) for _, w in kd.patches]
    b, offs = synth.build(idx, kinds, fields)
    return bytes(b), np.append(offs, len(b))


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    e = Engine(segment_bytes=256, pool_segments=1 << 12, timing=True)
    yield e
    e.close()


@pytest.mark.parametrize("mix", ["order", "timestamp", "order_timestamp", "wide", "config3"])
def test_sizes_and_mixes(eng, mix):
    rng = np.random.default_rng(0xE5 + len(mix))
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        b, _ = mix_bytes(MIXES.get(mix, mix), n, rng)
        cols = host_columns([b])
        assert cols.n_rec == n
        assert eng.encode_columns(cols) == b, (mix, n)


def wide_record(rng, i, length):
    from clonos_amd import determinants as D
    name = bytes(rng.integers(97, 123, length, dtype=np.uint8))
    if i % 2:
        return D.encode(D.SourceCheckpointDeterminant(7 + i, 11 + i, 9000 + i, D.CHECKPOINT, name))
    return D.encode(D.TimerTriggerDeterminant(100 + i, 5000 + i, D.INTERNAL, name))


def test_wide_records_at_the_tile_edges(eng):
    """A wide record as the last and as the first record of a tile: short payloads, long ones, none."""
    from clonos_amd import determinants as D
    rng = np.random.default_rng(0x7E)
    order = D.encode(D.OrderDeterminant(3))
    for lengths in ((5, 9), (70, 200), (0, 64)):
        w = [wide_record(rng, i, lengths[i % 2]) for i in range(4)]
        ign = D.encode(D.IgnoreCheckpointDeterminant(3, 4))
        b = order * (T - 1) + w[0] + w[1] + order * (T - 3) + ign + w[2] + w[3] + order
        cols = host_columns([b])
        assert cols.n_rec == 2 * T + 2 and cols.tag[T - 1] >= 3 and cols.tag[T] >= 3 and cols.tag[2 * T] >= 3
        assert eng.encode_columns(cols) == b


PAYLOAD_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65)


def payload_batch(rng, giant=0):
    """Timer names, storage references and Serializable streams of every edge length between short
    records; giant: one more reference of that many bytes."""
    from clonos_amd import determinants as D, synth
    parts = []
    for i, L in enumerate(PAYLOAD_LENGTHS + (300, 1300)):
        parts += [synth.random_log(3, rng, allow_serializable=False), wide_record(rng, 2 * i, L), wide_record(rng, 2 * i + 1, L)]
        if L >= 7:
            parts.append(D.encode(D.SerializableDeterminant(D.jser_string("s" * (L - 7)))))
    if giant:
        parts.insert(len(parts) // 2, wide_record(rng, 1, giant))
    return b"".join(parts)


def test_payload_lengths_staged_and_direct(eng):
    rng = np.random.default_rng(0x9A)
    staged = payload_batch(rng)
    assert len(staged) + 16 <= LDS  # one tile, through the LDS buffer (its long rows skip it)
    cols = host_columns([staged])
    assert set(PAYLOAD_LENGTHS) <= set(cols.w_var_len.tolist())
    assert eng.encode_columns(cols) == staged
    direct = payload_batch(rng, giant=LDS + 5000)
    assert LDS + 5000 > LDS  # the premise: this tile's bytes cannot fit the buffer, it stores directly
    cols = host_columns([direct])
    assert int(cols.w_var_len.max()) > LDS
    assert eng.encode_columns(cols) == direct


def device_run(eng, arrs, span_base, out_shift=0, shift=None, cap=None, idx=True):
    """Device columns to a device output at base + GUARD + out_shift.  Returns (status, enc, sbb,
    output bytes incl. guards, inputs intact)."""
    from _devbuf import DeviceBuf
    from clonos_amd import _lib
    dev = GuardedDevice(arrs, shift)
    ns = 1 if span_base is None else len(span_base) - 1
    e0, _ = encoded(None, 0, ns)
    want = 0
    if cap is None:
        cin, keep = columns_in(arrs, span_base, _lib.CLG_MEM_DEVICE, dev.ptr, idx)
        st = eng.encode_columns_raw(cin, e0)
        assert st == _lib.CLG_OK, st
        want = int(e0.n_bytes)
    size = want if cap is None else cap
    out = DeviceBuf(2 * GUARD + 16 + size, fill=FILL)
    cin, keep = columns_in(arrs, span_base, _lib.CLG_MEM_DEVICE, dev.ptr, idx)
    enc, sbb = encoded(out.p.value + GUARD + out_shift, size, ns, _lib.CLG_MEM_DEVICE)
    st = eng.encode_columns_raw(cin, enc)
    raw = out.host()
    ok = dev.intact()
    out.free()
    dev.free()
    return st, enc, sbb, raw, ok


def test_every_output_and_var_alignment(eng):
    """Device output at base + k for every k in 0..15 and var at base + k for k in 0, 1, 15: the
    bytes, and the guard bytes either side of the output and of every input."""
    rng = np.random.default_rng(0xA11)
    b = payload_batch(rng)
    arrs = arrays_of(host_columns([b]))
    for k in range(16):
        for vk in ((0, 1, 15) if k in (0, 5) else (0,)):
            st, enc, sbb, raw, ok = device_run(eng, arrs, None, out_shift=k, shift={"var": vk})
            assert st == 0 and enc.n_bytes == len(b) and ok
            at = GUARD + k
            assert raw[at:at + len(b)].tobytes() == b, (k, vk)
            assert (raw[:at] == FILL).all() and (raw[at + len(b):] == FILL).all(), (k, vk)


def cut_spans(b, offs, cuts):
    return [b[offs[a]:offs[z]] for a, z in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("n_spans", [1, 3, 70])
def test_spans(eng, n_spans):
    """Boundaries exactly on a tile edge and one record either side, empty spans, 70 spans."""
    rng = np.random.default_rng(0x5A + n_spans)
    n = 2 * T + 1
    b, offs = mix_bytes("config3", n, rng)
    if n_spans == 1:
        cuts = [0, n]
    elif n_spans == 3:
        cuts = [0, T, T, n]
    else:
        cuts = sorted([0, 0, T - 1, T, T + 1, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, n, n] +
                      [int(x) for x in rng.integers(0, n + 1, 70 + 1 - 11)])
    spans = cut_spans(b, offs, cuts)
    assert len(spans) == n_spans
    cols = host_columns(spans)
    assert eng.encode_columns(cols, per_span=True) == spans
    assert eng.encode_columns(cols) == b
    # the raw call's span_byte_base, and span_base null: one span
    from clonos_amd import _lib
    cin, keep = columns_in(arrays_of(cols), cols.span_base)
    enc, sbb = encoded(None, 0, n_spans)
    assert eng.encode_columns_raw(cin, enc) == _lib.CLG_OK
    assert (sbb == span_lengths(spans)).all()
    cin, keep = columns_in(arrays_of(cols), None)
    enc, sbb = encoded(None, 0, 1)
    assert eng.encode_columns_raw(cin, enc) == _lib.CLG_OK and list(sbb) == [0, len(b)]


class Mapped:
    """Registered host memory (clg_host_register) holding arrays at 64-byte steps."""

    def __init__(self, nbytes):
        from clonos_amd import _lib
        self._lib = _lib
        self.region = np.frombuffer(mmap.mmap(-1, (nbytes + 8191) & ~4095), np.uint8)
        self.region[:] = FILL
        _lib.check(_lib.lib.clg_host_register(self.region.ctypes.data, self.region.size))
        self.at = 0

    def put(self, a):
        p = self.take(a.nbytes)
        self.region[p - self.region.ctypes.data:p - self.region.ctypes.data + a.nbytes] = a.view(np.uint8).reshape(-1)
        return p

    def take(self, n):
        p = self.region.ctypes.data + self.at
        self.at += (n + 63) & ~63
        assert self.at <= self.region.size
        return p

    def free(self):
        self._lib.lib.clg_host_unregister(self.region.ctypes.data)


def test_memory_kinds_give_identical_bytes(eng):
    from _devbuf import DeviceBuf
    from clonos_amd import _lib
    rng = np.random.default_rng(0x3E3)
    spans = [payload_batch(rng), b"", mix_bytes("config3", 500, rng)[0]]
    cols = host_columns(spans)
    whole = b"".join(spans)
    arrs = arrays_of(cols)
    dev = GuardedDevice(arrs)
    mp = Mapped(sum(a.nbytes + 64 for a in arrs.values()) + len(whole) + 4096)
    mptr = {k: mp.put(a) for k, a in arrs.items()}
    m_out = mp.take(len(whole))
    d_out = DeviceBuf(len(whole) + 64, fill=FILL)
    h_out = np.full(len(whole), FILL, np.uint8)
    ins = {"host": (_lib.CLG_MEM_HOST, None), "device": (_lib.CLG_MEM_DEVICE, dev.ptr), "mapped": (_lib.CLG_MEM_MAPPED, mptr)}
    for ik, (kind, ptr) in ins.items():
        for ok in ("host", "device", "mapped"):
            cin, keep = columns_in(arrs, cols.span_base, kind, ptr)
            dst = {"host": h_out.ctypes.data, "device": d_out.p.value, "mapped": m_out}[ok]
            enc, sbb = encoded(dst, len(whole), len(spans), ins[ok][0])
            assert eng.encode_columns_raw(cin, enc) == _lib.CLG_OK, (ik, ok)
            assert (sbb == span_lengths(spans)).all()
            if ok == "host":
                got = h_out.tobytes()
                h_out[:] = FILL
            elif ok == "device":
                got = d_out.host()[:len(whole)].tobytes()
                d_out.fill(FILL)
            else:
                o = m_out - mp.region.ctypes.data
                got = mp.region[o:o + len(whole)].tobytes()
                mp.region[o:o + len(whole)] = FILL
            assert got == whole, (ik, ok)
    assert dev.intact()
    d_out.free()
    dev.free()
    mp.free()


def test_round_trip_from_logs(engine):
    """decode_logs_columns(payloads=True) of logs in 256-byte segments, then encode_columns: each
    log's getDeterminants, and what encode_batch gives over to_soa()."""
    from clonos_amd import CausalLogID
    spans = placed_spans()
    logs = []
    for i, b in enumerate(spans):
        lg = engine.open_log(CausalLogID.main(i))
        if len(b):
            lg.appendDeterminant(bytes(b), 0)
        logs.append(lg)
    cols = engine.decode_logs_columns(logs, [0] * len(logs), payloads=True)
    got = engine.encode_columns(cols, per_span=True)
    assert got == [lg.getDeterminants(0) for lg in logs] == [bytes(s) for s in spans]
    b = cols.to_soa()
    assert b"".join(got) == engine.encode_batch(b.tag, b.v0, b.w_idx, b.w_rc, b.w_v1, b.w_var_off, b.w_var_len, b.w_sub,
                                                cols.var.tobytes())


def test_errors_capacity_and_sizes_leave_the_output_untouched(eng):
    """Every error kind with the CPU version's answer, CLG_E_CAPACITY and sizes only."""
    from clonos_amd import _lib
    rng = np.random.default_rng(0xBAD)
    n = T + 300
    b, offs = mix_bytes("config3", n, rng)
    cuts = [0, 100, T - 1, T + 5, n]
    spans = cut_spans(b, offs, cuts)
    cols = host_columns(spans)
    total = len(b)
    E = _lib.CLG_E_INVALID_ARG

    def both(arrs, sb, idx=True):
        """The device call's (status, what, index), checked against the CPU version's."""
        cin, keep = columns_in(arrs, sb, idx=idx)
        enc, _ = encoded(None, 0, len(sb) - 1)
        hst = _lib.lib.clg_encode_columns_host(C.byref(cin), C.byref(enc))
        want = (hst, int(enc.bad_what), int(enc.bad_index))
        st, enc, sbb, raw, ok = device_run(eng, arrs, sb, cap=total, idx=idx)
        assert (raw == FILL).all() and ok
        assert (st, int(enc.bad_what), int(enc.bad_index)) == want
        return want

    a = arrays_of(cols)
    a["tag"] = a["tag"].copy()
    a["tag"][[T + 7, n - 2]] = [8, 200]
    assert both(a, cols.span_base) == (E, _lib.ENC_BAD_TAG, T + 7)

    a = arrays_of(cols)
    a["timestamp"] = a["timestamp"][:-1].copy()  # one fewer stated than the tags hold
    assert both(a, cols.span_base) == (E, _lib.ENC_BAD_TOTALS, 1)

    tags = np.asarray(cols.tag)[np.asarray(cols.w_idx)]
    rows = np.nonzero(((tags == 3) | ((tags == 4) & (cols.w_sub == 6))) & (cols.w_var_len > 0))[0]
    a = arrays_of(cols)
    a["pos"] = a["pos"].copy()
    a["pos"][rows[-1]] = a["var"].size
    a["pos"][rows[len(rows) // 2]] = 0xFFFFFFFFFFFFFFFF - 1
    assert both(a, cols.span_base) == (E, _lib.ENC_BAD_ROW, int(rows[len(rows) // 2]))

    a = arrays_of(cols)
    a["w_idx"] = a["w_idx"].copy()
    a["w_idx"][[len(a["w_idx"]) - 1, 3]] += 1
    assert both(a, cols.span_base) == (E, _lib.ENC_BAD_ROW, 3)

    sb = np.array(cols.span_base, np.uint64)
    dec = sb.copy()
    dec[3] = 0
    assert both(arrays_of(cols), dec) == (E, _lib.ENC_BAD_SPAN, 2)
    last = sb.copy()
    last[-1, 0] += 1
    assert both(arrays_of(cols), last) == (E, _lib.ENC_BAD_SPAN, len(spans))
    moved = sb.copy()
    frm = int(np.nonzero(moved[2] > moved[1])[0][0])
    to = int([k for k in range(5) if k != frm and moved[2][k] < moved[3][k]][0])
    moved[2, frm] -= 1
    moved[2, to] += 1
    assert both(arrays_of(cols), moved) == (E, _lib.ENC_BAD_SPAN, 2)

    # w_idx not given: not checked
    a = arrays_of(cols)
    a["w_idx"] = a["w_idx"] + 1
    st, enc, sbb, raw, ok = device_run(eng, a, cols.span_base, idx=False)
    assert st == _lib.CLG_OK and raw[GUARD:GUARD + total].tobytes() == b

    # capacity: the results filled, nothing written; sizes only
    st, enc, sbb, raw, ok = device_run(eng, arrays_of(cols), cols.span_base, cap=total - 1)
    assert st == _lib.CLG_E_CAPACITY and enc.n_bytes == total and (sbb == span_lengths(spans)).all()
    assert (raw == FILL).all() and ok
    cin, keep = columns_in(arrays_of(cols), cols.span_base)
    enc, sbb = encoded(None, 0, len(spans))
    assert eng.encode_columns_raw(cin, enc) == _lib.CLG_OK
    assert enc.n_bytes == total and enc.bad_what == 0 and enc.bad_index == NONE and (sbb == span_lengths(spans)).all()


def test_columns_without_a_payload_column_raise(eng):
    from _columns_util import oracle_batch
    from clonos_amd import columnize_host
    with pytest.raises(ValueError):
        eng.encode_columns(columnize_host(oracle_batch([mix_bytes(["order"], 10, np.random.default_rng(1))[0]])))


def test_stats(eng):
    eng.kernel_stats_reset()
    b, _ = mix_bytes("config3", 1000, np.random.default_rng(5))
    assert eng.encode_columns(host_columns([b])) == b
    st = eng.kernel_stats()["encode_columns"]
    assert st["launches"] >= 2 and st["bytes"] >= len(b)
