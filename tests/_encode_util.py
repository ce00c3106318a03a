"""Shared by the encode-columns tests: host columns with their payload column from span bytes (the
oracle's decode, clg_columnize_host, clg_gather_payloads_host), clg_columns_in over host or device
arrays, and the placed-payload logs of test_gpu_payload_logs.py (its helpers, copied)."""
import ctypes as C

import numpy as np

from _columns_util import oracle_batch

FILL = 0xA5
GUARD = 64
NONE = 0xFFFFFFFFFFFFFFFF
# clg_columns_in's arrays: name, dtype, the class whose count is its length (None: n_rec; 5: n_wide + 1; 6: n_var)
IN_ARRAYS = (("tag", np.uint8, None), ("order", np.int8, 0), ("timestamp", np.int64, 1), ("rng", np.int32, 2),
             ("buffer_built", np.int32, 3), ("w_rc", np.int32, 4), ("w_v1", np.int64, 4), ("w_var_len", np.uint32, 4),
             ("w_sub", np.uint8, 4), ("w_v0", np.int64, 4), ("w_idx", np.uint32, 4), ("pos", np.uint64, 5),
             ("var", np.uint8, 6))


def host_columns(spans):
    """Typed columns of the spans with their payload column, all on the CPU."""
    from clonos_amd import columnize_host, gather_payloads_host
    spans = [bytes(b) for b in spans]
    cols = columnize_host(oracle_batch(spans))
    lens = np.array([len(b) for b in spans], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(spans) else np.zeros(0, np.uint64)
    cols.var, cols.var_pos = gather_payloads_host(b"".join(spans), offs, lens, cols.w_var_off, cols.w_var_len,
                                                  cols.span_base[:, 4])
    return cols


def arrays_of(cols):
    """name -> contiguous host array of clg_columns_in's arrays, from a DecodedColumns."""
    a = {name: np.ascontiguousarray(getattr(cols, name), dt) for name, dt, _ in IN_ARRAYS[:11]}
    a["pos"] = np.ascontiguousarray(cols.var_pos, np.uint64)
    a["var"] = np.ascontiguousarray(cols.var, np.uint8)
    return a


def columns_in(arrs, span_base, kind=0, ptr=None, idx=True):
    """clg_columns_in over arrs (name -> host array; lengths give the counts).  ptr: name -> address
    to pass instead of the host array's (device or registered memory).  span_base: (n + 1, 5) or
    None (one span).  Returns (struct, keep-alive list)."""
    from clonos_amd import _lib
    cin = _lib.ColumnsIn()
    keep = [arrs]
    for name, _, _ in IN_ARRAYS:
        if name == "w_idx" and not idx:
            continue
        a = arrs[name]
        setattr(cin, name, (ptr[name] if ptr is not None else a.ctypes.data) if a.size or ptr is not None else None)
    cin.n_rec = arrs["tag"].size
    for c, name in enumerate(("order", "timestamp", "rng", "buffer_built", "w_v0")):
        cin.n_class[c] = arrs[name].size
    cin.n_var = arrs["var"].size
    if span_base is not None:
        sb = np.ascontiguousarray(span_base, np.uint64).reshape(-1)
        keep.append(sb)
        cin.span_base, cin.n_spans = sb.ctypes.data, sb.size // 5 - 1
    cin.in_kind = kind
    return cin, keep


def encoded(buf=None, cap=0, n_spans=1, kind=0):
    """(clg_encoded, span_byte_base array) over an output address (None: sizes only)."""
    from clonos_amd import _lib
    enc = _lib.Encoded()
    sbb = np.full(max(n_spans, 1) + 1, NONE, np.uint64)
    enc.bytes, enc.cap, enc.out_kind, enc.span_byte_base = buf, cap, kind, sbb.ctypes.data
    return enc, sbb


def span_lengths(spans):
    return np.concatenate([[0], np.cumsum([len(b) for b in spans])]).astype(np.uint64)


# ---- the placed-payload logs (test_gpu_payload_logs.py's helpers) ------------------------------
C256 = 256


def ascii_bytes(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))


def payload_record(kind, payload, i):
    """(determinant, offset of the payload in its record, payload bytes as the decode reports them)."""
    from clonos_amd import determinants as D
    if kind == "timer":       # [tag][rc i32][ts i64][type][len i32][name]
        return D.TimerTriggerDeterminant(100 + i, 5000 + i, D.INTERNAL, payload), 18, payload
    if kind == "source":      # [tag][rc i32][id i64][ts i64][type][has ref][len i32][ref]
        return D.SourceCheckpointDeterminant(200 + i, 7 + i, 9000 + i, D.CHECKPOINT, payload), 27, payload
    stream = D.jser_string(payload.decode())  # [tag][AC ED 00 05 74][len u16][chars]: the stream is the payload
    return D.SerializableDeterminant(stream), 1, stream


def padding(p):
    """p bytes of short records (ORDER 2 B, RNG 5 B); p is 0, 2, or at least 4."""
    from clonos_amd import determinants as D
    assert p >= 0 and p not in (1, 3)
    out = b""
    if p % 2:
        out += D.encode(D.RNGDeterminant(p))
        p -= 5
    return out + D.encode(D.OrderDeterminant(3)) * (p // 2)


def placed(prefix, wants, seg, rng):
    """prefix, then for each (kind, start mod seg, payload length) a record whose payload starts at
    that physical residue (padding records before it).  Returns the bytes."""
    from clonos_amd import determinants as D
    buf = bytearray(prefix)
    for i, (kind, start_mod, length) in enumerate(wants):
        plen = length if kind != "serial" else length - 7  # (a TC_STRING stream is 7 bytes + its chars)
        det, rel, payload = payload_record(kind, ascii_bytes(rng, plen), i)
        assert len(payload) == length
        pad = (start_mod - rel - len(buf)) % seg
        if pad in (1, 3):
            pad += seg
        buf += padding(pad) + D.encode(det)
        assert (len(buf) - length) % seg == start_mod
    return bytes(buf)


# (kind, payload start mod 256, payload length)
WANTS_256 = [
    ("timer", 255, 20), ("source", 255, 100), ("serial", 255, 300),   # start on a segment's last byte
    ("timer", 236, 20), ("serial", 156, 100), ("source", 0, 256),     # end exactly at a segment's end
    ("source", 250, 40), ("timer", 230, 63),                           # short, one boundary
    ("timer", 200, 100), ("serial", 200, 400), ("source", 100, 1300),  # long: one, two, five boundaries
    ("timer", 17, 0), ("timer", 40, 1), ("source", 255, 1), ("timer", 1, 64), ("serial", 129, 65),
]


def placed_spans():
    """The three spans of test_gpu_payload_logs.py's placed logs: one that starts mid-segment, one
    from a log's start, one empty."""
    from clonos_amd import synth
    rng = np.random.default_rng(0x9A7)
    first = synth.random_log(60, rng, allow_serializable=False)
    first += padding((300 - len(first)) % C256 + (C256 if (300 - len(first)) % C256 in (1, 3) else 0))
    a = placed(first, WANTS_256, C256, rng)
    b = placed(b"", list(reversed(WANTS_256)), C256, rng)
    return [a[len(first):], b, b""]


class GuardedDevice:
    """Host arrays uploaded to device memory, each with GUARD bytes of FILL either side and `shift`
    more bytes before it (so an array can start at base + k); ptr[name] is the array's address."""

    def __init__(self, arrs, shift=None):
        from _devbuf import DeviceBuf
        self.bufs, self.ptr, self.want = {}, {}, {}
        hip = None
        for name, a in arrs.items():
            k = (shift or {}).get(name, 0)
            raw = np.full(2 * GUARD + k + a.nbytes, FILL, np.uint8)
            raw[GUARD + k:GUARD + k + a.nbytes] = a.view(np.uint8).reshape(-1)
            b = DeviceBuf(max(raw.size, 1), fill=FILL)
            hip = b.hip
            assert hip.hipMemcpy(b.p, C.c_void_p(raw.ctypes.data), C.c_size_t(raw.size), 1) == 0
            self.bufs[name], self.ptr[name], self.want[name] = b, b.p.value + GUARD + k, raw
        if hip is not None:
            assert hip.hipDeviceSynchronize() == 0

    def intact(self):
        return all((b.host()[:self.want[n].size] == self.want[n]).all() for n, b in self.bufs.items())

    def free(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}
