"""Host-side mirror of Clonos' ThreadCausalLog / DeterminantEncoder (decode) on top of the
C-ABI of libclonos_engine.so.

Method names follow the reference Java interfaces so parity tests read like the
reference's own code:
  ThreadCausalLog  reference flink-runtime/.../causal/log/thread/ThreadCausalLog.java:33-96
  JobCausalLog     reference flink-runtime/.../causal/log/job/JobCausalLog.java:50-78 (see job.py)
Errors surface as ClonosError carrying the C status (the Java side throws the matching
exception: CorruptDeterminantArrayException, RuntimeException("Consumer went backwards"), ...).
"""
from __future__ import annotations

import collections
import ctypes as C
import mmap
import sys
import threading
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import ClonosError, check, lib
from . import determinants as D

ChannelLike = Union[Tuple[int, int], int]


def _ch(c: ChannelLike) -> _lib.ChannelId:
    if isinstance(c, tuple):
        return _lib.ChannelId(c[0] & 0xFFFFFFFFFFFFFFFF, c[1] & 0xFFFFFFFFFFFFFFFF)
    return _lib.ChannelId(int(c) & 0xFFFFFFFFFFFFFFFF, 0)


@dataclass(frozen=True)
class CausalLogID:
    """CausalLogID.java:38-198: main-thread log or (partition, subpartition) log of a vertex."""
    vertex_id: int
    is_main: bool = True
    irp_lower: int = 0
    irp_upper: int = 0
    subpartition: int = 0

    @staticmethod
    def main(vertex_id: int) -> "CausalLogID":
        return CausalLogID(vertex_id, True)

    @staticmethod
    def sub(vertex_id: int, lower: int, upper: int, index: int) -> "CausalLogID":
        return CausalLogID(vertex_id, False, lower, upper, index)

    def key(self):
        """equals/hashCode semantics (:128-163): main logs compare by vertex only."""
        return (self.vertex_id, True) if self.is_main else (self.vertex_id, False, self.irp_lower, self.irp_upper,
                                                            self.subpartition)

    def to_c(self) -> _lib.CausalLogIdC:
        return _lib.CausalLogIdC(self.vertex_id, 1 if self.is_main else 0, 0 if self.is_main else self.subpartition, 0,
                                 0 if self.is_main else self.irp_lower, 0 if self.is_main else self.irp_upper)

    def is_for_vertex(self, v: int) -> bool:
        return self.vertex_id == v


class DecodedBatch:
    """Dense SoA produced by the GPU decode (layout: include/clonos_engine.h clg_decoded)."""

    def __init__(self, off, tag, v0, w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, span_rec_base, spans_bytes=None):
        self.off, self.tag, self.v0 = off, tag, v0
        self.w_idx, self.w_rc, self.w_v1 = w_idx, w_rc, w_v1
        self.w_var_off, self.w_var_len, self.w_sub = w_var_off, w_var_len, w_sub
        self.span_rec_base = span_rec_base
        self.spans_bytes = spans_bytes  # optional: the raw span bytes, to materialise var fields
        # optional: the packed payload column (clg_payloads.var); w_var_off then indexes it (DecodedColumns.to_soa)
        self.var = None

    @property
    def n_rec(self) -> int:
        return int(self.tag.shape[0])

    def span_slice(self, s: int) -> slice:
        return slice(int(self.span_rec_base[s]), int(self.span_rec_base[s + 1]))

    def determinants(self, s: int) -> List[D.Determinant]:
        """Rebuild Determinant objects for span s (LogReplayer consumption order)."""
        raw = self.var if self.var is not None else self.spans_bytes[s] if self.spans_bytes is not None else None
        sl = self.span_slice(s)
        widx = {int(i): k for k, i in enumerate(self.w_idx)}
        var = (lambda vo, vl: bytes(raw[vo:vo + vl])) if raw is not None else None
        return [self._determinant(i, widx.get(i), var) for i in range(sl.start, sl.stop)]

    def determinant_at(self, s: int, k: int, var=None) -> D.Determinant:
        """Record k of span s alone.  var(off, len) returns span-relative bytes of the span (a
        name, storage reference or java stream); None: from spans_bytes when the batch kept them."""
        i = int(self.span_rec_base[s]) + k
        if not 0 <= k < int(self.span_rec_base[s + 1]) - int(self.span_rec_base[s]):
            raise IndexError("record index outside the span")
        if var is None and (self.var is not None or self.spans_bytes is not None):
            raw = self.var if self.var is not None else self.spans_bytes[s]
            var = lambda vo, vl: bytes(raw[vo:vo + vl])
        w = int(np.searchsorted(self.w_idx, i))  # w_idx ascends: global record indices in record order
        return self._determinant(i, w if w < len(self.w_idx) and int(self.w_idx[w]) == i else None, var)

    def _determinant(self, i: int, k: Optional[int], var) -> D.Determinant:
        """Record i (global index); k: its side-table row when it is wide."""
        t = int(self.tag[i])
        v0 = int(self.v0[i])
        if t == D.ORDER:
            return D.OrderDeterminant(v0)
        if t == D.TIMESTAMP:
            return D.TimestampDeterminant(v0)
        if t == D.RNG:
            return D.RNGDeterminant(v0)
        if t == D.BUFFER_BUILT:
            return D.BufferBuiltDeterminant(v0)
        rc, v1, vo, vl, sub = (int(self.w_rc[k]), int(self.w_v1[k]), int(self.w_var_off[k]),
                               int(self.w_var_len[k]), int(self.w_sub[k]))
        # (span-relative offset 0 is the record's tag, never a payload; an offset into the packed
        # payload column may be 0)
        b = var(vo, vl) if var is not None and (vo or self.var is not None) else None
        if t == D.IGNORE_CHECKPOINT:
            return D.IgnoreCheckpointDeterminant(rc, v0)
        if t == D.TIMER_TRIGGER:
            return D.TimerTriggerDeterminant(rc, v0, sub, b if sub == D.INTERNAL else None)
        if t == D.SOURCE_CHECKPOINT:
            return D.SourceCheckpointDeterminant(rc, v0, v1, sub & 0x7F, b if sub & 0x80 else None)
        if t == D.SERIALIZABLE:
            return D.SerializableDeterminant(b if b is not None else b"")
        raise ValueError(f"tag {t} in a decoded batch")


def _wide_determinant(t: int, v0: int, rc: int, v1: int, vo: int, vl: int, sub: int, var) -> D.Determinant:
    """A wide record from its side row (DecodedBatch._determinant's rules)."""
    b = var(vo, vl) if var is not None and vo else None
    if t == D.IGNORE_CHECKPOINT:
        return D.IgnoreCheckpointDeterminant(rc, v0)
    if t == D.TIMER_TRIGGER:
        return D.TimerTriggerDeterminant(rc, v0, sub, b if sub == D.INTERNAL else None)
    if t == D.SOURCE_CHECKPOINT:
        return D.SourceCheckpointDeterminant(rc, v0, v1, sub & 0x7F, b if sub & 0x80 else None)
    if t == D.SERIALIZABLE:
        return D.SerializableDeterminant(b if b is not None else b"")
    raise ValueError(f"tag {t} in a decoded batch")


# tag -> column class (clg_columns): ORDER, TIMESTAMP, RNG, BUFFER_BUILT, WIDE; 5: no class
COL_CLASS_OF_TAG = np.array([0, 1, 2, 4, 4, 4, 4, 3] + [5] * 248, np.uint8)
_COL_FIELDS = (("tag", np.uint8), ("order", np.int8), ("timestamp", np.int64), ("rng", np.int32),
               ("buffer_built", np.int32), ("w_idx", np.uint32), ("w_rc", np.int32), ("w_v1", np.int64),
               ("w_var_off", np.uint32), ("w_var_len", np.uint32), ("w_sub", np.uint8), ("w_v0", np.int64))
_SOA_IN_FIELDS = (("tag", np.uint8), ("v0", np.int64), ("w_idx", np.uint32), ("w_rc", np.int32), ("w_v1", np.int64),
                  ("w_var_off", np.uint32), ("w_var_len", np.uint32), ("w_sub", np.uint8))  # (off is not read)
_COL_WIDE = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")
_COL_CAP = {"tag": "cap_tag", "order": "cap_order", "timestamp": "cap_timestamp", "rng": "cap_rng",
            "buffer_built": "cap_buffer_built"}


@dataclass
class SpanColumns:
    """One span's view of the columns: its tags (the interleaving) and its slice of each column;
    w0 is the span's first row in the batch's wide columns."""
    tag: np.ndarray
    order: np.ndarray
    timestamp: np.ndarray
    rng: np.ndarray
    buffer_built: np.ndarray
    w0: int
    n_wide: int


class DecodedColumns:
    """Typed replay columns (layout: include/clonos_engine.h clg_columns): tag in record order,
    one array per determinant class holding that class's values in record order, the wide rows,
    and span_base[(n_spans + 1), 5], the class counts before each span.  Record offsets are not
    part of the columns (use decode_logs for those)."""

    def __init__(self, tag, order, timestamp, rng, buffer_built, w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, w_v0,
                 span_base, spans_bytes=None):
        self.tag, self.order, self.timestamp, self.rng, self.buffer_built = tag, order, timestamp, rng, buffer_built
        self.w_idx, self.w_rc, self.w_v1, self.w_v0 = w_idx, w_rc, w_v1, w_v0
        self.w_var_off, self.w_var_len, self.w_sub = w_var_off, w_var_len, w_sub
        self.span_base = np.asarray(span_base, np.uint64).reshape(-1, _lib.COL_CLASSES)
        self.spans_bytes = spans_bytes
        # the payload column (clg_payloads; decode_logs_columns(..., payloads=True)): the wide rows'
        # payload bytes packed in row order and var_pos[n_wide + 1], row k's bytes at
        # var[var_pos[k]:var_pos[k + 1]]; None when not asked for
        self.var: Optional[np.ndarray] = None
        self.var_pos: Optional[np.ndarray] = None
        # a decode error the columns stop at (decode_logs_columns(..., partial=True)): a ClonosError, or None
        self.error: Optional[ClonosError] = None

    @property
    def n_rec(self) -> int:
        return int(self.tag.shape[0])

    @property
    def n_spans(self) -> int:
        return int(self.span_base.shape[0]) - 1

    @property
    def span_rec_base(self) -> np.ndarray:
        """Each span's first record index (the decode's span_rec_base): the row sums."""
        return self.span_base.sum(axis=1, dtype=np.uint64)

    @property
    def n_bytes(self) -> int:
        """The delivered size: every column, span_base and the payload column when present."""
        arrs = [getattr(self, k) for k, _ in _COL_FIELDS] + [self.span_base, self.var, self.var_pos]
        return int(sum(a.nbytes for a in arrs if a is not None))

    def span(self, s: int) -> SpanColumns:
        if not 0 <= s < self.n_spans:
            raise IndexError("span index")
        a, b = self.span_base[s].astype(np.int64), self.span_base[s + 1].astype(np.int64)
        r0, r1 = int(a.sum()), int(b.sum())
        return SpanColumns(self.tag[r0:r1], self.order[a[0]:b[0]], self.timestamp[a[1]:b[1]], self.rng[a[2]:b[2]],
                           self.buffer_built[a[3]:b[3]], int(a[4]), int(b[4] - a[4]))

    def payload(self, k: int) -> bytes:
        """Wide row k's payload bytes (a name, a storage reference, a java stream; b"" for a row
        without one), from the payload column."""
        if self.var is None or self.var_pos is None:
            raise ValueError("the columns carry no payload column (payloads=True)")
        if not 0 <= k < len(self.var_pos) - 1:
            raise IndexError("wide row index")
        return self.var[int(self.var_pos[k]):int(self.var_pos[k + 1])].tobytes()

    def to_soa(self) -> DecodedBatch:
        """The inverse: tag, v0 and the side table as the decode gives them (off is None).  With
        a payload column the batch carries it (DecodedBatch.var) and its w_var_off index it."""
        tag = np.asarray(self.tag)
        cls = COL_CLASS_OF_TAG[tag]
        v0 = np.zeros(tag.shape[0], np.int64)
        for c, col in enumerate((self.order, self.timestamp, self.rng, self.buffer_built, self.w_v0)):
            m = cls == c
            if int(m.sum()) != len(col):
                raise ValueError(f"class {c}: the tags ask for {int(m.sum())} values, the column holds {len(col)}")
            v0[m] = col
        if (cls == 5).any():
            raise ValueError("a tag above 7 in the columns")
        if self.var is not None:
            if len(self.var) >> 32:
                raise ValueError("the payload column does not fit u32 offsets")
            batch = DecodedBatch(None, tag.copy(), v0, self.w_idx, self.w_rc, self.w_v1,
                                 self.var_pos[:-1].astype(np.uint32), self.w_var_len, self.w_sub, self.span_rec_base,
                                 self.spans_bytes)
            batch.var = self.var
            return batch
        return DecodedBatch(None, tag.copy(), v0, self.w_idx, self.w_rc, self.w_v1, self.w_var_off, self.w_var_len,
                            self.w_sub, self.span_rec_base, self.spans_bytes)

    def determinants(self, s: int, var=None) -> List[D.Determinant]:
        """The Determinant objects of span s, as DecodedBatch.determinants builds them.
        var(off, len): span-relative bytes (names, references, java streams); None: from
        spans_bytes when the columns kept them.  The payload column, when present, comes first."""
        packed = var is None and self.var is not None
        if var is None and not packed and self.spans_bytes is not None:
            raw = self.spans_bytes[s]
            var = lambda vo, vl: bytes(raw[vo:vo + vl])
        sp = self.span(s)
        at = [0, 0, 0, 0, sp.w0]
        out = []
        for t in sp.tag.tolist():
            c = int(COL_CLASS_OF_TAG[t])
            k = at[c]
            at[c] += 1
            if c == 0:
                out.append(D.OrderDeterminant(int(sp.order[k])))
            elif c == 1:
                out.append(D.TimestampDeterminant(int(sp.timestamp[k])))
            elif c == 2:
                out.append(D.RNGDeterminant(int(sp.rng[k])))
            elif c == 3:
                out.append(D.BufferBuiltDeterminant(int(sp.buffer_built[k])))
            else:
                v = (lambda vo, vl, _k=k: self.payload(_k)) if packed else var
                out.append(_wide_determinant(t, int(self.w_v0[k]), int(self.w_rc[k]), int(self.w_v1[k]),
                                             int(self.w_var_off[k]), int(self.w_var_len[k]), int(self.w_sub[k]), v))
        return out


def _columns_struct(arrs: dict, base: Optional[np.ndarray], kind: int) -> _lib.Columns:
    """clg_columns over host arrays (arrs: name -> array, capacity = its length)."""
    c = _lib.Columns()
    for name, _ in _COL_FIELDS:
        setattr(c, name, _np_ptr(arrs[name]) or None)
    for name, cap in _COL_CAP.items():
        setattr(c, cap, arrs[name].size)
    c.cap_wide = min(arrs[k].size for k in _COL_WIDE)
    c.span_base = _np_ptr(base) if base is not None else None
    c.out_kind = kind
    return c


def _columns_result(c: _lib.Columns, arrs: dict, base: np.ndarray, spans_bytes=None) -> DecodedColumns:
    n = [int(x) for x in c.n_class]
    cnt = {"tag": int(c.n_rec), "order": n[0], "timestamp": n[1], "rng": n[2], "buffer_built": n[3]}
    return DecodedColumns(*[arrs[k][:cnt.get(k, n[4])] for k, _ in _COL_FIELDS], base, spans_bytes)


def _columns_error(st: int, c: _lib.Columns) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.err_span, err.err_off, err.err_tag, err.n_rec = c.err_span, c.err_off, c.err_tag, c.n_rec
    err.n_class = [int(x) for x in c.n_class]
    return err


def _host_columns(n: int, n_class: Sequence[int]) -> dict:
    cnt = {"tag": n, "order": n_class[0], "timestamp": n_class[1], "rng": n_class[2], "buffer_built": n_class[3]}
    return {k: np.zeros(cnt.get(k, n_class[4]), dt) for k, dt in _COL_FIELDS}


def columnize_host(batch: DecodedBatch) -> DecodedColumns:
    """clg_columnize_host: the typed columns of a decoded batch on the CPU in one pass (no engine,
    no GPU) -- what Engine.columnize computes on the device."""
    d = _lib.Decoded()
    keep = []
    for name, dt in _SOA_IN_FIELDS:
        a =np.ascontiguousarray(getattr(batch, name), dt)
        keep.append(a)
        setattr(d, name, _np_ptr(a) or None)
    d.n_rec, d.n_wide = batch.n_rec, len(batch.w_idx)
    srb = np.ascontiguousarray(batch.span_rec_base, np.uint64)
    n_spans = max(len(srb) - 1, 0)
    base = np.zeros((n_spans + 1) * _lib.COL_CLASSES, np.uint64)
    c = _lib.Columns()  # every column pointer null: sizes only
    c.span_base = _np_ptr(base)
    st = lib.clg_columnize_host(C.byref(d), _np_ptr(srb), n_spans, C.byref(c))
    if st != _lib.CLG_OK:
        raise _columns_error(st, c)
    arrs = _host_columns(int(c.n_rec), [int(x) for x in c.n_class])
    c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
    st = lib.clg_columnize_host(C.byref(d), _np_ptr(srb), n_spans, C.byref(c))
    if st != _lib.CLG_OK:
        raise _columns_error(st, c)
    return _columns_result(c, arrs, base, batch.spans_bytes)


def _payloads_struct(var: Optional[np.ndarray], pos: Optional[np.ndarray], kind: int = _lib.CLG_MEM_HOST) -> _lib.Payloads:
    """clg_payloads over host arrays (capacity = their lengths); both None: sizes only."""
    p = _lib.Payloads()
    p.var = (_np_ptr(var) or None) if var is not None else None
    p.pos = (_np_ptr(pos) or None) if pos is not None else None
    p.cap_var = var.size if var is not None else 0
    p.cap_pos = pos.size if pos is not None else 0
    p.out_kind = kind
    return p


def _payloads_error(st: int, p: _lib.Payloads) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.n_rows, err.n_var, err.bad_row = int(p.n_rows), int(p.n_var), int(p.bad_row)
    return err


def _payloads_twice(call) -> Tuple[np.ndarray, np.ndarray]:
    """call(clg_payloads) -> status, first for the sizes, then into host arrays of exactly those."""
    p = _lib.Payloads()
    st = call(p)
    if st != _lib.CLG_OK:
        raise _payloads_error(st, p)
    var, pos = np.zeros(int(p.n_var), np.uint8), np.zeros(int(p.n_rows) + 1, np.uint64)
    p = _payloads_struct(var, pos)
    st = call(p)
    if st != _lib.CLG_OK:
        raise _payloads_error(st, p)
    return var, pos


def gather_payloads_host(data: Union[bytes, np.ndarray], span_off, span_len, w_var_off, w_var_len, row_base
                         ) -> Tuple[np.ndarray, np.ndarray]:
    """clg_gather_payloads_host: the payload column of spans data[span_off[s] : + span_len[s]] on
    the CPU (no engine, no GPU).  Rows w_var_off / w_var_len are span-relative; row k belongs to
    span s when row_base[s] <= k < row_base[s + 1].  Returns (var u8[n_var], pos u64[n_rows + 1])."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    so, sl = np.ascontiguousarray(span_off, np.uint64), np.ascontiguousarray(span_len, np.uint64)
    wo, wl = np.ascontiguousarray(w_var_off, np.uint32), np.ascontiguousarray(w_var_len, np.uint32)
    rb = np.ascontiguousarray(row_base, np.uint64)
    return _payloads_twice(lambda p: lib.clg_gather_payloads_host(_np_ptr(buf), _np_ptr(so), _np_ptr(sl), so.size,
                                                                  _np_ptr(wo), _np_ptr(wl), _np_ptr(rb), C.byref(p)))


# clg_columns_in's arrays that come from DecodedColumns fields of the same name
_ECOL_FIELDS = (("tag", np.uint8), ("order", np.int8), ("timestamp", np.int64), ("rng", np.int32),
                ("buffer_built", np.int32), ("w_rc", np.int32), ("w_v1", np.int64), ("w_var_len", np.uint32),
                ("w_sub", np.uint8), ("w_v0", np.int64))


def _columns_in(cols: Union["DecodedColumns", "PackedColumns"], check_idx: bool = True) -> Tuple[_lib.ColumnsIn, list]:
    """clg_columns_in over cols' host arrays and its payload column; the second value keeps the
    arrays alive.  For a PackedColumns the five narrow pointers stay null (they are given packed)
    and the totals are n_val's.  Columns without a payload column raise ValueError."""
    if cols.var is None or cols.var_pos is None:
        raise ValueError("the columns carry no payload column (payloads=True)")
    packed = isinstance(cols, PackedColumns)
    cin = _lib.ColumnsIn()
    keep = []
    for name, dt in _ECOL_FIELDS[5 if packed else 0:]:
        a = np.ascontiguousarray(getattr(cols, name), dt)
        keep.append(a)
        setattr(cin, name, _np_ptr(a) or None)
    if check_idx and cols.w_idx is not None:
        a = np.ascontiguousarray(cols.w_idx, np.uint32)
        keep.append(a)
        cin.w_idx = _np_ptr(a) or None
    pos, var = np.ascontiguousarray(cols.var_pos, np.uint64), np.ascontiguousarray(cols.var, np.uint8)
    keep += [pos, var]
    cin.pos, cin.var, cin.n_var = _np_ptr(pos) or None, _np_ptr(var) or None, var.size
    cin.n_rec = cols.n_rec
    for c, name in enumerate(("order", "timestamp", "rng", "buffer_built")):
        cin.n_class[c] = cols.n_val[c + 1] if packed else len(getattr(cols, name))
    cin.n_class[4] = len(cols.w_v0)
    if cols.n_spans:
        sb = np.ascontiguousarray(cols.span_base, np.uint64).reshape(-1)
        keep.append(sb)
        cin.span_base, cin.n_spans = _np_ptr(sb), cols.n_spans
    cin.in_kind = _lib.CLG_MEM_HOST
    return cin, keep


def _encoded_error(st: int, enc: _lib.Encoded) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.n_bytes, err.bad_what, err.bad_index = int(enc.n_bytes), int(enc.bad_what), int(enc.bad_index)
    return err


def _encode_twice(call, n_spans: int, per_span: bool):
    """call(clg_encoded) -> status, first for the sizes, then into a host buffer of exactly those."""
    sbb = np.zeros(max(n_spans, 1) + 1, np.uint64)
    enc = _lib.Encoded()
    enc.span_byte_base, enc.out_kind = _np_ptr(sbb), _lib.CLG_MEM_HOST
    st = call(enc)
    if st != _lib.CLG_OK:
        raise _encoded_error(st, enc)
    out = np.empty(max(1, int(enc.n_bytes)), np.uint8)
    enc.bytes, enc.cap = _np_ptr(out), out.size
    st = call(enc)
    if st != _lib.CLG_OK:
        raise _encoded_error(st, enc)
    n = int(enc.n_bytes)
    if not per_span:
        return out[:n].tobytes()
    return [out[int(sbb[s]):int(sbb[s + 1])].tobytes() for s in range(max(n_spans, 1))]


def encode_columns_host(cols: "DecodedColumns", per_span: bool = False):
    """clg_encode_columns_host: the log bytes of typed columns that carry their payload column, on
    the CPU (no engine, no GPU) -- what Engine.encode_columns computes on the device.  per_span: one
    bytes per span instead of the whole stream."""
    cin, keep = _columns_in(cols)
    return _encode_twice(lambda enc: lib.clg_encode_columns_host(C.byref(cin), C.byref(enc)), cols.n_spans, per_span)


# clg_pack_block rows
PACK_BLOCK = np.dtype([("ref", np.int64), ("first", np.int64), ("pos", np.uint64), ("width", np.uint32),
                       ("count", np.uint32)])
# the packed streams' element types, in stream order (the clg_columns arrays of the same names)
PACK_STREAM_FIELDS = (("tag", np.uint8), ("order", np.int8), ("timestamp", np.int64), ("rng", np.int32),
                      ("buffer_built", np.int32))


# The two packed families (clg_packed: _lib.Packed, clg_packed_wide: _lib.PackedWideC) share their
# first six fields and n_val / blk_base / n_bits; the helpers below serve both, told apart by the
# struct class (its n_val holds one entry per stream).
def _packed_over(cls, desc: Optional[np.ndarray], bits: Optional[np.ndarray], kind: int = _lib.CLG_MEM_HOST):
    """A cls struct over host arrays (capacity = their lengths); both None: sizes only."""
    p = cls()
    if desc is not None:
        p.desc, p.cap_desc = _np_ptr(desc), desc.size
    if bits is not None:
        p.bits, p.cap_bits = _np_ptr(bits), bits.size
    p.out_kind = kind
    return p


def _packed_of(cls, obj):
    """A cls struct over a PackedColumns' or PackedWide's arrays, with its n_val, blk_base and n_bits."""
    p = _packed_over(cls, obj.desc, obj.bits)
    p.n_val[:], p.blk_base[:], p.n_bits = obj.n_val, obj.blk_base, obj.bits.size
    return p


def _packed_error(st: int, p) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.n_blocks, err.n_bits = int(p.blk_base[len(p.n_val)]), int(p.n_bits)
    if isinstance(p, _lib.PackedWideC):
        err.bad_row = int(p.bad_row)
    return err


def _pack_twice(cls, call):
    """call(cls struct) -> status, first for the sizes, then into host arrays of exactly those:
    the filled struct and its desc and bits."""
    p = cls()
    st = call(p)
    if st != _lib.CLG_OK:
        raise _packed_error(st, p)
    desc, bits = np.zeros(int(p.blk_base[len(p.n_val)]), PACK_BLOCK), np.zeros(int(p.n_bits), np.uint8)
    p = _packed_over(cls, desc, bits)
    st = call(p)
    if st != _lib.CLG_OK:
        raise _packed_error(st, p)
    return p, desc, bits


def _packed_struct(desc: Optional[np.ndarray], bits: Optional[np.ndarray], kind: int = _lib.CLG_MEM_HOST) -> _lib.Packed:
    """clg_packed over host arrays (capacity = their lengths); both None: sizes only."""
    return _packed_over(_lib.Packed, desc, bits, kind)


class PackedColumns:
    """Typed replay columns with the five narrow columns bit-packed (layout: include/clonos_engine.h
    clg_packed; the format: clonos_amd/csrc/pack.h): desc, one PACK_BLOCK row per block of 1024
    values, stream c's rows at desc[blk_base[c]:blk_base[c + 1]], and bits, the blocks' payloads.
    The wide rows, span_base and the payload column are as DecodedColumns holds them.  span(s)
    unpacks only the blocks span s's ranges cover, so replay.ColumnReplayer(packed, s) works as it
    does over DecodedColumns; unpack() gives the whole DecodedColumns back.

    wide_packed (decode_logs_columns(..., packed=True, pack_wide=True)): the wide rows came packed
    too, as a PackedWide, and the payload column without var_pos.  The seven w_* arrays and var_pos
    are then not held: the first read of any of them unpacks the rows once through
    clg_unpack_wide_host and rebuilds var_pos as the prefix sum of w_var_len, so unpack(), span(),
    payload() and the encode and append of these columns work as they do over delivered rows."""

    def __init__(self, desc, bits, n_val, blk_base, w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, w_v0, span_base,
                 spans_bytes=None, wide_packed: Optional["PackedWide"] = None):
        self.desc, self.bits = desc, bits
        self.n_val = [int(x) for x in n_val]
        self.blk_base = [int(x) for x in blk_base]
        self.wide_packed = wide_packed
        if wide_packed is None:
            self.w_idx, self.w_rc, self.w_v1, self.w_v0 = w_idx, w_rc, w_v1, w_v0
            self.w_var_off, self.w_var_len, self.w_sub = w_var_off, w_var_len, w_sub
            self.var_pos: Optional[np.ndarray] = None
        self.span_base = np.asarray(span_base, np.uint64).reshape(-1, _lib.COL_CLASSES)
        self.spans_bytes = spans_bytes
        self.var: Optional[np.ndarray] = None
        self.error: Optional[ClonosError] = None

    def _wide(self) -> dict:
        """The seven w_* arrays of wide_packed columns, unpacked once (clg_unpack_wide_host) and kept."""
        d = self.__dict__
        if "w_idx" not in d:
            d.update(self.wide_packed.unpack())
        return {k: d[k] for k in _COL_WIDE}

    def __getattr__(self, name):
        # Reached only for a name the instance does not hold, which for wide_packed columns are the
        # w_* arrays and var_pos: ColumnReplayer and _columns_in read them as attributes, as they do
        # on DecodedColumns.  The rows are kept once unpacked; var_pos is kept only once there is a
        # payload column to index (var may be attached after construction).
        d = self.__dict__
        if d.get("wide_packed") is None or (name not in _COL_WIDE and name != "var_pos"):
            raise AttributeError(name)
        wide = self._wide()
        if name != "var_pos":
            return wide[name]
        if d.get("var") is None:
            return None
        pos = np.zeros(self.wide_packed.n_wide + 1, np.uint64)
        np.cumsum(wide["w_var_len"], dtype=np.uint64, out=pos[1:])
        d["var_pos"] = pos
        return pos

    @property
    def n_rec(self) -> int:
        return self.n_val[_lib.PACK_TAG]

    @property
    def n_spans(self) -> int:
        return int(self.span_base.shape[0]) - 1

    @property
    def n_bytes(self) -> int:
        """The delivered size: descriptors, payload bits, the wide rows, span_base and the
        payload column when present."""
        arrs = [self.desc, self.bits, self.span_base, self.var]
        if self.wide_packed is not None:  # (the rows and var_pos, once unpacked, were not delivered)
            return int(sum(a.nbytes for a in arrs if a is not None)) + self.wide_packed.n_bytes
        arrs += [self.var_pos] + [getattr(self, k) for k in _COL_WIDE]
        return int(sum(a.nbytes for a in arrs if a is not None))

    def _struct(self) -> _lib.Packed:
        return _packed_of(_lib.Packed, self)

    def unpack_stream(self, stream: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """clg_unpack_columns_host: values [first, first + count) of one stream, in its own type;
        only the blocks that range covers are read."""
        if not 0 <= stream < _lib.PACK_STREAMS:
            raise IndexError("stream index")
        if count is None:
            count = self.n_val[stream] - first
        out = np.empty(max(count, 0), PACK_STREAM_FIELDS[stream][1])
        p = self._struct()
        st = lib.clg_unpack_columns_host(C.byref(p), stream, first, count, _np_ptr(out) or None)
        if st != _lib.CLG_OK:
            raise _packed_error(st, p)
        return out

    def unpack(self) -> "DecodedColumns":
        cols = DecodedColumns(*[self.unpack_stream(c) for c in range(_lib.PACK_STREAMS)],
                              *[getattr(self, k) for k in _COL_WIDE], self.span_base, self.spans_bytes)
        cols.var, cols.var_pos, cols.error = self.var, self.var_pos, self.error
        return cols

    def span(self, s: int) -> SpanColumns:
        if not 0 <= s < self.n_spans:
            raise IndexError("span index")
        a, b = self.span_base[s].astype(np.int64), self.span_base[s + 1].astype(np.int64)
        r0, r1 = int(a.sum()), int(b.sum())
        cut = [(r0, r1)] + [(int(a[c]), int(b[c])) for c in range(4)]
        return SpanColumns(*[self.unpack_stream(c, lo, hi - lo) for c, (lo, hi) in enumerate(cut)], int(a[4]),
                           int(b[4] - a[4]))

    def payload(self, k: int) -> bytes:
        if self.var is None or self.var_pos is None:
            raise ValueError("the columns carry no payload column (payloads=True)")
        if not 0 <= k < len(self.var_pos) - 1:
            raise IndexError("wide row index")
        return self.var[int(self.var_pos[k]):int(self.var_pos[k + 1])].tobytes()


def _pack_in(cols: "DecodedColumns") -> Tuple[_lib.Columns, list]:
    """clg_columns over cols' five narrow host arrays, as the pack reads them."""
    c = _lib.Columns()
    keep = []
    for name, dt in PACK_STREAM_FIELDS:
        a = np.ascontiguousarray(getattr(cols, name), dt)
        keep.append(a)
        setattr(c, name, _np_ptr(a) or None)
    c.n_rec = keep[0].size
    for k in range(4):
        c.n_class[k] = keep[k + 1].size
    c.n_class[4] = len(cols.w_v0)
    c.out_kind = _lib.CLG_MEM_HOST
    return c, keep


def _pack_narrow(call, cols: "DecodedColumns") -> PackedColumns:
    """_pack_twice over a clg_packed; what is not packed is passed through from cols."""
    p, desc, bits = _pack_twice(_lib.Packed, call)
    out = PackedColumns(desc, bits, p.n_val, p.blk_base, *[getattr(cols, k) for k in _COL_WIDE], cols.span_base,
                        cols.spans_bytes)
    out.var, out.var_pos, out.error = cols.var, cols.var_pos, cols.error
    return out


def pack_columns_host(cols: "DecodedColumns") -> PackedColumns:
    """clg_pack_columns_host: the five narrow columns bit-packed on the CPU (no engine, no GPU) --
    the same bytes Engine.pack_columns produces on the device."""
    cin, keep = _pack_in(cols)
    return _pack_narrow(lambda p: lib.clg_pack_columns_host(C.byref(cin), C.byref(p)), cols)


def unpack_columns_host(packed: PackedColumns, stream: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
    """clg_unpack_columns_host (PackedColumns.unpack_stream)."""
    return packed.unpack_stream(stream, first, count)


def _unpack_error(st: int, bad: _lib.UnpackBad, enc: Optional[_lib.Encoded] = None) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.bad_what, err.bad_stream, err.bad_block = int(bad.what), int(bad.stream), int(bad.block)
    if enc is not None:
        err.n_bytes, err.enc_bad_what, err.bad_index = int(enc.n_bytes), int(enc.bad_what), int(enc.bad_index)
    return err


def _unpack_out(n_val: Sequence[int]) -> Tuple[_lib.Columns, list]:
    """clg_columns over fresh host arrays of exactly the streams' lengths."""
    c = _lib.Columns()
    arrs = []
    for (name, dt), n in zip(PACK_STREAM_FIELDS, n_val):
        a = np.empty(int(n), dt)
        arrs.append(a)
        setattr(c, name, _np_ptr(a) or None)
        setattr(c, _COL_CAP[name], a.size)
    c.out_kind = _lib.CLG_MEM_HOST
    return c, arrs


def _unpacked(packed: "PackedColumns", arrs: list) -> "DecodedColumns":
    cols = DecodedColumns(*arrs, *[getattr(packed, k) for k in _COL_WIDE], packed.span_base, packed.spans_bytes)
    cols.var, cols.var_pos, cols.error = packed.var, packed.var_pos, packed.error
    return cols


def unpack_packed_host(packed: "PackedColumns") -> "DecodedColumns":
    """clg_unpack_columns_all_host: the whole unpack on the CPU under the device unpack's rules (no
    engine, no GPU) -- what Engine.unpack_columns computes.  Invalid input raises ClonosError with
    bad_what, bad_stream and bad_block."""
    p = packed._struct()
    c, arrs = _unpack_out(packed.n_val)
    bad = _lib.UnpackBad()
    st = lib.clg_unpack_columns_all_host(C.byref(p), C.byref(c), C.byref(bad))
    if st != _lib.CLG_OK:
        raise _unpack_error(st, bad)
    return _unpacked(packed, arrs)


# the packed wide rows' six fields, in the format's order (clg_packed_wide, pack_wide.h)
WPACK_FIELDS = (("w_rc", np.int32), ("w_v1", np.int64), ("w_var_off", np.uint32), ("w_var_len", np.uint32),
                ("w_sub", np.uint8), ("w_v0", np.int64))


def _packed_wide_struct(desc: Optional[np.ndarray], bits: Optional[np.ndarray],
                        kind: int = _lib.CLG_MEM_HOST) -> _lib.PackedWideC:
    """clg_packed_wide over host arrays (capacity = their lengths); both None: sizes only."""
    return _packed_over(_lib.PackedWideC, desc, bits, kind)


class PackedWide:
    """The wide rows partitioned by record kind and bit-packed (layout: include/clonos_engine.h
    clg_packed_wide; the format: clonos_amd/csrc/pack_wide.h): desc, one PACK_BLOCK row per block of
    1024 values, stream c's rows at desc[blk_base[c]:blk_base[c + 1]], and bits, the blocks'
    payloads.  unpack() gives the seven w_* arrays back in row order; rows(kind) the rows of one
    kind."""

    def __init__(self, desc, bits, n_val, blk_base):
        self.desc, self.bits = desc, bits
        self.n_val = [int(x) for x in n_val]
        self.blk_base = [int(x) for x in blk_base]

    @property
    def n_wide(self) -> int:
        return self.n_val[_lib.WPACK_KIND]

    @property
    def n_bytes(self) -> int:
        """The delivered size: descriptors and payload bits."""
        return int(self.desc.nbytes + self.bits.nbytes)

    def _struct(self) -> _lib.PackedWideC:
        return _packed_of(_lib.PackedWideC, self)

    def unpack(self) -> dict:
        """clg_unpack_wide_host: the seven w_* arrays by name, in row order.  Invalid input raises
        ClonosError with bad_what, bad_stream and bad_block."""
        return unpack_wide_host(self)

    def kinds(self) -> np.ndarray:
        """The kind (tag - 3) of every row: stream 0, read from its blocks (unpack() validates)."""
        return _unpack_wide_kinds(self, np.empty(self.n_wide, np.uint8))

    def rows(self, kind: int) -> dict:
        """The rows of one kind (0 SERIALIZABLE .. 3 IGNORE_CHECKPOINT), the seven arrays by name."""
        if not 0 <= kind < _lib.WPACK_KINDS:
            raise IndexError("kind")
        w = self.unpack()
        sel = self.kinds() == kind
        return {k: v[sel] for k, v in w.items()}


def _unpack_wide_kinds(packed: "PackedWide", out: np.ndarray) -> np.ndarray:
    # stream 0 is u8 FOR: its values are ref + the payload's width-bit fields
    at = 0
    for b in packed.desc[packed.blk_base[0]:packed.blk_base[1]]:
        n, w = int(b["count"]), int(b["width"])
        if w == 0:
            out[at:at + n] = int(b["ref"])
        else:
            raw = packed.bits[int(b["pos"]):int(b["pos"]) + 16 * ((n * w + 127) // 128)]
            bits = np.unpackbits(raw, bitorder="little")[:n * w].reshape(n, w)
            out[at:at + n] = int(b["ref"]) + (bits << np.arange(w, dtype=np.uint8)).sum(axis=1)
        at += n
    return out


def _pack_wide_in(cols: "DecodedColumns") -> Tuple[_lib.Columns, list]:
    """clg_columns over cols' tags and seven wide host arrays, as the wide pack reads them."""
    c = _lib.Columns()
    keep = [np.ascontiguousarray(cols.tag, np.uint8)]
    c.tag = _np_ptr(keep[0]) or None
    for name, dt in _COL_FIELDS[5:]:
        a = np.ascontiguousarray(getattr(cols, name), dt)
        keep.append(a)
        setattr(c, name, _np_ptr(a) or None)
    c.n_rec = keep[0].size
    c.n_class[4] = keep[1].size
    c.out_kind = _lib.CLG_MEM_HOST
    return c, keep


def _pack_wide(call) -> PackedWide:
    """_pack_twice over a clg_packed_wide."""
    p, desc, bits = _pack_twice(_lib.PackedWideC, call)
    return PackedWide(desc, bits, p.n_val, p.blk_base)


def pack_wide_host(cols: "DecodedColumns") -> PackedWide:
    """clg_pack_wide_host: the wide rows partitioned by kind and bit-packed on the CPU (no engine,
    no GPU) -- the same bytes Engine.pack_wide produces on the device.  A row that is no wide
    record's raises ClonosError with bad_row."""
    cin, keep = _pack_wide_in(cols)
    return _pack_wide(lambda p: lib.clg_pack_wide_host(C.byref(cin), C.byref(p)))


def unpack_wide_host(packed: PackedWide) -> dict:
    """clg_unpack_wide_host: the seven w_* arrays of packed wide rows, by name, in row order.
    Invalid input raises ClonosError with bad_what, bad_stream and bad_block."""
    p = packed._struct()
    c = _lib.Columns()
    st = lib.clg_unpack_wide_host(C.byref(p), C.byref(c), None)  # the layout check and the rows
    bad = _lib.UnpackBad()
    arrs = {}
    if st == _lib.CLG_OK:
        for name, dt in _COL_FIELDS[5:]:
            arrs[name] = np.empty(int(c.n_class[4]), dt)
            setattr(c, name, _np_ptr(arrs[name]) or None)
        c.cap_wide = int(c.n_class[4])
    st = lib.clg_unpack_wide_host(C.byref(p), C.byref(c), C.byref(bad))
    if st != _lib.CLG_OK:
        raise _unpack_error(st, bad)
    return arrs


class PackedPayloads:
    """The payload column front-coded against same-length anchor rows (layout: include/clonos_engine.h
    clg_packed_payloads; the format: clonos_amd/csrc/ppay.h): desc and bits, the rows' lcps as one
    FOR stream of PACK_BLOCK blocks, and tail, the bytes behind each row's lcp, in row order.  The
    lengths are not part of it: unpack(pos) takes the column's pos."""

    def __init__(self, desc, bits, tail, n_rows, n_var):
        self.desc, self.bits, self.tail = desc, bits, tail
        self.n_rows, self.n_var = int(n_rows), int(n_var)

    @property
    def n_bytes(self) -> int:
        """The delivered size: descriptors, payload bits and tails."""
        return int(self.desc.nbytes + self.bits.nbytes + self.tail.nbytes)

    def _struct(self) -> _lib.PackedPayloadsC:
        p = _packed_payloads_struct(self.desc, self.bits, self.tail)
        p.n_rows, p.n_var, p.n_bits, p.n_tail = self.n_rows, self.n_var, self.bits.size, self.tail.size
        return p

    def unpack(self, pos) -> np.ndarray:
        """clg_unpack_payloads_host: var of the column whose pos is given.  Invalid input raises
        ClonosError with bad_what, bad_stream and bad_block."""
        return unpack_payloads_host(self, pos)


def _packed_payloads_struct(desc: Optional[np.ndarray], bits: Optional[np.ndarray], tail: Optional[np.ndarray],
                            kind: int = _lib.CLG_MEM_HOST) -> _lib.PackedPayloadsC:
    """clg_packed_payloads over host arrays (capacity = their lengths); all None: sizes only."""
    p = _lib.PackedPayloadsC()
    if desc is not None:
        p.desc, p.cap_desc = _np_ptr(desc), desc.size
    if bits is not None:
        p.bits, p.cap_bits = _np_ptr(bits), bits.size
    if tail is not None:
        p.tail, p.cap_tail = _np_ptr(tail), tail.size
    p.out_kind = kind
    return p


def _packed_payloads_error(st: int, p: _lib.PackedPayloadsC) -> ClonosError:
    err = ClonosError(st, lib.clg_last_error().decode(errors="replace"))
    err.n_rows, err.n_var, err.n_bits, err.n_tail = int(p.n_rows), int(p.n_var), int(p.n_bits), int(p.n_tail)
    err.bad_row = int(p.bad_row)
    return err


def _pack_payloads_twice(call) -> PackedPayloads:
    """call(clg_packed_payloads) -> status, first for the sizes, then into host arrays of exactly those."""
    p = _lib.PackedPayloadsC()
    st = call(p)
    if st != _lib.CLG_OK:
        raise _packed_payloads_error(st, p)
    desc = np.zeros((int(p.n_rows) + _lib.PACK_BLOCK - 1) // _lib.PACK_BLOCK, PACK_BLOCK)
    bits, tail = np.zeros(int(p.n_bits), np.uint8), np.zeros(int(p.n_tail), np.uint8)
    if int(p.n_rows) == 0:  # (every pointer would be null: the sizes-only call again)
        return PackedPayloads(desc, bits, tail, 0, 0)
    # (arrays without bytes still need an address: a null one of three is an array that holds nothing)
    keep = [a if a.size else np.zeros(1, a.dtype) for a in (desc, bits, tail)]
    p = _packed_payloads_struct(*keep)
    p.cap_desc, p.cap_bits, p.cap_tail = desc.size, bits.size, tail.size
    st = call(p)
    if st != _lib.CLG_OK:
        raise _packed_payloads_error(st, p)
    return PackedPayloads(desc, bits, tail, p.n_rows, p.n_var)


def _payload_column(var, pos) -> Tuple[np.ndarray, np.ndarray]:
    buf = np.frombuffer(bytes(var), np.uint8) if not isinstance(var, np.ndarray) else np.ascontiguousarray(var, np.uint8)
    pos = np.ascontiguousarray(pos, np.uint64)
    if pos.size == 0:
        raise ValueError("pos holds n_rows + 1 entries")
    return buf, pos


def pack_payloads_host(var, pos) -> PackedPayloads:
    """clg_pack_payloads_host: the payload column (var, pos) front-coded on the CPU (no engine, no
    GPU) -- the same bytes Engine.pack_payloads produces on the device.  A pos that is no prefix
    sum of row lengths below 2^32 raises ClonosError with bad_row."""
    buf, pos = _payload_column(var, pos)
    return _pack_payloads_twice(lambda p: lib.clg_pack_payloads_host(_np_ptr(buf) or None, _np_ptr(pos), pos.size - 1, C.byref(p)))


def _unpack_payloads(call, packed: PackedPayloads) -> np.ndarray:
    """call(clg_packed_payloads, clg_payloads, clg_unpack_bad) -> status, into a host var of n_var bytes."""
    p = packed._struct()
    var = np.empty(max(packed.n_var, 1), np.uint8)  # (one spare byte: a null var is the sizes-only call)
    out = _payloads_struct(var, None)
    out.cap_var = packed.n_var
    bad = _lib.UnpackBad()
    st = call(p, out, bad)
    if st != _lib.CLG_OK:
        raise _unpack_error(st, bad)
    return var[:packed.n_var]


def unpack_payloads_host(packed: PackedPayloads, pos) -> np.ndarray:
    """clg_unpack_payloads_host: var of a packed payload column whose pos is given, on the CPU.
    Invalid input raises ClonosError with bad_what, bad_stream (PPAY_STREAM) and bad_block."""
    pos = np.ascontiguousarray(pos, np.uint64)
    return _unpack_payloads(lambda p, out, bad: lib.clg_unpack_payloads_host(C.byref(p), _np_ptr(pos) or None, C.byref(out),
                                                                             C.byref(bad)), packed)


def _wide_route(cols, wide: str) -> bool:
    """Whether cols take the device route of the wide rows (clg_*_columns_packed_wide)."""
    if wide not in ("host", "device"):
        raise ValueError(f"wide={wide!r}: 'host' or 'device'")
    if wide == "device" and (not isinstance(cols, PackedColumns) or cols.wide_packed is None):
        raise ValueError("wide='device' takes PackedColumns whose wide rows came packed (wide_packed)")
    return wide == "device"


def _rest_in(cols: "PackedColumns") -> Tuple[_lib.ColumnsIn, list]:
    """clg_columns_in for the calls that take both packed forms: the payload bytes, the span bases
    and the totals.  No w_* array and no var_pos is read, so nothing is unpacked on the host."""
    if cols.var is None:
        raise ValueError("the columns carry no payload column (payloads=True)")
    cin = _lib.ColumnsIn()
    var = np.ascontiguousarray(cols.var, np.uint8)
    keep = [var]
    cin.var, cin.n_var = _np_ptr(var) or None, var.size
    cin.n_rec = cols.n_rec
    for c in range(4):
        cin.n_class[c] = cols.n_val[c + 1]
    cin.n_class[4] = cols.wide_packed.n_wide
    if cols.n_spans:
        sb = np.ascontiguousarray(cols.span_base, np.uint64).reshape(-1)
        keep.append(sb)
        cin.span_base, cin.n_spans = _np_ptr(sb), cols.n_spans
    cin.in_kind = _lib.CLG_MEM_HOST
    return cin, keep


def _encode_packed_wide(call, cols: "PackedColumns", per_span: bool):
    """_encode_twice over call(narrow, wide, rest, enc, bad) -> status, one of the two encodes that
    take both packed forms."""
    pk, pw, (rest, keep), bad = cols._struct(), cols.wide_packed._struct(), _rest_in(cols), _lib.UnpackBad()

    def twice(enc):
        st = call(C.byref(pk), C.byref(pw), C.byref(rest), C.byref(enc), C.byref(bad))
        if st != _lib.CLG_OK and bad.what != _lib.UNPACK_BAD_NONE:
            raise _unpack_error(st, bad, enc)
        return st
    return _encode_twice(twice, cols.n_spans, per_span)


def encode_columns_packed_wide_host(cols: "PackedColumns", per_span: bool = False):
    """clg_encode_columns_packed_wide_host: the log bytes of columns whose narrow columns and wide
    rows are both packed, on the CPU (no engine, no GPU) -- what Engine.encode_columns(cols,
    wide="device") computes.  A bad packed input raises ClonosError with bad_what, bad_stream
    (UNPACK_WIDE_STREAM + the stream for the wide rows) and bad_block."""
    _wide_route(cols, "device")
    return _encode_packed_wide(lib.clg_encode_columns_packed_wide_host, cols, per_span)


# clg_digest rows: two spans are equal only when both fields are equal
DIGEST =np.dtype([("hash", np.uint64), ("len", np.uint64)])


def digest_host(data: Union[bytes, np.ndarray]) -> Tuple[int, int]:
    """clg_digest_host: (hash, len) of host bytes on the CPU (no engine, no GPU) -- the same
    digest Engine.digest_logs / digest_spans compute on the device."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(
        data, np.uint8)
    d = _lib.Digest()
    check(lib.clg_digest_host(buf.ctypes.data if buf.size else None, buf.size, C.byref(d)))
    return int(d.hash), int(d.len)


# clg_diff rows: equal when lcp == len_log == len_ref; one a prefix of the other when
# lcp == min(len_log, len_ref) and the lengths differ; otherwise lcp is the first differing byte
DIFF = np.dtype([("lcp", np.uint64), ("len_log", np.uint64), ("len_ref", np.uint64)])


def lcp_host(a: Union[bytes, np.ndarray], b: Union[bytes, np.ndarray]) -> int:
    """clg_lcp_host: the number of leading bytes a and b have in common, on the CPU (no engine,
    no GPU) -- what Engine.diff_logs computes on the device."""
    ba, bb = (x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), np.uint8) for x in (a, b))
    ba, bb = np.ascontiguousarray(ba, np.uint8), np.ascontiguousarray(bb, np.uint8)
    out = C.c_uint64(0)
    check(lib.clg_lcp_host(ba.ctypes.data if ba.size else None, ba.size, bb.ctypes.data if bb.size else None, bb.size,
                           C.byref(out)))
    return int(out.value)


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def _flat_cuts(cuts, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """cuts as a list of n arrays, or a (first, flat) pair -> (first uint64[n + 1], flat uint32)."""
    if isinstance(cuts, tuple) and len(cuts) == 2 and np.ndim(cuts[0]) == 1 and len(cuts[0]) == n + 1:
        first = np.ascontiguousarray(cuts[0], np.uint64)
        wide = np.asarray(cuts[1])
    else:
        per = [np.asarray(c).reshape(-1) for c in cuts]
        if len(per) != n:
            raise ValueError("one array of cuts per request")
        first = np.zeros(n + 1, np.uint64)
        np.cumsum([c.size for c in per], out=first[1:])
        wide = np.concatenate(per) if per else np.zeros(0, np.uint32)
    wide = wide.reshape(-1)
    if wide.size and (int(wide.min()) < 0 or int(wide.max()) >> 32):
        raise ValueError("cuts must fit 32 bits")
    if first[0] != 0 or int(first[-1]) != wide.size or (np.diff(first.astype(np.int64)) < 0).any():
        raise ValueError("first must start at 0, not decrease and end at the number of cuts")
    return first, np.ascontiguousarray(wide, np.uint32)


def digest_prefixes_host(data: Union[bytes, np.ndarray], cuts) -> np.ndarray:
    """clg_digest_prefixes_host: a DIGEST row per cut, the digest of the first min(cut, len) bytes
    of host bytes, on the CPU in one pass (no engine, no GPU) -- what Engine.digest_prefixes
    computes on the device.  Cuts must not decrease."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(
        data, np.uint8)
    _, c = _flat_cuts([cuts], 1)
    out = np.zeros(c.size, DIGEST)
    check(lib.clg_digest_prefixes_host(buf.ctypes.data if buf.size else None, buf.size, _np_ptr(c), c.size,
                                       _np_ptr(out)))
    return out


class Engine:
    """One engine per GPU (one process per GPU).  Owns the HBM segment pool."""

    def __init__(self, segment_bytes: int = 16384, pool_segments: int = 16384, device: int = 0,
                 sharing_depth: int = _lib.CLG_FULL_SHARING, timing: bool = False, decode: str = "auto",
                 async_slice: bool = False, ifl_segment_bytes: Optional[int] = None,
                 ifl_pool_segments: Optional[int] = None, host_tail_bytes: Optional[int] = None):
        """decode: "auto" = single-launch decode for small batches, else the fast three-pass
        decode, robust multi-pass pipeline on abort; "three_pass" = no single-launch path
        (CLG_F_NO_SMALL_DECODE); "robust" = the robust pipeline only (CLG_F_ROBUST_DECODE).  async_slice: device-output
        slices return once queued on the gather stream (CLG_F_ASYNC_SLICE); sync() before
        reading them.  ifl_*: the in-flight log's own pool (default: the same geometry as the
        determinant pool)."""
        if decode not in ("auto", "three_pass", "robust"):
            raise ValueError(f"decode must be 'auto', 'three_pass' or 'robust', not {decode!r}")
        cfg = _lib.Config()
        lib.clg_config_default(C.byref(cfg))
        cfg.segment_bytes = segment_bytes
        cfg.pool_segments = pool_segments
        cfg.device = device
        cfg.sharing_depth = sharing_depth
        if host_tail_bytes is not None:
            cfg.host_tail_bytes = host_tail_bytes
        cfg.ifl_segment_bytes = ifl_segment_bytes if ifl_segment_bytes is not None else segment_bytes
        cfg.ifl_pool_segments = ifl_pool_segments if ifl_pool_segments is not None else pool_segments
        cfg.flags = ((_lib.CLG_F_TIMING if timing else 0) | (_lib.CLG_F_ROBUST_DECODE if decode == "robust" else 0)
                     | (_lib.CLG_F_NO_SMALL_DECODE if decode == "three_pass" else 0)
                     | (_lib.CLG_F_ASYNC_SLICE if async_slice else 0))
        h = C.c_void_p()
        check(lib.clg_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._out_slots: List[dict] = []  # _pooled_outputs
        self._in_sc = None  # _in_scratch
        self._in_mu = threading.Lock()  # its user
        self._pool_mu = threading.Lock()  # slot picks (a picked slot is busy until _finish)
        self.segment_bytes = segment_bytes
        self.sharing_depth = sharing_depth
        self.async_slice = async_slice
        self.device = device
        self._logs = {}
        self._queued = collections.deque()  # queued asynchronous decodes, oldest first (clg_decode_wait is FIFO)

    # ---- lifecycle ----------------------------------------------------------------
    def close(self):
        if self._h:
            self._out_release()
            lib.clg_engine_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return lib.clg_engine_stream(self._h) or 0

    def sync(self):
        check(lib.clg_sync(self._h))

    def pool_stats(self) -> Tuple[int, int]:
        u, f = C.c_uint32(), C.c_uint32()
        check(lib.clg_pool_stats(self._h, C.byref(u), C.byref(f)))
        return u.value, f.value

    def ifl_pool_stats(self) -> Tuple[int, int]:
        u, f = C.c_uint32(), C.c_uint32()
        check(lib.clg_ifl_pool_stats(self._h, C.byref(u), C.byref(f)))
        return u.value, f.value

    # ---- jobs (JobCausalLogImpl scope) ----------------------------------------------------
    def open_job(self, job_id: Tuple[int, int], sharing_depth: int = _lib.CLG_FULL_SHARING) -> int:
        """A further JobCausalLog on this engine (job 0 is the engine's default job): its own
        logs, sharing depth and latestCompletedCheckpoint CAS."""
        j = C.c_uint32()
        check(lib.clg_job_open(self._h, job_id[0], job_id[1], sharing_depth, C.byref(j)))
        return j.value

    def close_job(self, job: int) -> None:
        check(lib.clg_job_close(self._h, job))
        self._logs = {k: v for k, v in self._logs.items() if k[0] != job}

    # ---- logs -----------------------------------------------------------------------
    def open_log(self, cid: CausalLogID, job: int = 0) -> "ThreadCausalLog":
        h = C.c_uint32()
        check(lib.clg_log_open(self._h, job, C.byref(cid.to_c()), C.byref(h)))
        log = ThreadCausalLog(self, h.value, cid, job)
        self._logs[(job, cid.key())] = log
        return log

    def get_log(self, cid: CausalLogID, job: int = 0) -> Optional["ThreadCausalLog"]:
        """The open log for `cid` (also logs the engine opened itself, e.g. by processCausalLogDelta)."""
        log = self._logs.get((job, cid.key()))
        if log is None:
            h = C.c_uint32()
            if lib.clg_log_find(self._h, job, C.byref(cid.to_c()), C.byref(h)) == _lib.CLG_OK:
                log = self._logs[(job, cid.key())] = ThreadCausalLog(self, h.value, cid, job)
        return log

    def append_batch(self, logs: np.ndarray, epochs: np.ndarray, offs: np.ndarray, lens: np.ndarray,
                     data: np.ndarray):
        logs = np.ascontiguousarray(logs, np.uint32)
        epochs = np.ascontiguousarray(epochs, np.int64)
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint32)
        data = np.ascontiguousarray(data, np.uint8)
        check(lib.clg_append_batch(self._h, _np_ptr(logs), _np_ptr(epochs), _np_ptr(offs), _np_ptr(lens),
                                   len(logs), _np_ptr(data)))

    # ---- batched slicing ----------------------------------------------------------------
    def slice_batch(self, reqs: Sequence[Tuple["ThreadCausalLog", ChannelLike, int]], out=None,
                    cap: Optional[int] = None):
        """Batched hasDelta/getOffset/getDelta.  `out`: None (host bytes returned), a numpy
        uint8 array, or a device pointer (int, CLG_MEM_DEVICE) with `cap`."""
        n = len(reqs)
        creq = (_lib.SliceReq * max(n, 1))()
        for i, (log, ch, ep) in enumerate(reqs):
            creq[i].log = log.handle
            creq[i].consumer = _ch(ch)
            creq[i].epoch = ep
        cres = (_lib.SliceRes * max(n, 1))()
        total = C.c_uint64()
        if out is None or isinstance(out, np.ndarray):
            if out is None:
                out = np.empty(cap if cap is not None else self._slice_bound(reqs), np.uint8)
            st = lib.clg_slice_batch(self._h, C.cast(creq, C.c_void_p), n, C.cast(cres, C.c_void_p), _np_ptr(out),
                                     out.size, _lib.CLG_MEM_HOST, C.byref(total))
        else:
            st = lib.clg_slice_batch(self._h, C.cast(creq, C.c_void_p), n, C.cast(cres, C.c_void_p), int(out),
                                     int(cap), _lib.CLG_MEM_DEVICE, C.byref(total))
        check(st)
        res = [(cres[i].status, bool(cres[i].has_delta), cres[i].offset_from_epoch, cres[i].len, cres[i].out_off)
               for i in range(n)]
        return res, out, total.value

    def _slice_bound(self, reqs) -> int:
        b = 0
        for log in {id(r[0]): r[0] for r in reqs}.values():
            b += log.state()["writer"] * sum(1 for r in reqs if r[0] is log)
        return max(b, 1)

    def slice_batch_raw(self, creq, cres, n: int, out_ptr: int, cap: int, device: bool = True) -> int:
        """Zero-overhead variant for benchmarks: prebuilt ctypes request/result arrays."""
        total = C.c_uint64()
        check(lib.clg_slice_batch(self._h, C.cast(creq, C.c_void_p), n, C.cast(cres, C.c_void_p), out_ptr, cap,
                                  _lib.CLG_MEM_DEVICE if device else _lib.CLG_MEM_HOST, C.byref(total)))
        return total.value

    def log_lengths(self, handles: np.ndarray) -> Tuple[np.ndarray, int]:
        """logLength of many logs in one call: (per-log lengths, sum)."""
        h = np.ascontiguousarray(handles, np.uint32)
        out = np.zeros(max(h.size, 1), np.int32)
        tot = C.c_uint64()
        check(lib.clg_log_length_batch(self._h, _np_ptr(h), h.size, _np_ptr(out), C.byref(tot)))
        return out[:h.size], tot.value

    def upstream_delta_batch(self, reqs, n: int, src_ptr: int, in_kind: int) -> None:
        """Batched processUpstreamDelta over one buffer (host or device pointer); each
        request's status is written back into `reqs` (clg_delta_req)."""
        check(lib.clg_upstream_delta_batch(self._h, C.cast(reqs, C.c_void_p), n, src_ptr, in_kind))

    def seek_consumers_raw(self, creq, offsets: np.ndarray, n: int) -> None:
        """Batched consumer positioning over a prebuilt ctypes request array."""
        offs = np.ascontiguousarray(offsets, dtype=np.int32)
        check(lib.clg_consumer_seek_batch(self._h, C.cast(creq, C.c_void_p), offs.ctypes.data, n))

    # ---- checkpoint completion ---------------------------------------------------------
    def truncate_all(self, checkpoint_id: int, job: int = 0) -> bool:
        """JobCausalLogImpl.notifyCheckpointComplete (:230-246) for `job`: CAS, then every log of it."""
        applied = C.c_int32()
        check(lib.clg_truncate_all(self._h, job, checkpoint_id, C.byref(applied)))
        return bool(applied.value)

    # ---- decode -------------------------------------------------------------------------
    # (name, dtype, itemsize, side table?) of clg_decoded's host arrays
    _OUT_FIELDS = (("off", np.uint32, 4, 0), ("tag", np.uint8, 1, 0), ("v0", np.int64, 8, 0), ("w_idx", np.uint32, 4, 1),
                   ("w_rc", np.int32, 4, 1), ("w_v1", np.int64, 8, 1), ("w_var_off", np.uint32, 4, 1),
                   ("w_var_len", np.uint32, 4, 1), ("w_sub", np.uint8, 1, 1))

    @staticmethod
    def _out_bytes(cap: int, wcap: int, bcap: int = 0) -> Tuple[List[int], int]:
        """Offsets of the nine arrays (16-byte aligned), then of span_rec_base (bcap entries)."""
        offs, at = [], 0
        for _, _, isz, wide in Engine._OUT_FIELDS:
            offs.append(at)
            at = (at + isz * (wcap if wide else cap) + 15) & ~15
        offs.append(at)
        return offs, at + 8 * bcap

    @staticmethod
    def _host_outputs(cap: int, wcap: int, buf: Optional[np.ndarray] = None, bcap: int = 0):
        """The SoA output arrays as views of one host buffer (one allocation, one pointer),
        and their clg_decoded.  buf: a buffer to carve them from (large enough), else a new one.
        bcap: also a span_rec_base array ("base") of that many entries."""
        offs, at = Engine._out_bytes(cap, wcap, bcap)
        if buf is None or buf.size < at:
            buf = np.empty(max(at, 16), np.uint8)
        b0 = buf.ctypes.data
        d = _lib.Decoded()
        arrs = {}
        for (k, dt, isz, wide), o in zip(Engine._OUT_FIELDS, offs):
            arrs[k] = buf[o:o + isz * (wcap if wide else cap)].view(dt)
            setattr(d, k, b0 + o)
        if bcap:
            arrs["base"] = buf[offs[-1]:offs[-1] + 8 * bcap].view(np.uint64)
        d.cap, d.wcap, d.out_kind = cap, wcap, _lib.CLG_MEM_HOST
        return d, arrs

    @staticmethod
    def _slot_capacity(size: int, cap: int, wcap: int, bcap: int) -> Tuple[int, int, int]:
        """The largest capacities in the proportions of (cap, wcap) -- and at least 256 span
        entries -- whose arrays fit a slot of `size` bytes; (cap, wcap, bcap) when they do not."""
        b = max(bcap, 256)
        k = (size - 8 * b - 160) / max(13 * cap + 25 * wcap, 1)  # 160: more than the padding
        if k < 1.0:
            return cap, wcap, bcap
        return int(cap * k), int(wcap * k), b

    _OUT_SLOTS = 3  # pooled output buffers (a caller usually keeps one batch while asking for the next)

    @staticmethod
    def _slot_free(sl) -> bool:
        # not between its pick and _finish, and references when free: the slot, getrefcount's
        # argument, and the cached views
        return not sl["busy"] and sys.getrefcount(sl["buf"]) <= 2 + (
            len(sl["cache"][2]) if sl["cache"] is not None else 0)

    def _slot_done(self, arrs) -> None:
        """The decode that picked the slot of `arrs` has made its result (or failed)."""
        for sl in self._out_slots:
            if sl["cache"] is not None and sl["cache"][2] is arrs:
                sl["busy"] = False

    def _slot_use(self, pick):
        """The slot becomes busy and the most recent (by identity: the slots hold arrays); its
        cached clg_decoded, views and byref, counts reset."""
        pick["busy"] = True
        if self._out_slots[-1] is not pick:
            self._out_slots = [sl for sl in self._out_slots if sl is not pick] + [pick]
        _, d, arrs, ref = pick["cache"]
        d.n_rec = d.n_wide = 0
        return d, arrs, ref

    def _pooled_outputs(self, cap: int, wcap: int, bcap: int = 0):
        """_host_outputs from one of the engine's reusable buffers that no earlier result still
        holds (every returned array is a view of its buffer, so a live batch keeps the buffer's
        reference count up): the pages stay mapped -- not faulted in on every call -- and
        registered for the device (clg_host_register), so the single-launch small decode writes
        the outputs straight into them (CLG_MEM_MAPPED).  The views are carved at the slot's
        whole capacity (_slot_capacity) and serve again for every request they cover.
        Returns (clg_decoded, arrays, byref(clg_decoded))."""
        with self._pool_mu:
            return self._pooled_pick(cap, wcap, bcap)

    def _pooled_pick(self, cap: int, wcap: int, bcap: int):
        need = self._out_bytes(cap, wcap, bcap)[1]
        pick = None
        for sl in self._out_slots:
            c = sl["cache"]
            if c is not None and c[0][0] >= cap and c[0][1] >= wcap and c[0][2] >= bcap and self._slot_free(sl):
                return self._slot_use(sl)
            if pick is None and sl["buf"].size >= need and self._slot_free(sl):
                pick = sl
        if pick is None:
            idle = [i for i, sl in enumerate(self._out_slots) if not sl["busy"]]
            if len(self._out_slots) >= self._OUT_SLOTS and idle:  # all held (or too small): the oldest
                self._slot_release(self._out_slots.pop(idle[0]))  # not being decoded into leaves the pool
            size = (max(need, 1 << 16) + 4095) & ~4095  # page-aligned: an anonymous mapping
            buf = np.frombuffer(mmap.mmap(-1, size), np.uint8)
            mapped = self._h is not None and lib.clg_host_register(_np_ptr(buf), size) == _lib.CLG_OK
            pick = {"buf": buf, "mapped": mapped, "cache": None, "busy": False}
            self._out_slots.append(pick)
        pick["cache"] = None  # (its views would hold the buffer)
        key = self._slot_capacity(pick["buf"].size, cap, wcap, bcap)
        d, arrs = self._host_outputs(*key[:2], pick["buf"], key[2])
        if pick["mapped"]:
            d.out_kind = _lib.CLG_MEM_MAPPED
        pick["cache"] = (key, d, arrs, C.byref(d))
        pick["bptr"] = arrs["base"].ctypes.data if "base" in arrs else 0
        return self._slot_use(pick)

    def _slot_release(self, sl):
        """A pooled buffer leaves the pool: unregistered (a batch the caller keeps stays valid as
        ordinary host memory)."""
        if sl["mapped"]:
            lib.clg_host_unregister(_np_ptr(sl["buf"]))
        sl["cache"] = None

    def _out_release(self):
        while self._out_slots:
            self._slot_release(self._out_slots.pop())

    @property
    def _out_buf(self):  # the most recently used pooled buffer (tests)
        return self._out_slots[-1]["buf"] if self._out_slots else None

    @property
    def _out_cache(self):
        return self._out_slots[-1]["cache"] if self._out_slots else None

    @property
    def _out_mapped(self):
        return bool(self._out_slots) and self._out_slots[-1]["mapped"]

    def _finish(self, st, d, arrs, base, n_spans, spans_bytes):
        """The batch as slices of the slot's views (they hold its buffer); the slot's pick ends."""
        try:
            if st != _lib.CLG_OK:
                err = _lib.ClonosError(st, lib.clg_last_error().decode(errors="replace"))
                err.err_span, err.err_off, err.err_tag = d.err_span, d.err_off, d.err_tag
                err.n_rec = d.n_rec
                raise err
            nr, nw = d.n_rec, d.n_wide
            return DecodedBatch(arrs["off"][:nr], arrs["tag"][:nr], arrs["v0"][:nr], arrs["w_idx"][:nw],
                                arrs["w_rc"][:nw], arrs["w_v1"][:nw], arrs["w_var_off"][:nw],
                                arrs["w_var_len"][:nw], arrs["w_sub"][:nw], base[:n_spans + 1], spans_bytes)
        finally:
            self._slot_done(arrs)

    def decode_host(self, data: Union[bytes, np.ndarray], spans: Optional[Sequence[Tuple[int, int]]] = None
                    ) -> DecodedBatch:
        """DeterminantEncoder.decodeNext over whole spans of host bytes, on the GPU."""
        buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(
            data, np.uint8)
        if spans is None:
            spans = [(0, buf.size)]
        so = np.array([s[0] for s in spans], np.uint64)
        sl = np.array([s[1] for s in spans], np.uint64)
        cap = int(sl.sum()) // 2 + len(spans) + 1
        wcap = int(sl.sum()) // 6 + len(spans) + 1
        d, arrs, ref = self._pooled_outputs(cap, wcap)
        base = np.zeros(len(spans) + 1, np.uint64)
        st = lib.clg_decode_host(self._h, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans), ref, _np_ptr(base))
        return self._finish(st, d, arrs, base, len(spans),
                            [buf[int(o):int(o) + int(n)] for o, n in zip(so, sl)])

    def decode_logs(self, logs: Sequence["ThreadCausalLog"], start_epochs: Sequence[int],
                    keep_bytes: bool = False) -> DecodedBatch:
        n = len(logs)
        own = self._in_mu.acquire(blocking=False)  # the reused handle / epoch arrays, else new ones
        try:
            sc = self._in_scratch(n) if own else self._in_arrays(n)
            h, ep = sc[0][:n], sc[1][:n]
            h[:] = [l.handle for l in logs]
            ep[:] = start_epochs
            # a free registered slot whose capacity covers the batch decodes without logLength;
            # a batch beyond it fails with CLG_E_CAPACITY (nothing changed) and is sized below
            fast = self._pooled_fast(n)
            st = _lib.CLG_E_CAPACITY
            if fast is not None:
                d, arrs, ref, bptr = fast
                st = lib.clg_decode_logs(self._h, sc[2], sc[3], n, ref, bptr)
                if st == _lib.CLG_E_CAPACITY:
                    self._slot_done(arrs)
            if st == _lib.CLG_E_CAPACITY:
                total = self.log_lengths(h)[1]  # logLength bounds every span (one native call for the batch)
                d, arrs, ref = self._pooled_outputs(total // 2 + n + 1, total // 6 + n + 1, n + 1)
                st = lib.clg_decode_logs(self._h, sc[2], sc[3], n, ref, arrs["base"].ctypes.data)
        finally:
            if own:
                self._in_mu.release()
        sb = [np.frombuffer(l.getDeterminants(e), np.uint8) for l, e in zip(logs, start_epochs)] if keep_bytes else None
        return self._finish(st, d, arrs, arrs["base"], n, sb)

    def _in_scratch(self, n: int):
        """Reused handle / epoch arrays of decode_logs, with their addresses."""
        sc = self._in_sc
        if sc is None or sc[0].size < n:
            sc = self._in_sc = self._in_arrays(max(64, 1 << max(n - 1, 0).bit_length()))
        return sc

    @staticmethod
    def _in_arrays(n: int):
        h, ep = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int64)
        return h, ep, h.ctypes.data, ep.ctypes.data

    def _pooled_fast(self, n_spans: int):
        """A free registered slot with a span_rec_base of n_spans + 1 entries (its views carved at
        its whole capacity), or None."""
        with self._pool_mu:
            for sl in self._out_slots:
                c = sl["cache"]
                if c is not None and sl["mapped"] and c[0][2] > n_spans and self._slot_free(sl):
                    return self._slot_use(sl) + (sl["bptr"],)
        return None

    def decode_logs_async(self, logs: Sequence["ThreadCausalLog"], start_epochs: Sequence[int]) -> "PendingDecode":
        """clg_decode_logs_async into host arrays: returns at once; .wait() gives the batch.
        Up to CLG_DECODE_MAX_INFLIGHT may be queued; their waits complete them in queue order
        (waiting for a later one first completes the earlier ones, whose results are kept)."""
        h = np.array([l.handle for l in logs], np.uint32)
        ep = np.array(start_epochs, np.int64)
        total = self.log_lengths(h)[1]
        d, arrs, ref = self._pooled_outputs(total // 2 + len(logs) + 1, total // 6 + len(logs) + 1)
        base = np.zeros(len(logs) + 1, np.uint64)
        pd = PendingDecode(self, (h, ep, d, arrs, base), len(logs))
        st = lib.clg_decode_logs_async(self._h, _np_ptr(h), _np_ptr(ep), len(logs), ref, _np_ptr(base))
        if st != _lib.CLG_OK:
            self._slot_done(arrs)
            check(st)
        self._queued.append(pd)
        return pd

    def decode_logs_device(self, handles: np.ndarray, start_epochs: np.ndarray, dec: _lib.Decoded,
                           base: np.ndarray) -> None:
        """Benchmark variant: outputs are caller-owned device arrays described by `dec`."""
        check(lib.clg_decode_logs(self._h, _np_ptr(handles), _np_ptr(start_epochs), len(handles), C.byref(dec),
                                  _np_ptr(base)))

    def decode_logs_device_async(self, handles: np.ndarray, start_epochs: np.ndarray, dec: _lib.Decoded,
                                 base: np.ndarray) -> None:
        """clg_decode_logs_async: queues the decode and returns; `dec`, `base` and the output
        arrays stay untouched by the caller until the decode_wait() that pairs with it (FIFO;
        up to CLG_DECODE_MAX_INFLIGHT queued, each with its own outputs)."""
        keep = (handles, start_epochs, dec, base)  # kept alive until the wait
        check(lib.clg_decode_logs_async(self._h, _np_ptr(handles), _np_ptr(start_epochs), len(handles),
                                        C.byref(dec), _np_ptr(base)))
        self._queued.append(keep)

    # ---- typed replay columns (clg_columns)
    @staticmethod
    def _column_bounds(total: int, n_spans: int) -> dict:
        """Capacities no batch of `total` encoded bytes can exceed (the shortest record of each
        class: ORDER 2 B, TIMESTAMP 9, RNG and BUFFER_BUILT 5, wide 6), untouched pages of
        np.empty arrays cost nothing."""
        cap = {"tag": total // 2, "order": total // 2, "timestamp": total // 9, "rng": total // 5,
               "buffer_built": total // 5}
        return {k: np.empty(cap.get(k, total // 6) + n_spans + 1, dt) for k, dt in _COL_FIELDS}

    def _columns_finish(self, st: int, c: _lib.Columns, arrs, base, spans_bytes, partial: bool) -> DecodedColumns:
        if st != _lib.CLG_OK and not (partial and c.err_status == st):
            raise _columns_error(st, c)
        cols = _columns_result(c, arrs, base, spans_bytes)
        if st != _lib.CLG_OK:
            cols.error = _columns_error(st, c)
        return cols

    def columnize(self, dec: _lib.Decoded, base: np.ndarray, cols: Optional[_lib.Columns] = None
                  ) -> Optional[DecodedColumns]:
        """clg_columnize: the typed columns of a decoded batch that lies in device memory (or in
        registered host memory, dec.out_kind CLG_MEM_MAPPED); dec.n_rec / n_wide are the decode's
        results, base its span_rec_base.  cols: a clg_columns the caller set up (any out_kind, or
        all pointers null for sizes only) -- filled in place, its status raised; None: host arrays
        of exactly the batch's sizes (a sizes-only call first), returned as DecodedColumns."""
        base = np.ascontiguousarray(base, np.uint64)
        n_spans = max(base.size - 1, 0)
        if cols is not None:
            st = lib.clg_columnize(self._h, C.byref(dec), _np_ptr(base), n_spans, C.byref(cols))
            if st != _lib.CLG_OK:
                raise _columns_error(st, cols)
            return None
        sb = np.zeros((n_spans + 1) * _lib.COL_CLASSES, np.uint64)
        c = _lib.Columns()
        c.span_base = _np_ptr(sb)
        st = lib.clg_columnize(self._h, C.byref(dec), _np_ptr(base), n_spans, C.byref(c))
        if st != _lib.CLG_OK:
            raise _columns_error(st, c)
        arrs = _host_columns(int(c.n_rec), [int(x) for x in c.n_class])
        c = _columns_struct(arrs, sb, _lib.CLG_MEM_HOST)
        st = lib.clg_columnize(self._h, C.byref(dec), _np_ptr(base), n_spans, C.byref(c))
        if st != _lib.CLG_OK:
            raise _columns_error(st, c)
        return _columns_result(c, arrs, sb)

    @staticmethod
    def _payload_bounds(total: int, n_spans: int) -> Tuple[np.ndarray, np.ndarray]:
        """var / pos no batch of `total` encoded bytes can exceed (a wide record is at least 6 B)."""
        return np.empty(total + 1, np.uint8), np.empty(total // 6 + n_spans + 2, np.uint64)

    @staticmethod
    def _payloads_attach(cols: DecodedColumns, p: _lib.Payloads, var: np.ndarray, pos: np.ndarray) -> DecodedColumns:
        cols.var, cols.var_pos = var[:int(p.n_var)], pos[:int(p.n_rows) + 1]
        return cols

    # ---- packed typed columns (clg_packed)
    def pack_columns(self, cols: DecodedColumns) -> PackedColumns:
        """clg_pack_columns: the five narrow columns of host columns bit-packed on the device (staged
        in, packed, read back); the bytes are pack_columns_host's."""
        cin, keep = _pack_in(cols)
        return _pack_narrow(lambda p: lib.clg_pack_columns(self._h, C.byref(cin), C.byref(p)), cols)

    def pack_columns_raw(self, cin: _lib.Columns, out: _lib.Packed) -> int:
        """clg_pack_columns over a clg_columns and a clg_packed the caller set up (any kinds; desc
        and bits null: sizes only).  Returns the status; the results are in out."""
        return lib.clg_pack_columns(self._h, C.byref(cin), C.byref(out))

    def pack_wide(self, cols: DecodedColumns) -> PackedWide:
        """clg_pack_wide: the wide rows of host columns partitioned by kind and bit-packed on the
        device (staged in, packed, read back); the bytes are pack_wide_host's."""
        cin, keep = _pack_wide_in(cols)
        return _pack_wide(lambda p: lib.clg_pack_wide(self._h, C.byref(cin), C.byref(p)))

    def pack_wide_raw(self, cin: _lib.Columns, out: _lib.PackedWideC) -> int:
        """clg_pack_wide over a clg_columns and a clg_packed_wide the caller set up (any kinds; desc
        and bits NULL: sizes only); returns the status."""
        return lib.clg_pack_wide(self._h, C.byref(cin), C.byref(out))

    def unpack_columns(self, packed: PackedColumns) -> DecodedColumns:
        """clg_unpack_columns: the five narrow columns of host packed columns unpacked on the device
        (staged in, checked, unpacked, read back); the wide rows, span_base, var, var_pos and error
        are passed through as PackedColumns.unpack() does.  Invalid input raises ClonosError with
        bad_what, bad_stream and bad_block."""
        p = packed._struct()
        c, arrs = _unpack_out(packed.n_val)
        bad = _lib.UnpackBad()
        st = lib.clg_unpack_columns(self._h, C.byref(p), C.byref(c), C.byref(bad))
        if st != _lib.CLG_OK:
            raise _unpack_error(st, bad)
        return _unpacked(packed, arrs)

    def unpack_wide(self, packed_wide: PackedWide, pos: bool = False) -> dict:
        """clg_unpack_wide: host packed wide rows unpacked on the device (staged in, checked,
        unpacked, read back): the seven w_* arrays by name, in row order, as unpack_wide_host gives
        them; pos=True adds "pos", the exclusive prefix sum of w_var_len (n_wide + 1 entries).
        Invalid input raises ClonosError with bad_what, bad_stream and bad_block."""
        p = packed_wide._struct()
        c = _lib.Columns()
        bad = _lib.UnpackBad()
        st = lib.clg_unpack_wide(self._h, C.byref(p), C.byref(c), None, C.byref(bad))  # the layout check and the rows
        if st != _lib.CLG_OK:
            raise _unpack_error(st, bad)
        n = int(c.n_class[4])
        arrs = {}
        for name, dt in _COL_FIELDS[5:]:
            arrs[name] = np.empty(n, dt)
            setattr(c, name, _np_ptr(arrs[name]) or None)
        c.cap_wide, c.out_kind = n, _lib.CLG_MEM_HOST
        if pos:
            arrs["pos"] = np.empty(n + 1, np.uint64)
        if n == 0 and not pos:  # (every pointer is null: that would be the sizes-only call again)
            return arrs
        st = lib.clg_unpack_wide(self._h, C.byref(p), C.byref(c), _np_ptr(arrs["pos"]) if pos else None, C.byref(bad))
        if st != _lib.CLG_OK:
            raise _unpack_error(st, bad)
        return arrs

    def unpack_wide_raw(self, pin: _lib.PackedWideC, cols: _lib.Columns, pos: Optional[int], bad: _lib.UnpackBad) -> int:
        """clg_unpack_wide over a clg_packed_wide and a clg_columns the caller set up (any kinds; the
        seven w_* pointers and pos null: sizes only); pos is an address or None.  Returns the
        status; the results are in cols and bad."""
        return lib.clg_unpack_wide(self._h, C.byref(pin), C.byref(cols), pos, C.byref(bad))

    def unpack_columns_raw(self, pin: _lib.Packed, cols: _lib.Columns, bad: _lib.UnpackBad) -> int:
        """clg_unpack_columns over a clg_packed and a clg_columns the caller set up (any kinds; the
        five narrow pointers null: sizes only).  Returns the status; the results are in cols and bad."""
        return lib.clg_unpack_columns(self._h, C.byref(pin), C.byref(cols), C.byref(bad))

    # ---- the packed payload column (clg_packed_payloads)
    def pack_payloads(self, var, pos, device: bool = False, n_rows: Optional[int] = None) -> PackedPayloads:
        """clg_pack_payloads: the payload column (var, pos) front-coded on the device; the bytes are
        pack_payloads_host's.  device=False: var and pos are host arrays (staged); device=True: they
        are device addresses (ints) and n_rows is given.  The packed form is read back."""
        if device:
            vp, pp, n, kind, keep = int(var or 0), int(pos or 0), int(n_rows), _lib.CLG_MEM_DEVICE, None
        else:
            keep = _payload_column(var, pos)
            vp, pp, n, kind = _np_ptr(keep[0]), _np_ptr(keep[1]), keep[1].size - 1, _lib.CLG_MEM_HOST
        return _pack_payloads_twice(lambda p: lib.clg_pack_payloads(self._h, vp or None, pp or None, n, kind, C.byref(p)))

    def pack_payloads_raw(self, var: Optional[int], pos: Optional[int], n_rows: int, in_kind: int,
                          out: _lib.PackedPayloadsC) -> int:
        """clg_pack_payloads over addresses and a clg_packed_payloads the caller set up (any kinds;
        desc, bits and tail null: sizes only).  Returns the status; the results are in out."""
        return lib.clg_pack_payloads(self._h, var or None, pos or None, n_rows, in_kind, C.byref(out))

    def unpack_payloads(self, packed: PackedPayloads, pos) -> np.ndarray:
        """clg_unpack_payloads: a host packed payload column unpacked on the device (staged in,
        checked, unpacked, read back): var of the column whose pos (a host array) is given.  Invalid
        input raises ClonosError with bad_what, bad_stream and bad_block."""
        pos = np.ascontiguousarray(pos, np.uint64)
        return _unpack_payloads(lambda p, out, bad: lib.clg_unpack_payloads(
            self._h, C.byref(p), _np_ptr(pos) or None, _lib.CLG_MEM_HOST, C.byref(out), C.byref(bad)), packed)

    def unpack_payloads_raw(self, pin: _lib.PackedPayloadsC, pos: Optional[int], pos_kind: int, out: _lib.Payloads,
                            bad: _lib.UnpackBad) -> int:
        """clg_unpack_payloads over a clg_packed_payloads, a pos address and a clg_payloads the
        caller set up (any kinds; var null: sizes only).  Returns the status."""
        return lib.clg_unpack_payloads(self._h, C.byref(pin), pos or None, pos_kind, C.byref(out), C.byref(bad))

    def _decode_packed(self, call, total: int, n: int, spans_bytes, partial: bool, payloads: bool,
                       pack_wide: bool = False) -> PackedColumns:
        """call(wide, var or None, packed[, packed wide]) -> status, over bounds no batch of `total`
        encoded bytes can exceed: a record is at least 2 bytes and its value at most its encoded
        length less the tag, so the streams hold at most `total` bytes in at most total / 1024 + 5
        blocks, each padded by less than 16 bytes.  pack_wide: the wide rows (at most total / 6 + n + 1
        of them) come packed too, and the payload column without pos.  A residual is at most as wide
        as its element, but for the DELTA of a zero-extended u32 (IDX, VAR_OFF), which can take 33
        bits: 8 + 33 + 32 + 64 + 33 + 32 + 8 + 64 = 274 bits a row over KIND, IDX and a kind's six
        streams, under 35 bytes."""
        base = np.zeros((n + 1) * _lib.COL_CLASSES, np.uint64)
        c = _lib.Columns()
        if pack_wide:
            rows = total // 6 + n + 1
            wdesc = np.empty(8 * (rows // 1024) + _lib.WPACK_STREAMS, PACK_BLOCK)
            wbits = np.empty(35 * rows + 16 * wdesc.size, np.uint8)
            wpk = _packed_wide_struct(wdesc, wbits)
        else:
            arrs = {k: np.empty(total // 6 + n + 1, dt) for k, dt in _COL_FIELDS if k in _COL_WIDE}
            for k in _COL_WIDE:
                setattr(c, k, _np_ptr(arrs[k]))
            c.cap_wide = min(a.size for a in arrs.values())
        c.span_base, c.out_kind = _np_ptr(base), _lib.CLG_MEM_HOST
        desc = np.empty(total // 1024 + 5, PACK_BLOCK)
        bits = np.empty(total + 16 * desc.size, np.uint8)
        pk = _packed_struct(desc, bits)
        var = pos = p = None
        if payloads:
            var, pos = self._payload_bounds(total, n)
            p = _payloads_struct(var, None if pack_wide else pos)
        st = call(c, p, pk, wpk) if pack_wide else call(c, p, pk)
        if st != _lib.CLG_OK and not (partial and c.err_status == st):
            raise _columns_error(st, c)
        nw = int(c.n_class[_lib.COL_WIDE])
        narrow = (desc[:int(pk.blk_base[_lib.PACK_STREAMS])], bits[:int(pk.n_bits)], pk.n_val, pk.blk_base)
        if pack_wide:
            wide = PackedWide(wdesc[:int(wpk.blk_base[_lib.WPACK_STREAMS])], wbits[:int(wpk.n_bits)], wpk.n_val, wpk.blk_base)
            out = PackedColumns(*narrow, *[None] * len(_COL_WIDE), base, spans_bytes, wide_packed=wide)
        else:
            out = PackedColumns(*narrow, *[arrs[k][:nw] for k in _COL_WIDE], base, spans_bytes)
        if st != _lib.CLG_OK:
            out.error = _columns_error(st, c)
        if payloads:
            out.var = var[:int(p.n_var)]
            if not pack_wide:
                out.var_pos = pos[:int(p.n_rows) + 1]
        return out

    def decode_logs_columns(self, logs: Sequence["ThreadCausalLog"], start_epochs: Sequence[int],
                            keep_bytes: bool = False, partial: bool = False, payloads: bool = False,
                            packed: bool = False, pack_wide: bool = False) -> Union[DecodedColumns, PackedColumns]:
        """clg_decode_logs_columns: decode_logs' ranges decoded on the GPU and delivered as typed
        columns.  A decode error raises as decode_logs' does; partial=True returns the columns of
        each span's records up to its first error instead, the error in .error.  payloads=True
        (clg_decode_logs_columns_var): the wide rows' payload bytes come with the columns, gathered
        on the device (.var, .var_pos, .payload(k)); the logs' bytes do not cross the link.
        packed=True (clg_decode_logs_columns_packed): the five narrow columns come bit-packed, as
        PackedColumns.  pack_wide=True with packed=True (clg_decode_logs_columns_packed_wide): the
        wide rows come packed by kind as well (PackedColumns.wide_packed) and the payload column
        without var_pos, which is rebuilt from the lengths on first use."""
        n = len(logs)
        h = np.array([l.handle for l in logs], np.uint32)
        ep = np.array(start_epochs, np.int64)
        total = self.log_lengths(h)[1] if n else 0
        if pack_wide and not packed:
            raise ValueError("pack_wide needs packed=True")
        if packed and pack_wide:
            sb = [np.frombuffer(l.getDeterminants(e), np.uint8) for l, e in zip(logs, start_epochs)] if keep_bytes else None
            return self._decode_packed(
                lambda c, p, pk, wpk: lib.clg_decode_logs_columns_packed_wide(
                    self._h, _np_ptr(h), _np_ptr(ep), n, C.byref(c), C.byref(p) if p is not None else None, C.byref(pk),
                    C.byref(wpk)),
                total, n, sb, partial, payloads, pack_wide=True)
        if packed:
            sb = [np.frombuffer(l.getDeterminants(e), np.uint8) for l, e in zip(logs, start_epochs)] if keep_bytes else None
            return self._decode_packed(
                lambda c, p, pk: lib.clg_decode_logs_columns_packed(self._h, _np_ptr(h), _np_ptr(ep), n, C.byref(c),
                                                                    C.byref(p) if p is not None else None, C.byref(pk)),
                total, n, sb, partial, payloads)
        arrs = self._column_bounds(total, n)
        base = np.zeros((n + 1) * _lib.COL_CLASSES, np.uint64)
        c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
        if payloads:
            var, pos = self._payload_bounds(total, n)
            p = _payloads_struct(var, pos)
            st = lib.clg_decode_logs_columns_var(self._h, _np_ptr(h), _np_ptr(ep), n, C.byref(c), C.byref(p))
        else:
            st = lib.clg_decode_logs_columns(self._h, _np_ptr(h), _np_ptr(ep), n, C.byref(c))
        sb = [np.frombuffer(l.getDeterminants(e), np.uint8) for l, e in zip(logs, start_epochs)] if keep_bytes else None
        cols = self._columns_finish(st, c, arrs, base, sb, partial)
        return self._payloads_attach(cols, p, var, pos) if payloads else cols

    def decode_logs_columns_raw(self, handles: np.ndarray, start_epochs: np.ndarray, cols: _lib.Columns) -> int:
        """clg_decode_logs_columns into a clg_columns the caller set up (any out_kind; all pointers
        null: sizes only).  Returns the status; the results are in cols."""
        return lib.clg_decode_logs_columns(self._h, _np_ptr(handles), _np_ptr(start_epochs), len(handles), C.byref(cols))

    def decode_host_columns(self, data: Union[bytes, np.ndarray], spans: Optional[Sequence[Tuple[int, int]]] = None,
                            partial: bool = False, payloads: bool = False, packed: bool = False,
                            pack_wide: bool = False) -> Union[DecodedColumns, PackedColumns]:
        """clg_decode_host_columns: decode_host's spans decoded on the GPU and delivered as typed
        columns (errors, payloads, packed and pack_wide as decode_logs_columns)."""
        buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(
            data, np.uint8)
        if spans is None:
            spans = [(0, buf.size)]
        so = np.array([s[0] for s in spans], np.uint64)
        sl = np.array([s[1] for s in spans], np.uint64)
        if pack_wide and not packed:
            raise ValueError("pack_wide needs packed=True")
        if packed and pack_wide:
            return self._decode_packed(
                lambda c, p, pk, wpk: lib.clg_decode_host_columns_packed_wide(
                    self._h, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans), C.byref(c),
                    C.byref(p) if p is not None else None, C.byref(pk), C.byref(wpk)),
                int(sl.sum()), len(spans), [buf[int(o):int(o) + int(k)] for o, k in zip(so, sl)], partial, payloads,
                pack_wide=True)
        if packed:
            return self._decode_packed(
                lambda c, p, pk: lib.clg_decode_host_columns_packed(self._h, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans),
                                                                    C.byref(c), C.byref(p) if p is not None else None,
                                                                    C.byref(pk)),
                int(sl.sum()), len(spans), [buf[int(o):int(o) + int(k)] for o, k in zip(so, sl)], partial, payloads)
        arrs = self._column_bounds(int(sl.sum()), len(spans))
        base = np.zeros((len(spans) + 1) * _lib.COL_CLASSES, np.uint64)
        c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
        if payloads:
            var, pos = self._payload_bounds(int(sl.sum()), len(spans))
            p = _payloads_struct(var, pos)
            st = lib.clg_decode_host_columns_var(self._h, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans), C.byref(c),
                                                 C.byref(p))
        else:
            st = lib.clg_decode_host_columns(self._h, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans), C.byref(c))
        cols = self._columns_finish(st, c, arrs, base, [buf[int(o):int(o) + int(k)] for o, k in zip(so, sl)], partial)
        return self._payloads_attach(cols, p, var, pos) if payloads else cols

    # ---- the payload column (clg_payloads)
    def gather_payloads(self, data, span_off, span_len, w_var_off, w_var_len, row_base, device: bool = False,
                        out: Optional[_lib.Payloads] = None):
        """clg_gather_payloads: the payload column of spans data[span_off[s] : + span_len[s]].
        device=False: data, w_var_off and w_var_len are host arrays (staged); device=True: they
        are device addresses (ints).  span_off, span_len and row_base are host arrays.  out: a
        clg_payloads the caller set up (any out_kind; var and pos null: sizes only), filled in
        place, the status returned; None: (var, pos) as host arrays of exactly the batch's sizes."""
        so, sl = np.ascontiguousarray(span_off, np.uint64), np.ascontiguousarray(span_len, np.uint64)
        rb = np.ascontiguousarray(row_base, np.uint64)
        if device:
            dp, wo, wl, kind, keep = int(data or 0), int(w_var_off or 0), int(w_var_len or 0), _lib.CLG_MEM_DEVICE, None
        else:
            buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(
                data, np.uint8)
            keep = (buf, np.ascontiguousarray(w_var_off, np.uint32), np.ascontiguousarray(w_var_len, np.uint32))
            dp, wo, wl, kind = _np_ptr(keep[0]), _np_ptr(keep[1]), _np_ptr(keep[2]), _lib.CLG_MEM_HOST
        call = lambda p: lib.clg_gather_payloads(self._h, dp or None, _np_ptr(so), _np_ptr(sl), so.size, wo or None,  # noqa: E731
                                                 wl or None, _np_ptr(rb), kind, C.byref(p))
        return call(out) if out is not None else _payloads_twice(call)

    def gather_payloads_logs(self, handles, start_epochs, w_var_off, w_var_len, row_base, device: bool = False,
                             out: Optional[_lib.Payloads] = None):
        """clg_gather_payloads_logs: span i is getDeterminants(start_epochs[i]) of log handles[i],
        read in place from the pool (rows, row_base, device and out as gather_payloads)."""
        h, ep = np.ascontiguousarray(handles, np.uint32), np.ascontiguousarray(start_epochs, np.int64)
        rb = np.ascontiguousarray(row_base, np.uint64)
        if device:
            wo, wl, kind, keep = int(w_var_off or 0), int(w_var_len or 0), _lib.CLG_MEM_DEVICE, None
        else:
            keep = (np.ascontiguousarray(w_var_off, np.uint32), np.ascontiguousarray(w_var_len, np.uint32))
            wo, wl, kind = _np_ptr(keep[0]), _np_ptr(keep[1]), _lib.CLG_MEM_HOST
        call = lambda p: lib.clg_gather_payloads_logs(self._h, _np_ptr(h), _np_ptr(ep), h.size, wo or None, wl or None,  # noqa: E731
                                                      _np_ptr(rb), kind, C.byref(p))
        return call(out) if out is not None else _payloads_twice(call)

    def decode_wait(self) -> None:
        """clg_decode_wait: completes the oldest queued asynchronous decode and raises its error."""
        if self._queued and isinstance(self._queued[0], PendingDecode):
            self._queued[0].wait()
            return
        st = lib.clg_decode_wait(self._h)
        if self._queued:
            self._queued.popleft()
        check(st)

    # ---- piggybacked deltas (AbstractDeltaSerializerDeserializer) ---------------------------
    def enrich_batch(self, strategy: int, reqs):
        """enrichWithCausalLogDelta for many channels.  reqs: [(channel, epoch, [(log, send), ...])]
        with the logs in the strategy's iteration order.  Returns [(status, header+deltas bytes)]."""
        logs, flags, creq = [], [], (_lib.EnrichReq * max(1, len(reqs)))()
        for i, (ch, ep, entries) in enumerate(reqs):
            creq[i].consumer, creq[i].epoch, creq[i].first, creq[i].count = _ch(ch), ep, len(logs), len(entries)
            for log, send in entries:
                logs.append(log.handle)
                flags.append(_lib.CLG_DE_SEND if send else 0)
        la, fa = np.array(logs or [0], np.uint32), np.array(flags or [0], np.uint8)
        total = C.c_uint64()
        st = lib.clg_enrich_batch(self._h, strategy, creq, len(reqs), _np_ptr(la), _np_ptr(fa), None, 0,
                                  _lib.CLG_MEM_HOST, C.byref(total))
        if st == _lib.CLG_E_CAPACITY or (st == _lib.CLG_OK and total.value):
            out = np.empty(max(1, total.value), np.uint8)
            check(lib.clg_enrich_batch(self._h, strategy, creq, len(reqs), _np_ptr(la), _np_ptr(fa), _np_ptr(out),
                                       out.size, _lib.CLG_MEM_HOST, C.byref(total)))
        else:
            check(st)
            out = np.zeros(0, np.uint8)
        return [(creq[i].status, out[creq[i].out_off:creq[i].out_off + creq[i].out_len].tobytes())
                for i in range(len(reqs))]

    def process_delta(self, strategy: int, msg: bytes, job: int = 0):
        """processCausalLogDelta: returns (epoch, logs touched in header order, bytes consumed)."""
        buf = np.frombuffer(bytes(msg), np.uint8)
        ep, nl, used = C.c_int64(), C.c_uint32(), C.c_uint64()
        hs = np.zeros(4096, np.uint32)
        check(lib.clg_process_delta(self._h, job, strategy, _np_ptr(buf), len(msg), _lib.CLG_MEM_HOST, C.byref(ep),
                                    _np_ptr(hs), hs.size, C.byref(nl), C.byref(used)))
        return ep.value, [int(h) for h in hs[:min(nl.value, hs.size)]], used.value

    # ---- encode -----------------------------------------------------------------------------
    def encode_batch(self, tag, v0, w_idx=None, w_rc=None, w_v1=None, w_var_off=None, w_var_len=None, w_sub=None,
                     var: bytes = b"") -> bytes:
        """SimpleDeterminantEncoder.encodeTo over a batch, on the GPU: records in the decode's
        SoA layout (the side-table arrays for wide records; w_var_off indexes `var`)."""
        tag = np.ascontiguousarray(tag, np.uint8)
        v0 = np.ascontiguousarray(v0, np.int64)
        nw = 0 if w_idx is None else len(w_idx)
        arr = lambda a, t: np.ascontiguousarray(a if a is not None else np.zeros(0), t)  # noqa: E731
        side = [arr(w_idx, np.uint32), arr(w_rc, np.int32), arr(w_v1, np.int64), arr(w_var_off, np.uint32),
                arr(w_var_len, np.uint32), arr(w_sub, np.uint8)]
        vb = np.frombuffer(bytes(var), np.uint8) if len(var) else np.zeros(1, np.uint8)
        ein = _lib.EncodeIn(_np_ptr(tag), _np_ptr(v0), len(tag), *[_np_ptr(a) for a in side[:6]], nw,
                            _np_ptr(vb), len(var), _lib.CLG_MEM_HOST, 0)
        n_out, bad = C.c_uint64(), C.c_uint64()
        st = lib.clg_encode_batch(self._h, C.byref(ein), None, 0, _lib.CLG_MEM_HOST, C.byref(n_out), C.byref(bad))
        if st not in (_lib.CLG_OK, _lib.CLG_E_CAPACITY):
            err = _lib.ClonosError(st, lib.clg_last_error().decode(errors="replace"))
            err.bad_index = bad.value
            raise err
        out = np.empty(max(1, n_out.value), np.uint8)
        check(lib.clg_encode_batch(self._h, C.byref(ein), _np_ptr(out), out.size, _lib.CLG_MEM_HOST, C.byref(n_out),
                                   C.byref(bad)))
        return out[:n_out.value].tobytes()

    def encode_columns(self, cols: "DecodedColumns", per_span: bool = False, wide: str = "host"):
        """clg_encode_columns: re-encode columns that carry their payload column, on the GPU -- the
        batch's bytes, without the log crossing the link.  The columns go up as they are (no SoA
        rows are rebuilt).  per_span=True: one bytes per span instead of the whole stream.  A
        PackedColumns goes up packed and is unpacked on the device (clg_encode_columns_packed); a bad
        packed input raises ClonosError with bad_what, bad_stream and bad_block.  wide="device"
        (PackedColumns with wide_packed only, else ValueError): the packed wide rows go up packed as
        well and are unpacked on the device (clg_encode_columns_packed_wide); no w_* array and no
        var_pos is built on the host.  wide="host": they are unpacked on the host first."""
        if _wide_route(cols, wide):
            return _encode_packed_wide(lambda *a: lib.clg_encode_columns_packed_wide(self._h, *a), cols, per_span)
        if isinstance(cols, PackedColumns):
            pk, (rest, keep), bad = cols._struct(), _columns_in(cols), _lib.UnpackBad()

            def call(enc):
                st = lib.clg_encode_columns_packed(self._h, C.byref(pk), C.byref(rest), C.byref(enc), C.byref(bad))
                if st != _lib.CLG_OK and bad.what != _lib.UNPACK_BAD_NONE:
                    raise _unpack_error(st, bad, enc)
                return st
            return _encode_twice(call, cols.n_spans, per_span)
        cin, keep = _columns_in(cols)
        return _encode_twice(lambda enc: lib.clg_encode_columns(self._h, C.byref(cin), C.byref(enc)), cols.n_spans,
                             per_span)

    def encode_columns_raw(self, cin: _lib.ColumnsIn, enc: _lib.Encoded) -> int:
        """clg_encode_columns over a clg_columns_in and a clg_encoded the caller set up (any in_kind
        and out_kind; enc.bytes null: sizes only).  Returns the status; the results are in enc."""
        return lib.clg_encode_columns(self._h, C.byref(cin), C.byref(enc))

    def append_columns(self, logs, epochs: Sequence[int], cols: "DecodedColumns", statuses: bool = False,
                       wide: str = "host"):
        """clg_append_columns: encode cols on the device and append span s to logs[s] (a
        ThreadCausalLog or a handle) in epochs[s], as one appendDeterminant batch each, without an
        encoded byte crossing the link.  Returns the per-span byte counts; a span that could not be
        applied raises its status after the others were applied, or, with statuses=True, nothing
        raises for a span and (byte counts, statuses) is returned.  wide: as encode_columns'
        (clg_append_columns_packed_wide)."""
        device_wide = _wide_route(cols, wide)
        h = np.array([getattr(l, "handle", l) for l in logs], np.uint32)
        ep = np.ascontiguousarray(epochs, np.int64)
        ns = max(cols.n_spans, 1)
        if len(h) != ns or len(ep) != ns:
            raise ValueError(f"{len(h)} logs and {len(ep)} epochs for {ns} spans")
        nb, st = np.zeros(ns, np.uint64), np.zeros(ns, np.int32)
        if device_wide:  # both packed forms go up packed
            pk, pw, (rest, keep), bad = cols._struct(), cols.wide_packed._struct(), _rest_in(cols), _lib.UnpackBad()
            rc = lib.clg_append_columns_packed_wide(self._h, _np_ptr(h), _np_ptr(ep), ns, C.byref(pk), C.byref(pw),
                                                    C.byref(rest), _np_ptr(nb), _np_ptr(st), C.byref(bad))
            if rc != _lib.CLG_OK:
                raise _unpack_error(rc, bad)
        elif isinstance(cols, PackedColumns):  # goes up packed, unpacked on the device
            pk, (rest, keep), bad = cols._struct(), _columns_in(cols), _lib.UnpackBad()
            rc = lib.clg_append_columns_packed(self._h, _np_ptr(h), _np_ptr(ep), ns, C.byref(pk), C.byref(rest), _np_ptr(nb),
                                               _np_ptr(st), C.byref(bad))
            if rc != _lib.CLG_OK:
                raise _unpack_error(rc, bad)
        else:
            cin, keep = _columns_in(cols)
            check(lib.clg_append_columns(self._h, _np_ptr(h), _np_ptr(ep), ns, C.byref(cin), _np_ptr(nb), _np_ptr(st)))
        if statuses:
            return nb, st
        for s in range(ns):
            if st[s] != _lib.CLG_OK:
                err = ClonosError(int(st[s]), f"span {s} was not appended")
                err.span, err.statuses, err.span_bytes = s, st, nb
                raise err
        return nb

    def encode_decoded(self, dec: "DecodedBatch", span_bytes: bytes) -> bytes:
        """Round trip: re-encode a decoded span (its var fields index the span bytes)."""
        return self.encode_batch(dec.tag, dec.v0, dec.w_idx, dec.w_rc, dec.w_v1, dec.w_var_off, dec.w_var_len,
                                 dec.w_sub, span_bytes)

    # ---- replay-prep ----------------------------------------------------------------------
    def replay_prep(self, copies: Sequence[Tuple[int, bytes]]):
        """DeterminantResponseEvent.merge (longest wins, ties -> later) + batched decode of
        the winners.  Returns (winner indices, DecodedBatch over the winners)."""
        keys = np.array([c[0] for c in copies], np.uint64)
        blobs = [bytes(c[1]) for c in copies]
        offs = np.zeros(len(blobs), np.uint64)
        lens = np.array([len(b) for b in blobs], np.uint64)
        if len(blobs):
            offs[1:] = np.cumsum(lens)[:-1]
        data = np.frombuffer(b"".join(blobs) or b"\0", np.uint8)
        winner = np.zeros(max(len(blobs), 1), np.uint32)
        nk = C.c_uint32()
        total = int(lens.sum())
        d, arrs, _ = self._pooled_outputs(total // 2 + len(blobs) + 1, total // 6 + len(blobs) + 1)
        base = np.zeros(len(blobs) + 1, np.uint64)
        st = lib.clg_replay_prep(self._h, _np_ptr(keys), _np_ptr(data), _np_ptr(offs), _np_ptr(lens), len(blobs),
                                 _np_ptr(winner), C.byref(nk), C.byref(d), _np_ptr(base))
        k = nk.value
        win = winner[:k].copy()
        return win, self._finish(st, d, arrs, base, k, [np.frombuffer(blobs[i], np.uint8) for i in win])

    # ---- log digests (clg_digest_*) -----------------------------------------------------------
    def digest_logs(self, handles, start_epochs) -> np.ndarray:
        """Digest of getDeterminants(start_epochs[i]) of log handles[i], computed where the bytes
        live: a DIGEST row per request (16 bytes each come back).  Handles may repeat."""
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        if h.shape != ep.shape or h.ndim != 1:
            raise ValueError("handles and start_epochs must be 1-d and of equal length")
        out = np.zeros(h.size, DIGEST)
        if h.size:
            check(lib.clg_digest_logs(self._h, _np_ptr(h), _np_ptr(ep), h.size, _np_ptr(out)))
        return out

    def digest_spans(self, data_or_ptr, offs, lens, device: bool = False) -> np.ndarray:
        """Digest of span i = bytes[offs[i], offs[i] + lens[i]) of host bytes (bytes / uint8
        array) or, with device=True, of device memory at the address data_or_ptr."""
        so = np.ascontiguousarray(offs, np.uint64)
        sl = np.ascontiguousarray(lens, np.uint64)
        if so.shape != sl.shape or so.ndim != 1:
            raise ValueError("offs and lens must be 1-d and of equal length")
        out = np.zeros(so.size, DIGEST)
        if not so.size:
            return out
        if device:
            ptr, kind, keep = int(data_or_ptr), _lib.CLG_MEM_DEVICE, None
        else:
            keep = (np.ascontiguousarray(data_or_ptr, np.uint8) if isinstance(data_or_ptr, np.ndarray)
                    else np.frombuffer(bytes(data_or_ptr), np.uint8))
            if sl.size and int((so + sl).max()) > keep.size:
                raise ValueError("span outside the data")
            ptr, kind = (keep.ctypes.data if keep.size else None), _lib.CLG_MEM_HOST
        check(lib.clg_digest_spans(self._h, ptr, _np_ptr(so), _np_ptr(sl), so.size, kind, _np_ptr(out)))
        return out

    def digest_prefixes(self, handles, start_epochs, cuts) -> Tuple[np.ndarray, np.ndarray]:
        """Digest of getDeterminants(start_epochs[i]) of log handles[i] at each of its cuts, the
        range read once: cuts is a list of arrays (one per request, not decreasing) or a
        (first, flat) tuple.  Returns (rows, first): DIGEST row k, first[i] <= k < first[i + 1],
        is the digest of the first min(cut, len) bytes of request i's range.  The holder of a
        longer copy checks with it that a shorter copy is a prefix: its own row at the other
        side's length must equal the other side's whole digest."""
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        if h.shape != ep.shape or h.ndim != 1:
            raise ValueError("handles and start_epochs must be 1-d and of equal length")
        first, flat = _flat_cuts(cuts, h.size)
        out = np.zeros(flat.size, DIGEST)
        check(lib.clg_digest_prefixes(self._h, _np_ptr(h), _np_ptr(ep), h.size, _np_ptr(first), _np_ptr(flat),
                                      _np_ptr(out)))
        return out, first

    def digest_epochs(self, handles, start_epochs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Digests at the range's own epoch ends: (first, epoch_ids, rows); rows first[i] ..
        first[i + 1] are request i's, one per epoch of its range in order, each the digest of the
        range up to that epoch's end (the last is digest_logs' row).  Two copies of a log part
        in the first epoch whose rows differ."""
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        if h.shape != ep.shape or h.ndim != 1:
            raise ValueError("handles and start_epochs must be 1-d and of equal length")
        first = np.zeros(h.size + 1, np.uint64)
        total = C.c_uint64(0)
        check(lib.clg_digest_epochs(self._h, _np_ptr(h), _np_ptr(ep), h.size, 0, _np_ptr(first), None, None,
                                    C.byref(total)))
        ids = np.zeros(total.value, np.int64)
        out = np.zeros(total.value, DIGEST)
        if total.value:
            check(lib.clg_digest_epochs(self._h, _np_ptr(h), _np_ptr(ep), h.size, total.value, _np_ptr(first),
                                        _np_ptr(ids), _np_ptr(out), C.byref(total)))
        return first, ids, out

    # ---- log comparison (clg_diff_logs) -------------------------------------------------------
    def diff_logs(self, handles, start_epochs, data_or_ptr, offs, lens, device: bool = False) -> np.ndarray:
        """Longest common prefix of getDeterminants(start_epochs[i]) of log handles[i] and the
        reference span i = bytes[offs[i], offs[i] + lens[i]) of host bytes (bytes / uint8 array)
        or, with device=True, of device memory at the address data_or_ptr: a DIFF row
        (lcp, len_log, len_ref) per request (24 bytes each come back).  Handles may repeat."""
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        so = np.ascontiguousarray(offs, np.uint64)
        sl = np.ascontiguousarray(lens, np.uint64)
        if h.ndim != 1 or not (h.shape == ep.shape == so.shape == sl.shape):
            raise ValueError("handles, start_epochs, offs and lens must be 1-d and of equal length")
        out = np.zeros(h.size, DIFF)
        if not h.size:
            return out
        if device:
            ptr, kind, keep = int(data_or_ptr), _lib.CLG_MEM_DEVICE, None
        else:
            keep = (np.ascontiguousarray(data_or_ptr, np.uint8) if isinstance(data_or_ptr, np.ndarray)
                    else np.frombuffer(bytes(data_or_ptr), np.uint8))
            if int((so + sl).max()) > keep.size:
                raise ValueError("span outside the data")
            ptr, kind = (keep.ctypes.data if keep.size else None), _lib.CLG_MEM_HOST
        check(lib.clg_diff_logs(self._h, _np_ptr(h), _np_ptr(ep), h.size, ptr, _np_ptr(so), _np_ptr(sl), kind,
                                _np_ptr(out)))
        return out

    # ---- instrumentation ---------------------------------------------------------------------
    def kernel_stats(self):
        arr = (_lib.KernelStat * 64)()
        n = C.c_uint32()
        check(lib.clg_kernel_stats(self._h, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): dict(launches=arr[i].launches, ms=arr[i].total_ms, bytes=arr[i].bytes)
                for i in range(min(n.value, 64))}

    def kernel_stats_reset(self):
        check(lib.clg_kernel_stats_reset(self._h))


class PendingDecode:
    """A queued clg_decode_logs_async; holds the output arrays until wait().  The engine
    completes its queued decodes in order (clg_decode_wait is FIFO): waiting for this one
    first waits for the ones queued before it, whose results (or errors) they keep."""

    def __init__(self, engine: "Engine", keep, n_spans: int):
        self._e, self._keep, self._n = engine, keep, n_spans
        self._done = False
        self._res = None  # (result, exception)

    def _complete(self) -> None:
        q = self._e._queued
        assert q and q[0] is self
        st = lib.clg_decode_wait(self._e._h)
        q.popleft()
        self._done = True
        _, _, d, arrs, base = self._keep
        try:
            self._res = (self._e._finish(st, d, arrs, base, self._n, None), None)
        except ClonosError as ex:
            self._res = (None, ex)

    def wait(self) -> DecodedBatch:
        while not self._done:
            head = self._e._queued[0]
            if isinstance(head, PendingDecode):
                head._complete()
            else:  # an earlier device-output decode: its status is its own caller's to take
                raise RuntimeError("an earlier decode_logs_device_async is not waited for (decode_wait)")
        res, ex = self._res
        if ex is not None:
            raise ex
        return res


class ThreadCausalLog:
    """Mirror of ThreadCausalLog (ThreadCausalLog.java:33-96) backed by the engine."""

    def __init__(self, engine: Engine, handle: int, cid: CausalLogID, job: int = 0):
        self.engine = engine
        self.handle = handle
        self.cid = cid
        self.job = job

    def getCausalLogID(self) -> CausalLogID:
        return self.cid

    def appendDeterminant(self, det: Union[D.Determinant, bytes], epochID: int) -> None:
        b = det if isinstance(det, (bytes, bytearray)) else D.encode(det)
        check(lib.clg_append(self.engine.handle, self.handle, epochID, bytes(b), len(b)))

    def processUpstreamDelta(self, delta: bytes, offsetFromEpoch: int, epochID: int) -> None:
        check(lib.clg_upstream_delta(self.engine.handle, self.handle, epochID, offsetFromEpoch, bytes(delta),
                                     len(delta)))

    def logLength(self) -> int:
        v = C.c_int32()
        check(lib.clg_log_length(self.engine.handle, self.handle, C.byref(v)))
        return v.value

    def hasDeltaForConsumer(self, outputChannelID: ChannelLike, epochID: int) -> bool:
        v = C.c_int32()
        check(lib.clg_has_delta(self.engine.handle, self.handle, _ch(outputChannelID), epochID, C.byref(v)))
        return bool(v.value)

    def getOffsetFromEpochForConsumer(self, outputChannelID: ChannelLike, epochID: int) -> int:
        v = C.c_int32()
        check(lib.clg_offset_from_epoch(self.engine.handle, self.handle, _ch(outputChannelID), C.byref(v)))
        return v.value

    @staticmethod
    def _probe_fetch(call) -> bytes:
        """Size probe, then fetch; CLG_E_CAPACITY (the log grew in between: another thread
        appended) reports the new size without moving anything, so fetch again."""
        n = C.c_uint32()
        st = call(None, 0, C.byref(n))
        buf = np.empty(1, np.uint8)
        while st == _lib.CLG_E_CAPACITY:
            buf = np.empty(n.value + 256, np.uint8)
            st = call(_np_ptr(buf), buf.size, C.byref(n))
        check(st)
        return buf[:n.value].tobytes()

    def getDeltaForConsumer(self, outputChannelID: ChannelLike, epochID: int) -> bytes:
        ch = _ch(outputChannelID)
        return self._probe_fetch(lambda p, cap, n: lib.clg_get_delta(self.engine.handle, self.handle, ch, epochID, p,
                                                                     cap, _lib.CLG_MEM_HOST, n))

    def determinants_length(self, startEpochID: int) -> int:
        """len(getDeterminants(startEpochID)) without moving bytes."""
        n = C.c_uint32()
        st = lib.clg_get_determinants(self.engine.handle, self.handle, startEpochID, None, 0, _lib.CLG_MEM_HOST,
                                      C.byref(n))
        if st not in (_lib.CLG_OK, _lib.CLG_E_CAPACITY):
            check(st)
        return n.value

    def determinants_into(self, startEpochID: int, dev_ptr: int, cap: int) -> int:
        """getDeterminants(startEpochID) gathered into device memory (engine's device)."""
        n = C.c_uint32()
        check(lib.clg_get_determinants(self.engine.handle, self.handle, startEpochID, dev_ptr, cap,
                                       _lib.CLG_MEM_DEVICE, C.byref(n)))
        return n.value

    def getDeterminants(self, startEpochID: int) -> bytes:
        return self._probe_fetch(lambda p, cap, n: lib.clg_get_determinants(self.engine.handle, self.handle,
                                                                            startEpochID, p, cap, _lib.CLG_MEM_HOST,
                                                                            n))

    def notifyCheckpointComplete(self, checkpointID: int) -> None:
        check(lib.clg_notify_checkpoint_complete(self.engine.handle, self.handle, checkpointID))

    def unregisterConsumer(self, toCancel: ChannelLike) -> None:
        check(lib.clg_unregister_consumer(self.engine.handle, self.handle, _ch(toCancel)))

    def close(self) -> None:
        check(lib.clg_log_close(self.engine.handle, self.handle))
        self.engine._logs.pop((self.job, self.cid.key()), None)

    # ---- introspection (tests / safety assertions) ----
    def state(self) -> dict:
        st = _lib.LogState()
        ids = np.zeros(4096, np.int64)
        offs = np.zeros(4096, np.int32)
        check(lib.clg_log_get_state(self.engine.handle, self.handle, C.byref(st), _np_ptr(ids), _np_ptr(offs), 4096))
        n = st.n_epochs
        return dict(writer=st.writer, capacity=st.capacity, n_components=st.n_components,
                    epochs=list(zip(ids[:n].tolist(), offs[:n].tolist())))

    def consumer_state(self, ch: ChannelLike):
        ex, ep, off = C.c_int32(), C.c_int64(), C.c_int32()
        check(lib.clg_consumer_state(self.engine.handle, self.handle, _ch(ch), C.byref(ex), C.byref(ep), C.byref(off)))
        return (ep.value, off.value) if ex.value else None

    def seek_consumer(self, ch: ChannelLike, epoch: int, offset: int) -> None:
        check(lib.clg_consumer_seek(self.engine.handle, self.handle, _ch(ch), epoch, offset))

    def read_phys(self, phys: int, n: int) -> bytes:
        buf = np.empty(max(n, 1), np.uint8)
        check(lib.clg_log_read_phys(self.engine.handle, self.handle, phys, n, _np_ptr(buf)))
        return buf[:n].tobytes()
