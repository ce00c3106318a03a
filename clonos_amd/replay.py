"""Host-side mirror of DeterminantResponseEvent and of the replay preparation done by the
recovery states, on top of the C-ABI (libclonos_engine.so).

  DeterminantResponseEvent  reference flink-runtime/.../causal/DeterminantResponseEvent.java:36-148
                            (write :93-107, read :109-125, merge :128-148) -> clg_response_*
  WaitingDeterminantsState  .../causal/recovery/WaitingDeterminantsState.java:57,97-108
                            (accumulator (found=true, vertex), merge every direct response)
  ReplayingState            .../causal/recovery/ReplayingState.java:58-214 and
  LogReplayerImpl           .../causal/recovery/LogReplayerImpl.java:51-158
                            -> clg_replay_prepare (main logs decoded on the GPU; subpartition
                               recovery buffers turned into BufferBuilt size lists on the GPU)

The event's map keeps java.util.HashMap iteration order (see include/clonos_engine.h), so
write() produces the reference's bytes.  Entries reference Python-owned byte buffers that
this object keeps alive.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import time

import numpy as np

from . import _lib
from ._lib import check, lib
from . import determinants as D
from .engine import (CausalLogID, DecodedBatch, DecodedColumns, Engine, ThreadCausalLog, _columns_struct, _np_ptr,
                     _payloads_struct, _wide_determinant)


# numpy views of the C structs (include/clonos_engine.h)
LOG_ID = np.dtype([("vertex_id", "<i2"), ("is_main", "u1"), ("subpartition", "i1"), ("reserved", "<u4"),
                   ("irp_lower", "<i8"), ("irp_upper", "<i8")])
ENTRY = np.dtype([("id", LOG_ID), ("bytes", "<u8"), ("len", "<u8")])
assert LOG_ID.itemsize == C.sizeof(_lib.CausalLogIdC) and ENTRY.itemsize == C.sizeof(_lib.ResponseEntry)


def log_id_array(ids: Sequence[CausalLogID]) -> np.ndarray:
    """CausalLogIDs as a packed clg_causal_log_id array."""
    a = np.zeros(len(ids), LOG_ID)
    for i, c in enumerate(ids):
        a[i] = (c.vertex_id, 1 if c.is_main else 0, 0 if c.is_main else c.subpartition, 0,
                0 if c.is_main else c.irp_lower, 0 if c.is_main else c.irp_upper)
    return a


def table_ids(table) -> np.ndarray:
    """The job's log table (job.LogTable) as a clg_causal_log_id array, built once per table."""
    arr = getattr(table, "_c_ids", None)
    if arr is None:
        arr = log_id_array(table.ids)
        table._c_ids = arr
    return arr


def _from_c(c: _lib.CausalLogIdC) -> CausalLogID:
    if c.is_main:
        return CausalLogID.main(c.vertex_id)
    return CausalLogID.sub(c.vertex_id, c.irp_lower, c.irp_upper, c.subpartition)


def causal_log_id_hash(lid: CausalLogID) -> int:
    """CausalLogID.hashCode (CausalLogID.java:151-163)."""
    c = lid.to_c()
    return lib.clg_causal_log_id_hash(C.byref(c))


class DeterminantResponseEvent:
    """DeterminantResponseEvent (found, vertexID, correlationID, Map<CausalLogID, ByteBuf>)."""

    def __init__(self, found: bool = False, vertex_id: int = 0, correlation_id: int = 0, capacity: int = 256):
        self._entries = (_lib.ResponseEntry * max(1, capacity))()
        self._c = _lib.Response(1 if found else 0, vertex_id, 0, correlation_id, 0, capacity, 0, 0, self._entries)
        self._keep: List[object] = []  # buffers the entries point into
        self._bytes: Optional[Tuple[int, int]] = None  # (main log bytes, all bytes) when known (merged_responses)

    # ---- accessors (:71-89)
    def isFound(self) -> bool:
        return bool(self._c.found)

    def getVertexID(self) -> int:
        return int(self._c.vertex_id)

    def getCorrelationID(self) -> int:
        return int(self._c.correlation_id)

    def setCorrelationID(self, v: int) -> None:
        self._c.correlation_id = v

    def getDeterminants(self) -> Dict[CausalLogID, bytes]:
        """The map, in java.util.HashMap iteration order."""
        out = {}
        for i in range(self._c.n):
            e = self._entries[i]
            out[_from_c(e.id)] = C.string_at(e.bytes, e.len) if e.len else b""
        return out

    def __len__(self) -> int:
        return int(self._c.n)

    def _grow(self, need: int) -> None:
        if need <= self._c.cap:
            return
        cap = max(need, 2 * self._c.cap)
        new = (_lib.ResponseEntry * cap)()
        C.memmove(new, self._entries, C.sizeof(_lib.ResponseEntry) * self._c.n)
        self._entries, self._c.entries, self._c.cap = new, new, cap

    # ---- map building (JobCausalLogImpl.respondToDeterminantRequest :197-199)
    def put(self, lid: CausalLogID, data: bytes) -> None:
        self._bytes = None
        buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._keep.append(buf)
        self._grow(self._c.n + 1)
        c = lid.to_c()
        check(lib.clg_response_put(C.byref(self._c), C.byref(c), _np_ptr(buf), len(data)))

    def put_device(self, lid: CausalLogID, ptr: int, n: int, keep=None) -> None:
        """An entry whose bytes live in device memory (replay-prep over a cross-GPU merge's
        receive buffer, clg_replay_prepare_device); `keep` is held while the event lives."""
        self._bytes = None
        if keep is not None:
            self._keep.append(keep)
        self._grow(self._c.n + 1)
        c = lid.to_c()
        check(lib.clg_response_put(C.byref(self._c), C.byref(c), C.c_void_p(ptr), n))

    def put_device_batch(self, ids: np.ndarray, ptrs: np.ndarray, lens: np.ndarray, keep=None) -> None:
        """Many device-memory entries in one call (clg_response_put_batch); ids: LOG_ID array."""
        if keep is not None:
            self._keep.append(keep)
        self._bytes = None
        n = len(ids)
        self._grow(self._c.n + n)
        ids = np.ascontiguousarray(ids, LOG_ID)
        ptrs = np.ascontiguousarray(ptrs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        self._keep.extend((ids, ptrs, lens))
        check(lib.clg_response_put_batch(C.byref(self._c), ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data, n))

    def entries(self) -> np.ndarray:
        """The map's entries as an ENTRY array view (iteration order)."""
        if not self._c.n:
            return np.zeros(0, ENTRY)
        return np.frombuffer((C.c_char * (ENTRY.itemsize * self._c.n)).from_address(C.addressof(self._entries)),
                             ENTRY, self._c.n)

    # ---- wire format
    def write(self) -> bytes:
        n = C.c_uint64()
        st = lib.clg_response_write(C.byref(self._c), None, 0, C.byref(n))
        if st not in (_lib.CLG_OK, _lib.CLG_E_CAPACITY):
            check(st)
        out = np.empty(max(1, n.value), np.uint8)
        check(lib.clg_response_write(C.byref(self._c), _np_ptr(out), n.value, C.byref(n)))
        return out[:n.value].tobytes()

    @staticmethod
    def read(data: bytes) -> Tuple["DeterminantResponseEvent", int]:
        buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(0, np.uint8)
        ev = DeterminantResponseEvent(capacity=max(1, len(data) // 7 + 1))
        ev._keep.append(buf)
        used = C.c_uint64()
        check(lib.clg_response_read(_np_ptr(buf) if buf.size else None, len(data), C.byref(ev._c), C.byref(used)))
        return ev, int(used.value)

    def merge(self, other: "DeterminantResponseEvent") -> None:
        self._bytes = None
        self._grow(self._c.n + other._c.n)
        self._keep.extend(other._keep)
        check(lib.clg_response_merge(C.byref(self._c), C.byref(other._c)))


def accumulate(vertex_id: int, responses: Sequence[DeterminantResponseEvent]) -> DeterminantResponseEvent:
    """WaitingDeterminantsState: new DeterminantResponseEvent(true, vertex) (:57), then merge
    every direct response in arrival order (:102)."""
    acc = DeterminantResponseEvent(True, vertex_id)
    for r in responses:
        acc.merge(r)
    return acc


@dataclass
class SubpartitionReplay:
    """What SubpartitionRecoveryThread.run (ReplayingState.java:157-214) would rebuild."""
    log_id: CausalLogID
    buffer_sizes: np.ndarray  # buildAndLogBuffer(n) arguments, in order
    status: int               # CLG_OK or the error the thread hits after those buffers
    err_off: int
    err_tag: int


@dataclass
class VertexReplay:
    vertex_id: int
    main: DecodedBatch          # LogReplayerImpl's record sequence (span 0 of this batch view)
    main_slice: slice
    subpartitions: List[SubpartitionReplay]


def merged_responses(merged, table, vertices: Sequence[int]) -> Dict[int, DeterminantResponseEvent]:
    """The accumulated responses of failed vertices whose copies arrived by the cross-GPU merge
    (dist.merge_responses): entries point into the merge's receive buffer, in HBM under RCCL
    (prepare_replay(..., device_input=True)).  One batched put per vertex."""
    gids = np.asarray(merged.gids, np.int64)
    ids = table_ids(table)
    # the entries grouped by vertex once (a stable sort keeps each vertex's entries in the
    # merge's order), then one contiguous slice per vertex
    vert = table.vertex[gids] if len(gids) else np.zeros(0, np.int64)
    order = np.argsort(vert, kind="stable")
    vs = vert[order]
    # (rows moved as raw words: fancy indexing the structured array took 0.13 ms for 2 k rows)
    ids_o = np.take(ids.view(np.uint64).reshape(len(ids), -1), gids[order], axis=0).view(LOG_ID).reshape(-1)
    ptr_o = np.ascontiguousarray(np.asarray(merged.offs, np.uint64)[order] + np.uint64(merged.buf.data_ptr()))
    len_o = np.ascontiguousarray(np.asarray(merged.lens, np.uint64)[order])
    out = {}
    va = np.asarray(list(vertices), np.int64)
    lo_a = np.searchsorted(vs, va, "left")
    hi_a = np.searchsorted(vs, va, "right")
    los, his = lo_a.tolist(), hi_a.tolist()
    # each vertex's byte totals, for prepare_replay_raw's output sizes (prefix sums, once)
    c_all = np.zeros(len(len_o) + 1, np.uint64)
    np.cumsum(len_o, out=c_all[1:])
    c_main = np.zeros(len(len_o) + 1, np.uint64)
    np.cumsum(np.where(ids_o["is_main"] != 0, len_o, np.uint64(0)), out=c_main[1:])
    t_all = (c_all[hi_a] - c_all[lo_a]).tolist()
    t_main = (c_main[hi_a] - c_main[lo_a]).tolist()
    # one put per vertex into the three arrays above (pointer arithmetic, no per-vertex views)
    pi, pp, pl, isz = ids_o.ctypes.data, ptr_o.ctypes.data, len_o.ctypes.data, ids_o.itemsize
    keep = (merged.buf, ids_o, ptr_o, len_o)
    for v, lo, hi, tm, ta in zip(va.tolist(), los, his, t_main, t_all):
        ev = DeterminantResponseEvent(True, v, capacity=max(1, hi - lo))
        if hi > lo:
            ev._keep.append(keep)
            check(lib.clg_response_put_batch(C.byref(ev._c), pi + lo * isz, pp + lo * 8, pl + lo * 8, hi - lo))
        ev._bytes = (tm, ta)
        out[v] = ev
    return out


def merged_response(vertex_id: int, merged, table) -> DeterminantResponseEvent:
    """merged_responses for one vertex."""
    return merged_responses(merged, table, [vertex_id])[vertex_id]


@dataclass
class ReplayArrays:
    """clg_replay_prepare's outputs as arrays (prepare_replay_raw): per subpartition (global
    order: vertex order, then table order) its size list is sizes[base[j] : base[j] + count[j]]."""
    main: DecodedBatch
    sizes: np.ndarray
    base: np.ndarray
    count: np.ndarray
    status: np.ndarray
    err_off: np.ndarray
    err_tag: np.ndarray


def prepare_replay_raw(engine: Engine, jobs: Sequence[Tuple[int, DeterminantResponseEvent, np.ndarray]],
                       device_input: bool = False, timing: Optional[Dict[str, float]] = None) -> ReplayArrays:
    """clg_replay_prepare over jobs (vertex_id, merged response, subpartition table as a
    LOG_ID array in the task's order), without per-subpartition Python objects.  timing:
    (developer) seconds added per part -- build, alloc, call, finish."""
    t0 = time.perf_counter()
    n = len(jobs)
    vs = (_lib.ReplayVertex * max(1, n))()
    tables = []
    main_bytes, sub_bytes, n_sub = 0, 0, 0
    for i, (vid, acc, subs) in enumerate(jobs):
        t = np.ascontiguousarray(subs, LOG_ID)
        tables.append(t)
        n_sub += len(t)
        vs[i] = _lib.ReplayVertex(C.pointer(acc._c), C.cast(t.ctypes.data, C.POINTER(_lib.CausalLogIdC)), len(t), vid, 0)
        if acc._bytes is not None:
            mb, ab = acc._bytes
        else:
            e = acc.entries()
            ln = e["len"]
            mb, ab = int(ln[e["id"]["is_main"] != 0].sum()), int(ln.sum())
        main_bytes += mb
        sub_bytes += ab - mb  # a bound: the table may name fewer
    t1 = time.perf_counter()
    cap = main_bytes // 2 + n + 1
    d, arrs, _ = engine._pooled_outputs(cap, main_bytes // 6 + n + 1)
    base = np.zeros(n + 1, np.uint64)
    sizes = np.empty(max(1, sub_bytes // 5), np.int32)
    sbase = np.zeros(n_sub + 1, np.uint64)
    cnt = np.zeros(max(1, n_sub), np.uint64)
    sst = np.zeros(max(1, n_sub), np.int32)
    soff = np.zeros(max(1, n_sub), np.int64)
    stag = np.zeros(max(1, n_sub), np.int32)
    out = _lib.ReplayOut(C.pointer(d), _np_ptr(base), _np_ptr(sizes), sizes.size, _np_ptr(sbase), _np_ptr(cnt),
                         _np_ptr(sst), _np_ptr(soff), _np_ptr(stag))
    fn = lib.clg_replay_prepare_device if device_input else lib.clg_replay_prepare
    t2 = time.perf_counter()
    st = fn(engine.handle, vs, n, C.byref(out))
    t3 = time.perf_counter()
    main = engine._finish(st, d, arrs, base, n, None)
    res = ReplayArrays(main, sizes, sbase[:n_sub], cnt[:n_sub], sst[:n_sub], soff[:n_sub], stag[:n_sub])
    if timing is not None:
        for k, v in (("build", t1 - t0), ("alloc", t2 - t1), ("call", t3 - t2), ("finish", time.perf_counter() - t3)):
            timing[k] = timing.get(k, 0.0) + v
    return res


def prepare_replay(engine: Engine, jobs: Sequence[Tuple[int, DeterminantResponseEvent, Sequence[CausalLogID]]],
                   device_input: bool = False) -> Tuple[DecodedBatch, List[VertexReplay]]:
    """ReplayingState construction for a batch of failed vertices: jobs are
    (vertex_id, merged response, subpartition table in the task's order).  device_input:
    the responses' bytes are in device memory (clg_replay_prepare_device)."""
    n = len(jobs)
    vs = (_lib.ReplayVertex * max(1, n))()
    tables = []
    main_bytes, sub_bytes = 0, 0
    for i, (vid, acc, subs) in enumerate(jobs):
        t = (_lib.CausalLogIdC * max(1, len(subs)))(*[s.to_c() for s in subs])
        tables.append(t)
        vs[i] = _lib.ReplayVertex(C.pointer(acc._c), t, len(subs), vid, 0)
        sizes_of = {_from_c(acc._entries[k].id): int(acc._entries[k].len) for k in range(acc._c.n)}
        main_bytes += sizes_of.get(CausalLogID.main(vid), 0)
        sub_bytes += sum(sizes_of.get(CausalLogID.sub(vid, s.irp_lower, s.irp_upper, s.subpartition), 0)
                         for s in subs)
    n_sub = sum(len(j[2]) for j in jobs)
    cap = main_bytes // 2 + n + 1
    d, arrs, _ = engine._pooled_outputs(cap, main_bytes // 6 + n + 1)
    base = np.zeros(n + 1, np.uint64)
    sizes = np.empty(max(1, sub_bytes // 5), np.int32)
    sbase = np.zeros(n_sub + 1, np.uint64)
    cnt = np.zeros(max(1, n_sub), np.uint64)
    sst = np.zeros(max(1, n_sub), np.int32)
    soff = np.zeros(max(1, n_sub), np.int64)
    stag = np.zeros(max(1, n_sub), np.int32)
    out = _lib.ReplayOut(C.pointer(d), _np_ptr(base), _np_ptr(sizes), sizes.size, _np_ptr(sbase), _np_ptr(cnt),
                         _np_ptr(sst), _np_ptr(soff), _np_ptr(stag))
    fn = lib.clg_replay_prepare_device if device_input else lib.clg_replay_prepare
    st = fn(engine.handle, vs, n, C.byref(out))
    main = engine._finish(st, d, arrs, base, n, None)
    res, j = [], 0
    for i, (vid, acc, subs) in enumerate(jobs):
        sp = []
        for s in subs:
            lid = CausalLogID.sub(vid, s.irp_lower, s.irp_upper, s.subpartition)
            b0 = int(sbase[j])
            sp.append(SubpartitionReplay(lid, sizes[b0:b0 + int(cnt[j])].copy(), int(sst[j]), int(soff[j]),
                                         int(stag[j])))
            j += 1
        res.append(VertexReplay(vid, main, main.span_slice(i), sp))
    return main, res


@dataclass
class ReplayColumns:
    """clg_replay_prepare_columns' outputs (prepare_replay_columns): the main logs as typed
    columns (span i = job i; with payloads main.var / main.var_pos / main.payload(k)), and
    ReplayArrays' subpartition arrays.  A decode error in a main log is in main.error; the
    columns then hold each vertex's records up to its first error."""
    main: DecodedColumns
    sizes: np.ndarray
    base: np.ndarray
    count: np.ndarray
    status: np.ndarray
    err_off: np.ndarray
    err_tag: np.ndarray
    vertex_ids: List[int]
    tables: List[np.ndarray]  # per job its subpartition table (LOG_ID)

    def replayer(self, i: int) -> "ColumnReplayer":
        """LogReplayerImpl's cursor over job i's main log."""
        return ColumnReplayer(self.main, i)

    def vertex(self, i: int) -> List[SubpartitionReplay]:
        """Job i's subpartitions, as prepare_replay gives them."""
        j = sum(len(t) for t in self.tables[:i])
        out = []
        for s in self.tables[i]:
            lid = CausalLogID.sub(self.vertex_ids[i], int(s["irp_lower"]), int(s["irp_upper"]), int(s["subpartition"]))
            b0 = int(self.base[j])
            out.append(SubpartitionReplay(lid, self.sizes[b0:b0 + int(self.count[j])].copy(), int(self.status[j]),
                                          int(self.err_off[j]), int(self.err_tag[j])))
            j += 1
        return out


def prepare_replay_columns(engine: Engine, jobs: Sequence[Tuple[int, DeterminantResponseEvent, Sequence]],
                           device_input: bool = False, payloads: bool = True, packed: bool = False,
                           pack_wide: bool = False) -> ReplayColumns:
    """clg_replay_prepare_columns over jobs (vertex_id, merged response, subpartition table: a
    LOG_ID array or a sequence of CausalLogID, in the task's order): prepare_replay with the main
    logs delivered as typed columns and, with payloads, the wide rows' payload bytes -- one engine
    call.  device_input: the responses' bytes are in device memory.  packed=True
    (clg_replay_prepare_columns_packed): `main` is a PackedColumns, the five narrow columns
    bit-packed; pack_wide=True with it: the wide rows come packed by kind too (main.wide_packed).
    replayer(i) pops from either as it does from plain columns."""
    if pack_wide and not packed:
        raise ValueError("pack_wide needs packed=True")
    n = len(jobs)
    vs = (_lib.ReplayVertex * max(1, n))()
    tables = []
    main_bytes, sub_bytes, n_sub = 0, 0, 0
    for i, (vid, acc, subs) in enumerate(jobs):
        t = np.ascontiguousarray(subs, LOG_ID) if isinstance(subs, np.ndarray) else log_id_array(list(subs))
        tables.append(t)
        n_sub += len(t)
        vs[i] = _lib.ReplayVertex(C.pointer(acc._c), C.cast(t.ctypes.data, C.POINTER(_lib.CausalLogIdC)), len(t), vid, 0)
        if acc._bytes is not None:
            mb, ab = acc._bytes
        else:
            e = acc.entries()
            ln = e["len"]
            mb, ab = int(ln[e["id"]["is_main"] != 0].sum()), int(ln.sum())
        main_bytes += mb
        sub_bytes += ab - mb  # a bound: the table may name fewer
    sizes = np.empty(max(1, sub_bytes // 5), np.int32)
    sbase = np.zeros(n_sub + 1, np.uint64)
    cnt = np.zeros(max(1, n_sub), np.uint64)
    sst = np.zeros(max(1, n_sub), np.int32)
    soff = np.zeros(max(1, n_sub), np.int64)
    stag = np.zeros(max(1, n_sub), np.int32)
    if packed:  # the outputs sized and finished as the packed decodes' are
        fn = lib.clg_replay_prepare_columns_packed_device if device_input else lib.clg_replay_prepare_columns_packed

        def call(c, p, pk, wpk=None):
            out = _lib.ReplayPackedOut(C.pointer(c), C.pointer(p) if p is not None else None, C.pointer(pk),
                                       C.pointer(wpk) if wpk is not None else None, _np_ptr(sizes), sizes.size,
                                       _np_ptr(sbase), _np_ptr(cnt), _np_ptr(sst), _np_ptr(soff), _np_ptr(stag))
            return fn(engine.handle, vs, n, C.byref(out))

        main = engine._decode_packed(call, main_bytes, n, None, True, payloads, pack_wide=pack_wide)
        return ReplayColumns(main, sizes, sbase[:n_sub], cnt[:n_sub], sst[:n_sub], soff[:n_sub], stag[:n_sub],
                             [int(j[0]) for j in jobs], tables)
    fn = lib.clg_replay_prepare_columns_device if device_input else lib.clg_replay_prepare_columns
    arrs = engine._column_bounds(main_bytes, n)
    var, pos = engine._payload_bounds(main_bytes, n) if payloads else (None, None)
    for attempt in range(2):
        base = np.zeros((n + 1) * _lib.COL_CLASSES, np.uint64)
        c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
        p = _payloads_struct(var, pos) if payloads else None
        out = _lib.ReplayColumnsOut(C.pointer(c), C.pointer(p) if payloads else None, _np_ptr(sizes), sizes.size,
                                    _np_ptr(sbase), _np_ptr(cnt), _np_ptr(sst), _np_ptr(soff), _np_ptr(stag))
        st = fn(engine.handle, vs, n, C.byref(out))
        if st != _lib.CLG_E_CAPACITY or attempt or not int(c.n_rec):
            break
        # (the bounds hold for every decodable log, so this is not expected: the reported totals, once)
        nc = [int(x) for x in c.n_class]
        want = {"tag": int(c.n_rec), "order": nc[0], "timestamp": nc[1], "rng": nc[2], "buffer_built": nc[3]}
        arrs = {k: np.empty(want.get(k, nc[4]) + 1, a.dtype) for k, a in arrs.items()}
        if payloads:
            var, pos = np.empty(int(p.n_var) + 1, np.uint8), np.empty(int(p.n_rows) + 2, np.uint64)
    main = engine._columns_finish(st, c, arrs, base, None, True)
    if payloads:
        engine._payloads_attach(main, p, var, pos)
    return ReplayColumns(main, sizes, sbase[:n_sub], cnt[:n_sub], sst[:n_sub], soff[:n_sub], stag[:n_sub],
                         [int(j[0]) for j in jobs], tables)


# ---- replay verification -----------------------------------------------------------------
@dataclass
class Divergence:
    """Where a regenerated log leaves its recovered copy (locate_divergence).  Offsets are
    relative to the start of the compared range, getDeterminants(start_epoch) of the log."""
    offset: int                   # bytes the two have in common (clg_diff.lcp)
    kind: str                     # "differs" | "log_is_prefix" | "recovered_is_prefix"
    epoch: Optional[int]          # the last epoch of the log's range that starts at or before `offset`
    epoch_offset: Optional[int]   # ... and the offset inside it (None: the log has no epoch)
    record: Optional[int]         # index of the record that holds the byte (None: no record on either side)
    record_offset: Optional[int]  # ... and where it starts in the range
    regenerated: Optional[D.Determinant]  # that record as the log holds it; None: the log ended
    recovered: Optional[D.Determinant]    # before it, or its decode stopped at or before it


@dataclass
class ReplayCheck:
    """verify_replay's answer for one item: `matches` only when both fields of the two digests
    (hash, len) are equal."""
    matches: bool
    regenerated: Tuple[int, int]  # digest of getDeterminants(start_epoch) of the regenerated log
    recovered: Tuple[int, int]    # digest of the recovered copy
    divergence: Optional[Divergence] = None  # verify_replay(locate=True), when the two do not match


# the statuses with which a decode stops at a record (clg_decoded.err_off names it)
_DECODE_STOPS = (_lib.CLG_E_CORRUPT_TAG, _lib.CLG_E_TRUNCATED, _lib.CLG_E_BAD_ENUM, _lib.CLG_E_NEG_LEN,
                 _lib.CLG_E_BAD_SERIAL)


def range_epochs(log: ThreadCausalLog, start_epoch: int) -> Tuple[int, List[Tuple[int, int]]]:
    """The physical start of getDeterminants(start_epoch) of `log` and the epochs of that range
    as (epoch id, offset in the range), from the log's own epoch table (an absent epoch starts
    the range at the earliest one, as clg_get_determinants does)."""
    eps = log.state()["epochs"]
    if not eps:
        return 0, []
    at = [k for k, (e, _) in enumerate(eps) if e == start_epoch]
    k0 = at[0] if at else 0
    s = eps[k0][1]
    return s, [(int(e), int(o) - s) for e, o in eps[k0:]]


def _decode_clipped(decode, n: int):
    """decode(clip) with clip[i] = None (the whole of item i) or a length; an item at which the
    decode stops is clipped to the bytes before its failing record and the batch decoded again
    (one more call per such item, none for clean input).  Returns (batch, clip)."""
    clip: List[Optional[int]] = [None] * n
    while True:
        try:
            return decode(clip), clip
        except _lib.ClonosError as x:
            if x.status not in _DECODE_STOPS or not hasattr(x, "err_span"):
                raise
            clip[x.err_span] = int(x.err_off)


def locate_records(engine: Engine, handles, start_epochs, blobs: Sequence[bytes], offsets: Sequence[int]):
    """The record rule of locate_divergence for items that are known to diverge at range offset
    offsets[i]: per item (epoch, epoch_offset, record, record_offset, log's determinant, the
    bytes' determinant).  Both sides go through the batched decode, one call each for all items
    (decode_logs over the pool, decode_host over the given bytes).  k_side = that side's decoded
    records with off <= offset; record = max(k_log, k_bytes) - 1; a side's determinant is its
    record at that index when it has one.  The records before it are byte-identical on both
    sides, so both agree on its start."""
    n = len(handles)
    if not n:
        return []
    logs = [ThreadCausalLog(engine, int(h), None) for h in handles]
    epochs = [int(e) for e in start_epochs]
    ranges = [range_epochs(l, e) for l, e in zip(logs, epochs)]
    blobs = [bytes(b) for b in blobs]

    # a log whose decode stops is decoded from the host, from its bytes before the failing record
    moved: Dict[int, bytes] = {}

    keep, dec_l = list(range(n)), None
    while keep:
        try:
            dec_l = engine.decode_logs([logs[i] for i in keep], [epochs[i] for i in keep])
            break
        except _lib.ClonosError as x:
            if x.status not in _DECODE_STOPS or not hasattr(x, "err_span"):
                raise
            i = keep.pop(x.err_span)  # (one more call per such log, none for clean input)
            moved[i] = logs[i].read_phys(ranges[i][0], int(x.err_off)) if x.err_off else b""
    span_l = {i: k for k, i in enumerate(keep)}
    extra = sorted(moved)
    host = blobs + [moved[i] for i in extra]
    lens = [len(b) for b in host]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if host else []
    joined = b"".join(host)

    def decode_h(clip):
        return engine.decode_host(joined, [(int(o), ln if c is None else c) for o, ln, c in zip(starts, lens, clip)])

    dec_h, _ = _decode_clipped(decode_h, len(host))
    span_m = {i: n + k for k, i in enumerate(extra)}

    out = []
    for i in range(n):
        off = int(offsets[i])
        s_phys, eps = ranges[i]
        # the log's side: its own span of the pool decode, or of the host decode when it was moved
        if i in span_l:
            bl, sl = dec_l, span_l[i]
            var_l = (lambda vo, vl, i=i, s=s_phys: logs[i].read_phys(s + vo, vl))
        else:
            bl, sl = dec_h, span_m[i]
            var_l = (lambda vo, vl, b=moved[i]: b[vo:vo + vl])
        off_l = np.asarray(bl.off[bl.span_slice(sl)])
        off_r = np.asarray(dec_h.off[dec_h.span_slice(i)])
        k_l = int(np.searchsorted(off_l, off, side="right"))
        k_r = int(np.searchsorted(off_r, off, side="right"))
        rec = max(k_l, k_r) - 1
        ep = [(e, o) for e, o in eps if o <= off]
        epoch, epoch_off = (ep[-1][0], off - ep[-1][1]) if ep else (None, None)
        if rec < 0:
            out.append((epoch, epoch_off, None, None, None, None))
            continue
        d_l = bl.determinant_at(sl, rec, var_l) if rec < len(off_l) else None
        d_r = dec_h.determinant_at(i, rec, lambda vo, vl, b=blobs[i]: b[vo:vo + vl]) if rec < len(off_r) else None
        rec_off = int(off_l[rec]) if rec < len(off_l) else int(off_r[rec])
        out.append((epoch, epoch_off, rec, rec_off, d_l, d_r))
    return out


def locate_divergence(engine: Engine, items: Sequence[Tuple[int, int, bytes]]) -> List[Optional[Divergence]]:
    """Where does each regenerated log leave its recovered copy?  Items as verify_replay's:
    (log handle, start_epoch, recovered bytes).  None for an item whose two sides are equal,
    else a Divergence: the first differing byte (clg_diff_logs compares the log where it lies
    with the recovered bytes, 24 bytes per item come back), whether one side is a prefix of the
    other, the epoch (from the log's own epoch table: the recovered bytes carry none), and the
    record that holds the byte, decoded on each side.  Only divergent items are decoded: the
    logs with one decode_logs and the recovered bytes with one decode_host for all of them.  A
    replay that diverged logged some nondeterminism differently: the two determinants say which."""
    n = len(items)
    if not n:
        return []
    handles = np.array([it[0] for it in items], np.uint32)
    epochs = np.array([it[1] for it in items], np.int64)
    blobs = [bytes(it[2]) for it in items]
    lens = np.array([len(b) for b in blobs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rows = engine.diff_logs(handles, epochs, b"".join(blobs), offs, lens)
    out: List[Optional[Divergence]] = [None] * n
    bad = [i for i in range(n) if not int(rows[i]["lcp"]) == int(rows[i]["len_log"]) == int(rows[i]["len_ref"])]
    recs = locate_records(engine, handles[bad], epochs[bad], [blobs[i] for i in bad], [int(rows[i]["lcp"]) for i in bad])
    for i, r in zip(bad, recs):
        lcp, ll, lr = (int(rows[i][f]) for f in ("lcp", "len_log", "len_ref"))
        kind = "differs" if lcp < min(ll, lr) else ("log_is_prefix" if ll < lr else "recovered_is_prefix")
        out[i] = Divergence(lcp, kind, *r)
    return out


def verify_replay(engine: Engine, items: Sequence[Tuple[int, int, bytes]], locate: bool = False) -> List[ReplayCheck]:
    """Does each regenerated log equal its recovered copy?  An item is (log handle,
    start_epoch, recovered bytes): the log as the replay re-appended it, and the response bytes
    the replay was fed from.  LogReplayerImpl.checkFinished (LogReplayerImpl.java:126-128)
    asserts only that the two have the same length, and only under -ea: a replay that diverged
    but logged as many bytes passes it.  Here both sides are digested on the device
    (clg_digest_logs over the segment pool, clg_digest_spans over the recovered bytes) and
    compared by content.

    locate=True: each item that does not match also carries where the two part
    (ReplayCheck.divergence, from locate_divergence over those items alone).

    To find the first divergent epoch without it, digest the suffixes from each epoch in one batch:
    items [(h, e, recovered[start_of(e):]) for e in epochs] -- the suffixes from the epochs
    after the divergence match, so the last epoch whose suffix does not is where it diverged."""
    n = len(items)
    if not n:
        return []
    handles = np.array([it[0] for it in items], np.uint32)
    epochs = np.array([it[1] for it in items], np.int64)
    blobs = [bytes(it[2]) for it in items]
    lens = np.array([len(b) for b in blobs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    regen = engine.digest_logs(handles, epochs)
    recov = engine.digest_spans(b"".join(blobs), offs, lens)
    out = []
    for a, b in zip(regen, recov):
        ra, rb = (int(a["hash"]), int(a["len"])), (int(b["hash"]), int(b["len"]))
        out.append(ReplayCheck(ra == rb, ra, rb))
    if locate:
        bad = [i for i, c in enumerate(out) if not c.matches]
        for i, d in zip(bad, locate_divergence(engine, [items[i] for i in bad])):
            out[i].divergence = d
    return out


# ---- LogReplayerImpl over typed columns ---------------------------------------------------------
class ReplayOrderError(AssertionError):
    """A replay call whose type is not the next determinant's (the reference's `assert
    nextDeterminant instanceof ...`, LogReplayerImpl.java:62, :72, :82, :92, :103)."""

    def __init__(self, position: int, asked: str, found: str):
        super().__init__(f"record {position} of the span: asked for {asked}, the next determinant is {found}")
        self.position, self.asked, self.found = position, asked, found


_ASYNC_TAGS = (D.TIMER_TRIGGER, D.SOURCE_CHECKPOINT, D.IGNORE_CHECKPOINT)  # AsyncDeterminant's subclasses


class ColumnReplayer:
    """LogReplayerImpl's cursor (LogReplayerImpl.java:51-158) over one span of DecodedColumns:
    the next determinant is the next tag; every method reads that tag and bumps one index into
    one column.  var(off, len): the span's bytes for names, references and java streams (None:
    from the columns' payload column when they carry one -- the offsets are then var_pos, not
    w_var_off -- else from their spans_bytes when they kept them)."""

    def __init__(self, columns, s: int, var=None):
        sp = columns.span(s)
        self._c = columns
        self._tag = sp.tag
        self._order, self._ts, self._rng, self._bb = sp.order, sp.timestamp, sp.rng, sp.buffer_built
        self._pos = 0                      # records consumed
        self._at = [0, 0, 0, 0, sp.w0]     # the next index into each class's column
        self._packed = var is None and getattr(columns, "var", None) is not None
        if var is None and not self._packed and columns.spans_bytes is not None:
            raw = columns.spans_bytes[s]
            var = lambda vo, vl: bytes(raw[vo:vo + vl])
        self._var = var

    def _next(self, asked: str, *tags) -> int:
        """The next tag, which must be one of `tags`; the record is consumed."""
        t = int(self._tag[self._pos]) if self._pos < len(self._tag) else None
        if t not in tags:
            raise ReplayOrderError(self._pos, asked, "nothing (the log is finished)" if t is None else D.TAG_NAMES[t])
        self._pos += 1
        return t

    def _bump(self, cls: int) -> int:
        k = self._at[cls]
        self._at[cls] = k + 1
        return k

    def _wide(self, t: int) -> D.Determinant:
        c, k = self._c, self._bump(4)
        if self._packed:  # (w_var_off still says whether the row has a payload: nonzero)
            return _wide_determinant(t, int(c.w_v0[k]), int(c.w_rc[k]), int(c.w_v1[k]), int(c.w_var_off[k]),
                                     int(c.w_var_len[k]), int(c.w_sub[k]), lambda vo, vl: c.payload(k))
        return _wide_determinant(t, int(c.w_v0[k]), int(c.w_rc[k]), int(c.w_v1[k]), int(c.w_var_off[k]),
                                 int(c.w_var_len[k]), int(c.w_sub[k]), self._var)

    def replayNextChannel(self) -> int:  # :71-78, a Java byte
        self._next("ORDER", D.ORDER)
        return int(self._order[self._bump(0)])

    def replayNextTimestamp(self) -> int:  # :81-88
        self._next("TIMESTAMP", D.TIMESTAMP)
        return int(self._ts[self._bump(1)])

    def replayRandomInt(self) -> int:  # :61-68
        self._next("RNG", D.RNG)
        return int(self._rng[self._bump(2)])

    def replayNextBufferSize(self) -> int:
        """The next BufferBuilt size (SubpartitionRecoveryThread.run, ReplayingState.java:161-188)."""
        self._next("BUFFER_BUILT", D.BUFFER_BUILT)
        return int(self._bb[self._bump(3)])

    def replaySerializableDeterminant(self) -> bytes:  # :91-98; the java stream (Python does not deserialize it)
        return self._wide(self._next("SERIALIZABLE", D.SERIALIZABLE)).stream

    def triggerAsyncEvent(self, current_record_count: int) -> D.Determinant:
        """:102-119: the async determinant, consumed; raises when the epoch tracker's record
        count is not the determinant's (:110-111), with the determinant left in place."""
        t = int(self._tag[self._pos]) if self._pos < len(self._tag) else None
        if t not in _ASYNC_TAGS:
            raise ReplayOrderError(self._pos, "an async determinant",
                                   "nothing (the log is finished)" if t is None else D.TAG_NAMES[t])
        rc = int(self._c.w_rc[self._at[4]])
        if current_record_count != rc:
            raise RuntimeError("Current record count is not the determinants record count. "
                               f"Current: {current_record_count}, determinant: {rc}")
        self._pos += 1
        return self._wide(t)

    def record_count_target(self) -> Optional[int]:
        """What postHook hands the epoch tracker (:147-152): the next determinant's record count
        when that determinant is async, else None."""
        if self._pos < len(self._tag) and int(self._tag[self._pos]) in _ASYNC_TAGS:
            return int(self._c.w_rc[self._at[4]])
        return None

    def next_tag(self) -> Optional[int]:
        return int(self._tag[self._pos]) if self._pos < len(self._tag) else None

    def isFinished(self) -> bool:  # :154-156
        return self._pos >= len(self._tag)
