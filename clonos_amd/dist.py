"""Multi-GPU sharding, sharing-depth replication and the cross-GPU replay-prep merge
(SURVEY.md 8e).

One process per GPU, one Engine per process.  Logs shard by VertexID (job.owner_rank):
rank g owns the vertices v with v mod G == g and is the only writer of their logs.

Replication.  Consumers on other GPUs need replicas of upstream logs within the sharing
depth (job.replication_masks).  Every rank builds the same canonical log table
(job.LogTable: a global index `gid` per CausalLogID), so the wire carries gids and every
per-log step is a numpy gather over dense tables -- no per-log Python.  One exchange (per
epoch, or per batch of buffers):

  1. the owner slices the new bytes of every owned log for every other rank that wants it
     (each receiving rank is one consumer of the log, with its own offset): the engine's
     batched hasDelta/getOffset/getDelta (clg_slice_batch), ONE device gather into a
     payload buffer grouped by destination;
  2. two all-to-alls (RCCL over xGMI with the "nccl" backend; gloo on CPU): the header
     rows, one per planned (log, destination) request, with static split sizes every rank
     knows from the plan; then, after one read-back of the headers, the payload with the
     split sizes they carry.  A rank receives only the logs within its sharing depth (at
     depth 1 only its direct producers'), and with one rank no collective runs;
  3. every rank applies the received rows with the batched processUpstreamDelta
     (clg_upstream_delta_batch) reading straight from the receive buffer in HBM.  The dedup
     rule of ThreadCausalLogImpl.java:117-154 makes re-delivery harmless.

This replaces the reference's piggybacking of CausalLogDelta on network buffers for
GPU-to-GPU traffic (AbstractDeltaSerializerDeserializer.java:89-163,
FlatDeltaSerializerDeserializer.java:57-90): the bytes and the (offsetFromEpoch, epoch)
pairs are the same, the transport is a collective.

Replay-prep merge (concurrent / connected failures).  DeterminantResponseEvent.merge
(DeterminantResponseEvent.java:128-148) keeps, per CausalLogID, the longest copy among
the responses (WaitingDeterminantsState.java:97-109).  Across GPUs: every rank measures its
copy of each log of the failed vertices, one all-reduce(MAX) over packed
(len << 8 | rank) picks the winner per log, and one all-to-all moves each winner's bytes to
the rank hosting the failed vertex's replacement (merge_responses).

Verification.  A replica is trusted to equal its owner's log, and a merged winner the log its
rank measured; the log digest (clg_digest_logs / clg_digest_spans: 16 bytes per log, computed
where the bytes live) lets the product check both without moving the bytes: Replicator.verify
compares every replica with its owner at a quiescent point, merge_responses(verify=True) the
received winners with what their ranks hold.  Replicator.locate then says where a flagged
replica leaves its owner's log (clg_diff_logs on the fetched copy): only the flagged logs move.

Prefixes.  The merge by length and the offset dedup both take the shorter copy of a log for a
prefix of the longer one.  Prefix digests (clg_digest_prefixes: a log's digest at many cut
lengths in one read) let the holder of the longer copy check that with the other side's 16
bytes: Replicator.verify(prefixes=True) tells a lagging replica from a diverged one,
Replicator.first_bad_epoch names the epoch in which two copies part from per-epoch rows
(clg_digest_epochs), and merge_responses(verify="prefixes") checks every losing copy against
the winner.  No log bytes move in any of them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import itertools

import numpy as np

from . import _lib
from ._lib import check, lib
from .engine import CausalLogID, Engine, ThreadCausalLog
from .job import JobGraph, LogTable, owner_rank, replication_masks

# One header row per delta (little-endian, 32 bytes): global log index, epoch,
# offsetFromEpoch, length, payload offset inside the sender's payload for this receiver.
HEADER = np.dtype([("gid", "<i4"), ("offset_from_epoch", "<i4"), ("epoch", "<i8"), ("len", "<u4"),
                   ("pad", "<u4"), ("payload_off", "<u8")])
assert HEADER.itemsize == 32
BLOB_ALIGN = 64
REPLICATION_CHANNEL = (0xC1055EED00000000, 0x5EED)  # replication consumer; destination rank in ch_hi bits 16+

# numpy views of the C request / result structs (include/clonos_engine.h)
SLICE_REQ = np.dtype([("log", "<u4"), ("reserved", "<u4"), ("ch_lo", "<u8"), ("ch_hi", "<u8"), ("epoch", "<i8")])
SLICE_RES = np.dtype([("status", "<i4"), ("has_delta", "<i4"), ("offset_from_epoch", "<i4"), ("len", "<i4"),
                      ("out_off", "<u8")])
DELTA_REQ = np.dtype([("log", "<u4"), ("offset_from_epoch", "<i4"), ("epoch", "<i8"), ("src_off", "<u8"),
                      ("len", "<u4"), ("status", "<i4")])
assert SLICE_REQ.itemsize == C.sizeof(_lib.SliceReq) and SLICE_RES.itemsize == C.sizeof(_lib.SliceRes)
assert DELTA_REQ.itemsize == C.sizeof(_lib.DeltaReq)
# Replicator.verify's wire row, one per planned request: the owner's digest of the log
VERIFY_ROW = np.dtype([("gid", "<i8"), ("len", "<u8"), ("hash", "<u8")])
# Replicator.first_bad_epoch's wire row, one per epoch of an asked log: the digest up to its end
EPOCH_ROW = np.dtype([("epoch", "<i8"), ("len", "<u8"), ("hash", "<u8")])


def _align(n: int) -> int:
    return (n + BLOB_ALIGN - 1) // BLOB_ALIGN * BLOB_ALIGN


# ---- collectives ------------------------------------------------------------------------
def _to_comm(t, backend: str):
    """gloo moves host tensors; RCCL ("nccl") moves device tensors in place."""
    return t if (backend == "nccl" or not t.is_cuda) else t.cpu()


# ---- replication ------------------------------------------------------------------------
@dataclass
class ExchangeStats:
    sent_bytes: int = 0     # header rows + payload this rank sent
    recv_bytes: int = 0     # header rows + payload this rank received
    applied: int = 0        # deltas applied to replicas
    applied_bytes: int = 0  # delta bytes those deltas carried
    skipped: int = 0        # rows for logs this rank does not want


@dataclass
class VerifyReport:
    """Replicator.verify on one rank: the gids whose replica here is shorter / longer than the
    owner's log, or of its length with another hash; `checked` replicas were compared.
    verify(prefixes=True) also fills short_diverged / long_diverged: the subsets of short / long
    whose shorter copy is NOT a prefix of the longer one (the rest of `short` merely lag)."""
    short: List[int]
    long: List[int]
    differs: List[int]
    checked: int = 0
    short_diverged: List[int] = field(default_factory=list)
    long_diverged: List[int] = field(default_factory=list)

    @property
    def clean(self) -> bool:
        return not (self.short or self.long or self.differs)

    @property
    def diverged(self) -> List[int]:
        """The gids whose copies hold different bytes somewhere in their common part."""
        return sorted(set(self.differs) | set(self.short_diverged) | set(self.long_diverged))

    def only_diverged(self) -> "VerifyReport":
        """A report of the diverged gids alone, for Replicator.locate: lagging true prefixes
        move no bytes."""
        return VerifyReport(list(self.short_diverged), list(self.long_diverged), list(self.differs), self.checked,
                            list(self.short_diverged), list(self.long_diverged))


class EpochResult(dict):
    """Replicator.first_bad_epoch's answer: gid -> the first epoch id in which the replica here
    and the owner's log differ (None: every epoch row is equal); `unlocated`: the gids beyond
    `limit` per owner rank, which were not compared."""

    def __init__(self, items=(), unlocated=()):
        super().__init__(items)
        self.unlocated: List[int] = list(unlocated)


@dataclass
class ReplicaDivergence:
    """Replicator.locate's answer for one flagged log: where this rank's replica leaves the
    owner's copy.  Offsets are relative to getDeterminants(start_epoch).  The epoch and record
    fields are filled where the io offers them (EngineIO does), following
    replay.locate_divergence's record rule, from the replica's own epoch table."""
    gid: int
    offset: int        # bytes the two have in common
    len_replica: int
    len_owner: int
    kind: str          # "differs" | "replica_is_prefix" | "owner_is_prefix" ("equal": flagged, yet no difference)
    epoch: Optional[int] = None
    epoch_offset: Optional[int] = None
    record: Optional[int] = None
    record_offset: Optional[int] = None
    replica: object = None  # that record as the replica holds it (determinants.Determinant or None)
    owner: object = None    # ... and as the owner does


class LocateResult(list):
    """Replicator.locate's list of ReplicaDivergence; `unlocated`: the flagged gids beyond
    `limit` per owner rank, which were not fetched."""

    def __init__(self, items=(), unlocated=()):
        super().__init__(items)
        self.unlocated: List[int] = list(unlocated)


class ReplicationPlan:
    """The static part of sharing-depth replication for one rank: which owned logs it
    sends to which rank, which logs it keeps replicas of, and the dense handle tables.
    Built once per job and rank (registerTask time), identically on every rank.

    Each receiving rank is one downstream consumer of every log it wants (its own consumer
    offset per log, as each output channel is in FlatDeltaSerializerDeserializer.java:57-90),
    so a rank receives exactly the logs within its sharing depth and nothing else: the
    requests (req_gid, req_dest) are grouped by destination rank."""

    def __init__(self, table: LogTable, depth: int, rank: int, world: int,
                 need: Optional[np.ndarray] = None):
        self.table, self.rank, self.world = table, rank, world
        g = table.graph
        need = replication_masks(g, depth, world) if need is None else need  # [rank, vertex]
        owner = np.array([owner_rank(int(v), world) for v in range(need.shape[1])], np.int64)
        lv = table.vertex
        self.owned = np.nonzero(owner[lv] == rank)[0]            # gids this rank writes
        wanted_anywhere = need.any(axis=0)
        self.send = self.owned[wanted_anywhere[lv[self.owned]]]  # owned gids some rank wants
        self.wanted = np.nonzero(need[rank][lv])[0]               # gids this rank keeps replicas of
        # one slice request per (sent log, destination rank that wants it), by destination
        per_dest = [self.owned[need[r][lv[self.owned]]] if r != rank else self.owned[:0] for r in range(world)]
        self.req_gid = np.concatenate(per_dest).astype(np.int64) if world else np.zeros(0, np.int64)
        self.req_dest = np.repeat(np.arange(world, dtype=np.int64), [len(p) for p in per_dest])
        self.n_to = np.array([len(p) for p in per_dest], np.int64)  # requests per destination
        # header rows every other rank sends here (one per its planned request for this rank):
        # static, so the header all-to-all needs no count exchange first
        mine_needed = need[rank][lv]
        src_of = owner[lv]
        self.n_from = np.array([int(((src_of == r) & mine_needed).sum()) if r != rank else 0 for r in range(world)],
                               np.int64)


class EngineIO:
    """The byte work of replication on the engine (HBM): batched slices into a device
    blob, batched device-input processUpstreamDelta into replicas."""

    def __init__(self, engine: Engine, job: int = 0):
        self.engine, self.job = engine, job

    def open_replica(self, cid: CausalLogID) -> int:
        return self.engine.open_log(cid, self.job).handle

    def payload_bound(self, handles: np.ndarray) -> int:
        return self.engine.log_lengths(handles)[1]

    def slice(self, sreq: np.ndarray, sres: np.ndarray, n: int, out_ptr: int, cap: int) -> int:
        total = C.c_uint64()
        check(lib.clg_slice_batch(self.engine.handle, sreq.ctypes.data, n, sres.ctypes.data, out_ptr, cap,
                                  _lib.CLG_MEM_DEVICE, C.byref(total)))
        if self.engine.async_slice:  # the collective reads the payload: order it after the gather
            import torch
            gs = lib.clg_gather_stream(self.engine.handle)
            torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(gs))
        return total.value

    def apply(self, req: np.ndarray, recv) -> None:
        kind = _lib.CLG_MEM_DEVICE if recv.is_cuda else _lib.CLG_MEM_HOST
        check(lib.clg_upstream_delta_batch(self.engine.handle, req.ctypes.data, len(req), recv.data_ptr(), kind))

    def digest(self, handles: np.ndarray, start_epochs: np.ndarray) -> np.ndarray:
        """DIGEST rows of getDeterminants(start_epochs[i]) of handles[i] (clg_digest_logs)."""
        return self.engine.digest_logs(handles, start_epochs)

    def digest_spans(self, tensor, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
        """DIGEST rows of tensor[offs[i] : offs[i] + lens[i]] (clg_digest_spans; device input
        for a tensor in HBM)."""
        if tensor.is_cuda:
            return self.engine.digest_spans(tensor.data_ptr(), offs, lens, device=True)
        return self.engine.digest_spans(tensor.numpy(), offs, lens)

    def digest_prefixes(self, handles: np.ndarray, start_epochs: np.ndarray, first: np.ndarray, cuts: np.ndarray
                        ) -> np.ndarray:
        """DIGEST rows of getDeterminants(start_epochs[i]) of handles[i] at its cut lengths
        cuts[first[i] : first[i + 1]], not decreasing (clg_digest_prefixes)."""
        return self.engine.digest_prefixes(handles, start_epochs, (first, cuts))[0]

    def digest_epochs(self, handles: np.ndarray, start_epochs: np.ndarray):
        """(first, epoch ids, DIGEST rows): a row per epoch of each range (clg_digest_epochs)."""
        return self.engine.digest_epochs(handles, start_epochs)

    def diff(self, handles: np.ndarray, start_epochs: np.ndarray, tensor, offs: np.ndarray, lens: np.ndarray
             ) -> np.ndarray:
        """DIFF rows of getDeterminants(start_epochs[i]) of handles[i] against
        tensor[offs[i] : offs[i] + lens[i]] (clg_diff_logs; device input for a tensor in HBM)."""
        if tensor.is_cuda:
            return self.engine.diff_logs(handles, start_epochs, tensor.data_ptr(), offs, lens, device=True)
        return self.engine.diff_logs(handles, start_epochs, tensor.numpy(), offs, lens)

    def locate_records(self, handles, start_epochs, tensor, offs, lens, offsets):
        """replay.locate_records for logs that part from tensor[offs[i] : offs[i] + lens[i]] at
        offsets[i]: (epoch, epoch_offset, record, record_offset, the log's determinant, the
        tensor's) per item.  Only these spans are read back for the decode."""
        from .replay import locate_records
        blobs = [tensor[int(o):int(o) + int(n)].cpu().numpy().tobytes() for o, n in zip(offs, lens)]
        return locate_records(self.engine, handles, start_epochs, blobs, offsets)

    # replay-prep merge: a copy is getDeterminants(startEpoch) of a log (owned or replica);
    # both calls are one native call for all the copies (clg_get_determinants_batch)
    def copy_lengths(self, handles: np.ndarray, start_epochs: np.ndarray) -> np.ndarray:
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        ln = np.zeros(max(1, len(h)), np.uint32)
        total = C.c_uint64()
        check(lib.clg_get_determinants_batch(self.engine.handle, h.ctypes.data, ep.ctypes.data, len(h), None, 0,
                                             _lib.CLG_MEM_DEVICE, None, ln.ctypes.data, C.byref(total)))
        return ln[:len(h)].astype(np.int64)

    def copy_batch(self, handles: np.ndarray, start_epochs: np.ndarray, tensor, off: int) -> int:
        """The copies back to back in the given order into tensor[off:] (one gather)."""
        h = np.ascontiguousarray(handles, np.uint32)
        ep = np.ascontiguousarray(start_epochs, np.int64)
        ln = np.zeros(max(1, len(h)), np.uint32)
        total = C.c_uint64()
        kind = _lib.CLG_MEM_DEVICE if tensor.is_cuda else _lib.CLG_MEM_HOST
        check(lib.clg_get_determinants_batch(self.engine.handle, h.ctypes.data, ep.ctypes.data, len(h),
                                             tensor.data_ptr() + off, tensor.numel() - off, kind, None,
                                             ln.ctypes.data, C.byref(total)))
        return int(total.value)


class Replicator:
    """Sharing-depth replication for one rank.  `io` does the byte work (EngineIO; the CPU
    tests pass a stand-in over the oracle).  owned_handles: gid -> handle of each owned log
    that is sent; replicas of the wanted logs are opened here.

    One exchange moves each destination only the logs it wants: the slices of all requests
    land in one payload buffer grouped by destination (one batched slice), and two
    collectives carry them -- an all-to-all of the header rows (static split sizes: one row
    per planned request) and an all-to-all of the payload (split sizes from the headers).
    With one rank there is nothing to move and no collective runs."""

    def __init__(self, io, plan: ReplicationPlan, device, owned_handles: Dict[int, int], group=None):
        self.io, self.plan, self.device, self.group = io, plan, device, group
        n = len(plan.table)
        self.handle = np.full(n, -1, np.int64)
        for gid, h in owned_handles.items():
            self.handle[gid] = h
        self.replica_handle = np.full(n, -1, np.int64)
        for gid in plan.wanted:
            self.replica_handle[gid] = io.open_replica(plan.table.ids[gid])
        missing = sorted({int(g) for g in plan.req_gid if self.handle[g] < 0})
        if missing:
            raise ValueError(f"no log handle for owned gids {missing[:8]}")
        # prebuilt slice requests: one per (sent log, destination), the destination's consumer
        nq = len(plan.req_gid)
        self._sreq = np.zeros(max(nq, 1), SLICE_REQ)
        self._sreq["log"][:nq] = self.handle[plan.req_gid]
        self._sreq["ch_lo"][:nq] = REPLICATION_CHANNEL[0]
        self._sreq["ch_hi"][:nq] = REPLICATION_CHANNEL[1] | (plan.req_dest.astype(np.uint64) << np.uint64(16))
        self._sres = np.zeros(max(nq, 1), SLICE_RES)
        self._payload = None

    def payload_bound(self) -> int:
        """Bytes the requests' slices can need at most (their logs' lengths)."""
        nq = len(self.plan.req_gid)
        return self.io.payload_bound(self._sreq["log"][:nq]) if nq else 0

    def build_payload(self, epoch: int, payload_cap: Optional[int] = None):
        """Slice every request into the payload buffer (grouped by destination).  Returns
        (payload, one header row per planned request -- len 0 where there is no delta --,
        bytes per destination)."""
        import torch
        plan = self.plan
        nq = len(plan.req_gid)
        cap = payload_cap if payload_cap is not None else self.payload_bound()
        if self._payload is None or self._payload.numel() < cap + BLOB_ALIGN:
            self._payload = torch.empty(_align(cap) + BLOB_ALIGN, dtype=torch.uint8, device=self.device)
        self._sreq["epoch"][:nq] = epoch
        if nq:
            self.io.slice(self._sreq, self._sres, nq, self._payload.data_ptr(), cap)
        res = self._sres[:nq]
        bad = np.nonzero(res["status"])[0]
        if bad.size:
            check(int(res["status"][bad[0]]))
        ln = np.where(res["has_delta"] != 0, res["len"], 0).astype(np.int64)
        # clg_slice_batch packs the slices back to back in request order (requests are grouped
        # by destination), so each destination's part is contiguous; checked, not assumed
        out_off = res["out_off"].astype(np.int64)
        packed = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64) if nq else out_off
        keep = ln > 0
        if not np.array_equal(out_off[keep], packed[keep]):
            raise RuntimeError("slice outputs are not packed in request order")
        bytes_to = np.bincount(plan.req_dest, weights=ln, minlength=plan.world).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(bytes_to)[:-1]]).astype(np.int64)
        rows = np.zeros(nq, HEADER)
        rows["gid"] = plan.req_gid
        rows["offset_from_epoch"] = np.where(keep, res["offset_from_epoch"], 0)
        rows["epoch"] = epoch
        rows["len"] = ln
        rows["payload_off"] = np.where(keep, packed - start[plan.req_dest], 0)  # within its destination's part
        return self._payload, rows, bytes_to

    def exchange(self, epoch: int, payload_cap: Optional[int] = None) -> ExchangeStats:
        """One replication round for `epoch` (all ranks call it together): two all-to-alls
        and one read-back.  The header rows go first with STATIC split sizes (one row per
        planned request, ReplicationPlan.n_to / n_from, so no count exchange precedes them);
        their read-back gives the payload's split sizes and the apply requests; then the
        payload."""
        import torch
        import torch.distributed as dist
        st = ExchangeStats()
        plan = self.plan
        if plan.world == 1:
            return st
        payload, rows, bytes_to = self.build_payload(epoch, payload_cap)
        backend = dist.get_backend(self.group)
        dev = self.device if backend == "nccl" else "cpu"
        # 1. header rows, static splits
        hsend = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        hrecv = torch.empty(int(plan.n_from.sum()) * HEADER.itemsize, dtype=torch.uint8, device=dev)
        dist.all_to_all_single(hrecv, hsend, output_split_sizes=(plan.n_from * HEADER.itemsize).tolist(),
                               input_split_sizes=(plan.n_to * HEADER.itemsize).tolist(), group=self.group)
        rr = hrecv.cpu().numpy().view(HEADER)  # the one read-back (it also orders the host after the collective)
        src_rank = np.repeat(np.arange(plan.world), plan.n_from)
        bytes_from = np.bincount(src_rank, weights=rr["len"].astype(np.int64), minlength=plan.world).astype(np.int64)
        st.sent_bytes = int(rows_sent(rows)) * HEADER.itemsize + int(bytes_to.sum())
        st.recv_bytes = int(rows_sent(rr)) * HEADER.itemsize + int(bytes_from.sum())
        # 2. payload
        nrecv = int(bytes_from.sum())
        recv = torch.empty(max(nrecv, 1) + BLOB_ALIGN, dtype=torch.uint8, device=dev)
        psend = _to_comm(payload[:int(bytes_to.sum())], backend)
        dist.all_to_all_single(recv[:nrecv], psend, output_split_sizes=bytes_from.tolist(),
                               input_split_sizes=bytes_to.tolist(), group=self.group)
        live = rr["len"] > 0
        if not live.any():
            return st
        src_start = np.concatenate([[0], np.cumsum(bytes_from)[:-1]]).astype(np.uint64)
        src = src_start[src_rank] + rr["payload_off"].astype(np.uint64)
        h = self.replica_handle[rr["gid"]]
        want = live & (h >= 0)
        st.skipped = int((live & (h < 0)).sum())
        n = int(want.sum())
        if n:
            req = np.zeros(n, DELTA_REQ)
            req["log"] = h[want]
            req["offset_from_epoch"] = rr["offset_from_epoch"][want]
            req["epoch"] = rr["epoch"][want]
            req["src_off"] = src[want]
            req["len"] = rr["len"][want]
            if str(self.device).startswith("cuda") and not recv.is_cuda:  # gloo: into HBM once
                recv = recv.to(self.device)
            self.io.apply(req, recv)
            bad = np.nonzero(req["status"])[0]
            if bad.size:
                check(int(req["status"][bad[0]]))
            st.applied = n
            st.applied_bytes = int(req["len"].sum())
        return st


    def verify(self, start_epoch: int, prefixes: bool = False) -> VerifyReport:
        """Compare every replica with its owner's log from `start_epoch` by digest.  All ranks
        call it together at a quiescent point (after exchange, before new appends).  Each
        owner digests every log it sends, once; one all-to-all carries one row per planned
        request (gid, len, hash) with the header rows' static splits (ReplicationPlan.n_to /
        n_from); each receiver digests its replicas from the same epoch.  With one rank no
        collective runs and the report is empty.

        prefixes=True (every rank passes the same value) also says whether the shorter copy
        of a short / long pair is a prefix of the longer one -- a lagging replica, the benign
        case, or a diverged one.  Whichever side holds the longer copy digests it at the other
        side's length (io.digest_prefixes) and compares: the replica does so for `long` with
        the row it already has; for `short` a second all-to-all carries the replicas'
        (gid, len, hash) back to the owners (the same static splits, swapped), each owner
        digests every sent log once at the distinct lengths its replicas reported, and a
        third all-to-all returns one verdict byte per planned request.  short, long and
        differs are what verify(start_epoch) gives."""
        import torch
        import torch.distributed as dist
        plan = self.plan
        rep = VerifyReport([], [], [])
        if plan.world == 1:
            return rep
        nq = len(plan.req_gid)
        rows = np.zeros(nq, VERIFY_ROW)
        if nq:
            sent, inv = np.unique(plan.req_gid, return_inverse=True)  # each sent log digested once
            dg = self.io.digest(self.handle[sent].astype(np.uint32), np.full(len(sent), start_epoch, np.int64))
            rows["gid"] = plan.req_gid
            rows["len"] = dg["len"][inv]
            rows["hash"] = dg["hash"][inv]
        backend = dist.get_backend(self.group)
        dev = self.device if backend == "nccl" else "cpu"
        vsend = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        vrecv = torch.empty(int(plan.n_from.sum()) * VERIFY_ROW.itemsize, dtype=torch.uint8, device=dev)
        dist.all_to_all_single(vrecv, vsend, output_split_sizes=(plan.n_from * VERIFY_ROW.itemsize).tolist(),
                               input_split_sizes=(plan.n_to * VERIFY_ROW.itemsize).tolist(), group=self.group)
        rr = vrecv.cpu().numpy().view(VERIFY_ROW)
        h = self.replica_handle[rr["gid"]]
        have = np.nonzero(h >= 0)[0]
        if not len(have) and not prefixes:
            return rep
        mine = self.io.digest(h[have].astype(np.uint32), np.full(len(have), start_epoch, np.int64))
        theirs = rr[have]
        gid = theirs["gid"]
        rep.short = gid[mine["len"] < theirs["len"]].tolist()
        rep.long = gid[mine["len"] > theirs["len"]].tolist()
        rep.differs = gid[(mine["len"] == theirs["len"]) & (mine["hash"] != theirs["hash"])].tolist()
        rep.checked = len(have)
        if not prefixes:
            return rep
        # long: this rank holds the longer copy -- its digest at the owner's length
        lg = np.nonzero(mine["len"] > theirs["len"])[0]
        if len(lg):
            at = self.io.digest_prefixes(h[have][lg].astype(np.uint32), np.full(len(lg), start_epoch, np.int64),
                                         np.arange(len(lg) + 1, dtype=np.uint64), theirs["len"][lg].astype(np.uint32))
            rep.long_diverged = gid[lg[(at["hash"] != theirs["hash"][lg]) | (at["len"] != theirs["len"][lg])]].tolist()
        # short: the owner holds the longer copy -- the replicas' rows go back, splits swapped
        back = np.zeros(len(rr), VERIFY_ROW)
        back["gid"] = -1  # (a log this rank keeps no replica of)
        back["gid"][have] = gid
        back["len"][have] = mine["len"]
        back["hash"][have] = mine["hash"]
        bsend = torch.from_numpy(back.view(np.uint8).copy()).to(dev)
        brecv = torch.empty(nq * VERIFY_ROW.itemsize, dtype=torch.uint8, device=dev)
        dist.all_to_all_single(brecv, bsend, output_split_sizes=(plan.n_to * VERIFY_ROW.itemsize).tolist(),
                               input_split_sizes=(plan.n_from * VERIFY_ROW.itemsize).tolist(), group=self.group)
        br = brecv.cpu().numpy().view(VERIFY_ROW)  # row k answers planned request k
        verdict = np.zeros(nq, np.uint8)
        ask = np.nonzero((br["gid"] >= 0) & (br["len"] < rows["len"]))[0] if nq else np.zeros(0, np.int64)
        if len(ask):
            if not np.array_equal(br["gid"][ask], plan.req_gid[ask]):
                raise RuntimeError("verify: the replicas' rows do not follow the plan's requests")
            # each sent log once, at the distinct lengths its replicas reported
            pairs = np.unique(np.stack([plan.req_gid[ask], br["len"][ask].astype(np.int64)], axis=1), axis=0)
            logs, first = np.unique(pairs[:, 0], return_index=True)
            first = np.concatenate([first, [len(pairs)]]).astype(np.uint64)
            at = self.io.digest_prefixes(self.handle[logs].astype(np.uint32), np.full(len(logs), start_epoch, np.int64),
                                         first, pairs[:, 1].astype(np.uint32))
            key = pairs[:, 0] * (1 << 32) + pairs[:, 1]  # (sorted: np.unique orders the rows)
            row = np.searchsorted(key, plan.req_gid[ask] * (1 << 32) + br["len"][ask].astype(np.int64))
            verdict[ask] = (at["hash"][row] != br["hash"][ask]) | (at["len"][row] != br["len"][ask])
        vt = torch.empty(int(plan.n_from.sum()), dtype=torch.uint8, device=dev)
        dist.all_to_all_single(vt, torch.from_numpy(verdict).to(dev), output_split_sizes=plan.n_from.tolist(),
                               input_split_sizes=plan.n_to.tolist(), group=self.group)
        bad = vt.cpu().numpy()[have] != 0
        rep.short_diverged = gid[bad & (mine["len"] < theirs["len"])].tolist()
        return rep

    def first_bad_epoch(self, start_epoch: int, gids: Sequence[int], limit: int = 8) -> "EpochResult":
        """In which epoch does this rank's replica of each of `gids` part from its owner's log?
        Collective: every rank calls it at the same quiescent point with the same `limit` and
        its own gids (flagged by verify, say).  Owner and replica each digest the log at its
        own epoch ends (io.digest_epochs: one row per epoch of getDeterminants(start_epoch),
        the digest of the range up to that epoch's end) and the owner's rows come here:
        three all-to-alls as locate does them -- the requests with static splits (`limit` gid
        slots per rank pair, padded with -1), the row counts with the same splits, then the
        rows with the splits the counts give.  The answer per gid is the first epoch id whose
        rows (id, len, hash) differ -- a copy that merely lags differs in its last epoch --
        or None when all are equal.  No log bytes move: 24 bytes per epoch and log.  Gids
        beyond `limit` per owner rank are returned in `unlocated`.  With one rank no
        collective runs."""
        import torch
        import torch.distributed as dist
        plan = self.plan
        world = plan.world
        want = sorted({int(g) for g in gids})
        if world == 1:
            return EpochResult({}, want)
        if limit < 1:
            raise ValueError("limit must be at least 1")
        if any(self.replica_handle[g] < 0 for g in want):
            raise ValueError("first_bad_epoch: a gid this rank keeps no replica of")
        owner = np.array([owner_rank(int(plan.table.vertex[g]), world) for g in want], np.int64)
        ask = np.full((world, limit), -1, np.int64)
        unlocated: List[int] = []
        for r in range(world):
            of_r = [g for g, o in zip(want, owner) if o == r]
            ask[r, :len(of_r[:limit])] = of_r[:limit]
            unlocated += of_r[limit:]
        backend = dist.get_backend(self.group)
        dev = self.device if backend == "nccl" else "cpu"
        # 1. requests, static splits: asked[r] = the gids rank r wants from this rank
        asked_t = torch.empty(world * limit, dtype=torch.int64, device=dev)
        dist.all_to_all_single(asked_t, torch.from_numpy(ask.reshape(-1).copy()).to(dev), group=self.group)
        asked = asked_t.cpu().numpy().reshape(world, limit)
        live = asked >= 0
        og = asked[live]
        oh = self.handle[og] if len(og) else np.zeros(0, np.int64)
        if len(og) and (oh < 0).any():
            raise ValueError(f"asked for gids this rank does not send: {og[oh < 0][:8].tolist()}")
        # 2. rows per slot, the same splits
        n_out = np.zeros((world, limit), np.int64)
        orow = np.zeros(0, EPOCH_ROW)
        if len(og):
            f, ids, dg = self.io.digest_epochs(oh.astype(np.uint32), np.full(len(og), start_epoch, np.int64))
            n_out[live] = np.diff(np.asarray(f, np.int64))
            orow = np.zeros(len(ids), EPOCH_ROW)
            orow["epoch"], orow["len"], orow["hash"] = ids, dg["len"], dg["hash"]
        n_t = torch.empty(world * limit, dtype=torch.int64, device=dev)
        dist.all_to_all_single(n_t, torch.from_numpy(n_out.reshape(-1).copy()).to(dev), group=self.group)
        n_in = n_t.cpu().numpy().reshape(world, limit)
        # 3. the rows: by destination then slot, as digest_epochs returned them
        to_b, from_b = n_out.sum(axis=1) * EPOCH_ROW.itemsize, n_in.sum(axis=1) * EPOCH_ROW.itemsize
        rt = torch.empty(int(from_b.sum()), dtype=torch.uint8, device=dev)
        dist.all_to_all_single(rt, torch.from_numpy(orow.view(np.uint8).copy()).to(dev),
                               output_split_sizes=from_b.tolist(), input_split_sizes=to_b.tolist(), group=self.group)
        theirs = rt.cpu().numpy().view(EPOCH_ROW)
        filled = ask >= 0
        got = ask[filled]
        out = EpochResult({}, unlocated)
        if not len(got):
            return out
        f, ids, dg = self.io.digest_epochs(self.replica_handle[got].astype(np.uint32),
                                           np.full(len(got), start_epoch, np.int64))
        f = np.asarray(f, np.int64)
        tf = np.concatenate([[0], np.cumsum(n_in[filled])]).astype(np.int64)  # (row-major: owner rank then slot)
        for k, g in enumerate(got.tolist()):
            a = [(int(i), int(d["len"]), int(d["hash"])) for i, d in zip(ids[f[k]:f[k + 1]], dg[f[k]:f[k + 1]])]
            b = [(int(r["epoch"]), int(r["len"]), int(r["hash"])) for r in theirs[tf[k]:tf[k + 1]]]
            same = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            rest = [x[0] for x in (a[same:same + 1] + b[same:same + 1])]
            out[g] = min(rest) if rest else None
        return out


    def locate(self, start_epoch: int, report: VerifyReport, limit: int = 8) -> "LocateResult":
        """Where do the replicas that `report` (this rank's verify(start_epoch)) flags leave
        their owners' logs?  Collective: every rank calls it after verify, at the same quiescent
        point, with the same `limit`.  For up to `limit` flagged gids (short, long, differs) per
        owner rank, this rank fetches the owner's copy and compares its replica with it where
        the bytes arrive (io.diff: device input on the engine).  Three all-to-alls, as exchange
        does it: the requests with static splits (`limit` gid slots per rank pair, padded with
        -1), the copies' lengths with the same splits, and the payload with the splits the
        lengths give (owners fill it with io.copy_lengths / io.copy_batch).  Only the flagged
        logs' bytes move.  Returns a LocateResult: one ReplicaDivergence per fetched gid, and in
        `unlocated` the flagged gids beyond `limit`, which are reported, never dropped.  With
        one rank no collective runs."""
        import torch
        import torch.distributed as dist
        plan = self.plan
        world = plan.world
        flagged = sorted({int(g) for g in list(report.short) + list(report.long) + list(report.differs)})
        if world == 1:
            return LocateResult([], flagged)
        if limit < 1:
            raise ValueError("limit must be at least 1")
        owner = np.array([owner_rank(int(plan.table.vertex[g]), world) for g in flagged], np.int64)
        ask = np.full((world, limit), -1, np.int64)
        unlocated: List[int] = []
        for r in range(world):
            of_r = [g for g, o in zip(flagged, owner) if o == r]
            ask[r, :len(of_r[:limit])] = of_r[:limit]
            unlocated += of_r[limit:]
        backend = dist.get_backend(self.group)
        dev = self.device if backend == "nccl" else "cpu"
        # 1. requests, static splits: asked[r] = the gids rank r wants from this rank
        asked_t = torch.empty(world * limit, dtype=torch.int64, device=dev)
        dist.all_to_all_single(asked_t, torch.from_numpy(ask.reshape(-1).copy()).to(dev), group=self.group)
        asked = asked_t.cpu().numpy().reshape(world, limit)
        live = asked >= 0
        gids = asked[live]
        h = self.handle[gids] if len(gids) else np.zeros(0, np.int64)
        if len(gids) and (h < 0).any():
            raise ValueError(f"asked for gids this rank does not send: {gids[h < 0][:8].tolist()}")
        eps = np.full(len(gids), start_epoch, np.int64)
        # 2. the copies' lengths, the same splits
        lens_out = np.zeros((world, limit), np.int64)
        if len(gids):
            lens_out[live] = self.io.copy_lengths(h.astype(np.uint32), eps)
        lens_t = torch.empty(world * limit, dtype=torch.int64, device=dev)
        dist.all_to_all_single(lens_t, torch.from_numpy(lens_out.reshape(-1).copy()).to(dev), group=self.group)
        lens_in = lens_t.cpu().numpy().reshape(world, limit)
        # 3. the payload: the asked copies back to back, by destination then slot
        bytes_to, bytes_from = lens_out.sum(axis=1), lens_in.sum(axis=1)
        nsend, nrecv = int(bytes_to.sum()), int(bytes_from.sum())
        send = torch.empty(nsend + BLOB_ALIGN, dtype=torch.uint8, device=self.device)
        if len(gids) and self.io.copy_batch(h.astype(np.uint32), eps, send, 0) != nsend:
            raise RuntimeError("the copies changed between measuring and gathering them (not quiescent)")
        recv = torch.empty(max(nrecv, 1) + BLOB_ALIGN, dtype=torch.uint8, device=dev)
        dist.all_to_all_single(recv[:nrecv], _to_comm(send[:nsend], backend), output_split_sizes=bytes_from.tolist(),
                               input_split_sizes=bytes_to.tolist(), group=self.group)
        filled = ask >= 0
        got = ask[filled]
        if not len(got):
            return LocateResult([], unlocated)
        if str(self.device).startswith("cuda") and not recv.is_cuda:  # gloo: into HBM once
            recv = recv.to(self.device)
        ln = lens_in[filled].astype(np.uint64)  # (row-major: by owner rank then slot, as the payload lies)
        offs = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
        rh = self.replica_handle[got].astype(np.uint32)
        eps = np.full(len(got), start_epoch, np.int64)
        rows = self.io.diff(rh, eps, recv, offs, ln)
        out = LocateResult([], unlocated)
        for g, r in zip(got.tolist(), rows):
            lcp, ll, lr = int(r["lcp"]), int(r["len_log"]), int(r["len_ref"])
            kind = ("differs" if lcp < min(ll, lr) else "replica_is_prefix" if ll < lr else
                    "owner_is_prefix" if ll > lr else "equal")
            out.append(ReplicaDivergence(g, lcp, ll, lr, kind))
        part = [k for k, d in enumerate(out) if d.kind != "equal"]
        if part and hasattr(self.io, "locate_records"):
            recs = self.io.locate_records(rh[part], eps[part], recv, offs[part], ln[part], [out[k].offset for k in part])
            for k, r in zip(part, recs):
                d = out[k]
                d.epoch, d.epoch_offset, d.record, d.record_offset, d.replica, d.owner = r
        return out


def rows_sent(rows: np.ndarray) -> int:
    """Header rows that carry a delta (the rest are the static slots of requests with none)."""
    return int((rows["len"] > 0).sum())


# ---- replay-prep merge across GPUs ---------------------------------------------------------
MERGE_GUARD = 64  # bytes before and after the received winners (device gathers read aligned 16-byte words)


class MergedCopies:
    """The winners delivered to one rank: every log's winning copy inside one buffer (an RCCL
    receive buffer in HBM, or host memory over gloo) at place[gid] = (offset, length), with
    MERGE_GUARD bytes around them, ready for clg_replay_prepare_device as they lie.  Also as
    arrays (gids, offsets, lengths), which the batched consumers read."""

    def __init__(self, buf, place: Optional[Dict[int, Tuple[int, int]]] = None, gids=None, offs=None, lens=None,
                 ranks=None):
        self.buf = buf
        if place is not None:
            gids = np.fromiter(place.keys(), np.int64, len(place))
            ol = np.array(list(place.values()), np.int64).reshape(-1, 2)
            offs, lens = ol[:, 0], ol[:, 1]
        self.gids = np.asarray(gids if gids is not None else [], np.int64)
        self.offs = np.asarray(offs if offs is not None else [], np.int64)
        self.lens = np.asarray(lens if lens is not None else [], np.int64)
        self.ranks = np.asarray(ranks if ranks is not None else np.full(len(self.gids), -1), np.int64)  # winner's rank
        self._place = place

    @property
    def place(self) -> Dict[int, Tuple[int, int]]:
        if self._place is None:
            self._place = dict(zip(self.gids.tolist(), zip(self.offs.tolist(), self.lens.tolist())))
        return self._place

    def bytes_of(self, gid: int) -> bytes:
        o, n = self.place[gid]
        return self.buf[o:o + n].cpu().numpy().tobytes() if n else b""

    def as_dict(self) -> Dict[int, bytes]:
        return {g: self.bytes_of(g) for g in self.place}


_GROUP_INFO: Dict[int, tuple] = {}


def _group_info(group) -> Tuple[int, int, str]:
    """(rank, world size, backend) of a process group, looked up once per group object (each
    torch.distributed query goes through its logging wrapper: ~10 us apiece on the merge's
    critical path).  The entry holds the group itself, so a re-initialised default group
    (a new object) is looked up afresh."""
    import torch.distributed as dist
    g = group if group is not None else dist.group.WORLD
    got = _GROUP_INFO.get(id(g))
    if got is None or got[0] is not g:
        got = (g, dist.get_rank(group), dist.get_world_size(group), dist.get_backend(group))
        _GROUP_INFO[id(g)] = got
    return got[1], got[2], got[3]


def copy_arrays(copies) -> Tuple[np.ndarray, np.ndarray]:
    """merge_responses' `copies` as (gids ascending, handles): from a dict gid -> handle, or
    already such a pair (a caller that merges every step converts its dict once)."""
    if isinstance(copies, tuple):
        return copies
    kv = np.fromiter(itertools.chain.from_iterable(copies.items()), np.int64, 2 * len(copies)).reshape(-1, 2)
    ck, cv = kv[:, 0], kv[:, 1]
    if len(ck) > 1 and not (ck[1:] > ck[:-1]).all():  # (callers usually build it in gid order)
        srt = np.argsort(ck)
        ck, cv = ck[srt], cv[srt]
    return ck, cv


def merge_responses(io, table: LogTable, failed: Sequence[int], copies,
                    start_epochs: Dict[int, int], dest_of: Dict[int, int], device, group=None,
                    timing: Optional[Dict[str, float]] = None, verify=False) -> MergedCopies:
    """Cross-GPU DeterminantResponseEvent.merge for the logs of the failed vertices.

    copies: gid -> io handle of this rank's copy (owned log or replica) of a log of a failed
    vertex (a dict, or copy_arrays' pair); start_epochs: failed VertexID -> the epoch the request asks from
    (respondToDeterminantRequest -> getDeterminants(startEpoch), JobCausalLogImpl.java:
    188-204); dest_of: failed VertexID -> rank hosting its replacement.

    Step 1: every rank measures all its copies in one call and reports (len << 8 | rank);
    an all-reduce(MAX) picks, per log, the longest copy (DeterminantResponseEvent.java:
    137-146; equal lengths are equal bytes -- every copy is a prefix of the same log -- so the
    rank tie-break picks identical content).  Step 2: the winners this rank holds are
    gathered in one call, grouped by destination, and one all-to-all carries them to the
    ranks hosting the replacements.  Returns this rank's MergedCopies (a log no rank holds
    is absent, as in the merged map).

    verify=True (off by default): each winning rank also digests its winners where they lie
    (io.digest) and the digests travel beside the lengths, one 8-byte hash per winner in a
    third collective; the destination digests the spans it received (io.digest_spans, device
    input for a buffer in HBM) and raises RuntimeError on a mismatch.

    verify="prefixes" does all of that and checks the assumption of step 1 itself, that every
    losing copy is a prefix of the winner: one all-gather carries each rank's (len, hash) per
    log (len -1: not held), each winning rank digests its winners once at the distinct losing
    lengths (io.digest_prefixes) and, after the last collective, raises RuntimeError naming
    the gids and ranks whose copy is not a prefix of the winner this rank holds."""
    import time as _time
    import torch
    import torch.distributed as dist
    t_in = _time.perf_counter()
    rank, world, backend = _group_info(group)
    if world > 255:
        raise ValueError("rank must fit the packed key's low byte")
    # every per-log step below is an array operation: a failed task has 129 logs at p=128
    fv = np.unique(np.fromiter((int(v) for v in failed), np.int64))
    gids = table.gids_of(fv)
    n = len(gids)
    vslot = np.searchsorted(fv, table.vertex[gids])  # each log's failed vertex, as an index into fv
    ep_of = np.array([start_epochs[int(v)] for v in fv], np.int64)
    dest = np.array([dest_of[int(v)] for v in fv], np.int64)[vslot]
    ck, cv = copy_arrays(copies)
    pos = np.minimum(np.searchsorted(ck, gids), max(len(ck) - 1, 0))
    held = np.nonzero(ck[pos] == gids)[0] if len(ck) else np.zeros(0, np.int64)  # logs this rank holds
    handles = cv[pos[held]]
    epochs = ep_of[vslot[held]]
    key = np.full(max(n, 1), -1, np.int64)
    t0 = _time.perf_counter()
    if timing is not None:
        timing["setup"] = timing.get("setup", 0.0) + t0 - t_in
    if len(held):
        key[held] = (io.copy_lengths(handles, epochs) << 8) | rank
    if timing is not None:  # (developer: the bench's phase split)
        timing["lengths"] = timing.get("lengths", 0.0) + _time.perf_counter() - t0
    if world == 1:  # every copy is this rank's: the winners are gathered in place, nothing moves
        win = key[:n]
        mine = np.nonzero(win >= 0)[0]
        lens = (win[mine] >> 8).astype(np.int64)
        tot = int(lens.sum())
        buf = torch.empty(MERGE_GUARD + max(tot, 1) + MERGE_GUARD, dtype=torch.uint8, device=device)
        t1 = _time.perf_counter()
        if tot:
            sel = np.searchsorted(held, mine)
            got = io.copy_batch(handles[sel], epochs[sel], buf, MERGE_GUARD)
            if got != tot:
                raise RuntimeError(f"logs changed during the merge ({got} != {tot} bytes)")
        t2 = _time.perf_counter()
        if timing is not None:
            timing["gather"] = timing.get("gather", 0.0) + t2 - t1
            timing["alloc"] = timing.get("alloc", 0.0) + t1 - t0
        offs = MERGE_GUARD + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(mine) else lens
        if verify and len(mine):
            sel = np.searchsorted(held, mine)
            _check_winners(io, buf, gids[mine], offs, lens, io.digest(handles[sel], epochs[sel])["hash"])
        res = MergedCopies(buf, gids=gids[mine], offs=offs, lens=lens, ranks=np.zeros(len(mine), np.int64))
        if timing is not None:
            timing["finish"] = timing.get("finish", 0.0) + _time.perf_counter() - t2
        return res
    dev = device if backend == "nccl" else "cpu"
    kt = torch.from_numpy(key).to(dev)
    dist.all_reduce(kt, op=dist.ReduceOp.MAX, group=group)
    win = kt.cpu().numpy()[:n]
    win_rank = np.where(win >= 0, win & 0xFF, -1)
    win_len = np.where(win >= 0, win >> 8, 0)
    mine = np.nonzero(win_rank == rank)[0]
    not_prefix: List[Tuple[int, int]] = []  # (gid, rank) of losing copies that are no prefix of this rank's winner
    if verify == "prefixes":
        said = np.full((max(n, 1), 2), -1, np.int64)
        if len(held):
            dg = io.digest(handles, epochs)
            said[held, 0] = dg["len"].astype(np.int64)
            said[held, 1] = np.ascontiguousarray(dg["hash"]).view(np.int64)
        st = torch.from_numpy(said).to(dev)
        every = [torch.empty_like(st) for _ in range(world)]
        dist.all_gather(every, st, group=group)
        every = np.stack([t.cpu().numpy() for t in every])[:, :n]  # [rank, log, (len, hash)]
        if len(mine):
            sel = np.searchsorted(held, mine)
            lens_l = every[:, mine, 0]  # [rank, winner]
            lose = (lens_l >= 0) & (np.arange(world)[:, None] != rank)
            cuts = [np.unique(lens_l[lose[:, j], j]) for j in range(len(mine))]
            first = np.concatenate([[0], np.cumsum([len(c) for c in cuts])]).astype(np.uint64)
            flat = np.concatenate(cuts).astype(np.uint32) if len(cuts) else np.zeros(0, np.uint32)
            if len(flat):
                at = io.digest_prefixes(handles[sel], epochs[sel], first, flat)
                for j in range(len(mine)):
                    c = cuts[j]
                    for r in np.nonzero(lose[:, j])[0]:
                        k = int(first[j]) + int(np.searchsorted(c, lens_l[r, j]))
                        if (int(at["len"][k]) != int(lens_l[r, j])
                                or int(at["hash"][k]) != int(every[r, mine[j], 1].view(np.uint64))):
                            not_prefix.append((int(gids[mine[j]]), int(r)))
    order = mine[np.argsort(dest[mine], kind="stable")]  # by destination, then log order
    send_split = np.bincount(dest[mine], weights=win_len[mine], minlength=world).astype(np.int64)
    inbound = np.nonzero((win_rank >= 0) & (dest == rank))[0]
    recv_split = np.bincount(win_rank[inbound], weights=win_len[inbound], minlength=world).astype(np.int64)
    send = torch.empty(max(int(send_split.sum()), 1), dtype=torch.uint8, device=device)
    if int(send_split.sum()):
        sel = np.searchsorted(held, order)  # (every winner of this rank is a held log)
        got = io.copy_batch(handles[sel], epochs[sel], send, 0)
        if got != int(send_split.sum()):
            raise RuntimeError(f"logs changed during the merge ({got} != {int(send_split.sum())} bytes)")
    nrecv = int(recv_split.sum())
    buf = torch.empty(MERGE_GUARD + max(nrecv, 1) + MERGE_GUARD, dtype=torch.uint8, device=dev)
    s_in = _to_comm(send, backend)
    dist.all_to_all_single(buf[MERGE_GUARD:MERGE_GUARD + nrecv], s_in[:int(send_split.sum())],
                           output_split_sizes=recv_split.tolist(), input_split_sizes=send_split.tolist(),
                           group=group)
    # received in source-rank order, each source's winners in log order
    recv = inbound[np.lexsort((inbound, win_rank[inbound]))]
    lens = win_len[recv]
    offs = MERGE_GUARD + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(recv) else lens
    if verify:  # the winners' hashes, in the order their bytes went
        hsend = np.zeros(len(order), np.uint64)
        if len(order):
            sel = np.searchsorted(held, order)
            hsend[:] = io.digest(handles[sel], epochs[sel])["hash"]
        n_to = np.bincount(dest[mine], minlength=world).astype(np.int64)
        n_from = np.bincount(win_rank[inbound], minlength=world).astype(np.int64)
        ht = torch.from_numpy(hsend.view(np.int64).copy()).to(dev)
        hr = torch.empty(len(recv), dtype=torch.int64, device=dev)
        dist.all_to_all_single(hr, ht, output_split_sizes=n_from.tolist(), input_split_sizes=n_to.tolist(), group=group)
        _check_winners(io, buf, gids[recv], offs, lens, hr.cpu().numpy().view(np.uint64))
    if not_prefix:
        raise RuntimeError("merged winners are not extensions of every other copy: (gid, rank) "
                           f"{not_prefix[:8]} hold bytes that are no prefix of the winner")
    return MergedCopies(buf, gids=gids[recv], offs=offs, lens=lens, ranks=win_rank[recv])


def _check_winners(io, buf, gids: np.ndarray, offs: np.ndarray, lens: np.ndarray, want_hash: np.ndarray) -> None:
    """merge_responses(verify=True): the received winners' digests against their ranks'."""
    if not len(gids):
        return
    got = io.digest_spans(buf, offs.astype(np.uint64), lens.astype(np.uint64))
    bad = np.nonzero((got["hash"] != want_hash) | (got["len"] != lens.astype(np.uint64)))[0]
    if len(bad):
        raise RuntimeError(f"merged copies differ from the logs their ranks measured: gids {gids[bad][:8].tolist()}")
