"""CPU, world 2 over gloo: Replicator.locate of clonos_amd/dist.py -- the protocol (a request
all-to-all of `limit` gid slots per rank pair, the copies' lengths with the same splits, the
payload with the splits the lengths give, then the holder's comparison) over the oracle's logs.
The stand-in's diff is os.path.commonprefix.  The same protocol over real engines is
tests/test_gpu_dist_locate.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_dist_cpu import PAR, SEG, STAGES, OracleIO, OracleStore, records, run_world  # noqa: E402
from test_dist_verify_cpu import digest_rows  # noqa: E402


class LocateIO(OracleIO, OracleStore):
    """OracleIO's logs with digests, OracleStore's copies (taken from the logs when they are
    measured) and a Python diff."""

    def __init__(self):
        OracleIO.__init__(self)
        self.copies = {}

    def _bytes(self, h, e):
        return self.logs[int(h)].get_determinants(int(e))[1]

    def digest(self, handles, start_epochs):
        return digest_rows([self._bytes(h, e) for h, e in zip(handles, start_epochs)])

    def copy_lengths(self, handles, start_epochs):
        self.copies = {int(h): self._bytes(h, e) for h, e in zip(handles, start_epochs)}
        return OracleStore.copy_lengths(self, handles, start_epochs)

    def diff(self, handles, start_epochs, tensor, offs, lens):
        from clonos_amd import DIFF
        buf = tensor.numpy().tobytes()
        out = np.zeros(len(handles), DIFF)
        for i, (h, e, o, n) in enumerate(zip(handles, start_epochs, offs, lens)):
            mine, ref = self._bytes(h, e), buf[int(o):int(o) + int(n)]
            out[i] = (len(os.path.commonprefix([mine, ref])), len(mine), len(ref))
        return out


def locate_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        from clonos_amd import dist as X
        from clonos_amd import job as J
        dist.init_process_group("gloo", rank=rank, world_size=world)
        table = J.LogTable(J.dag(STAGES, PAR))
        plan = X.ReplicationPlan(table, -1, rank, world)
        io = LocateIO()
        owned = {int(gid): io.new_log() for gid in plan.owned}
        rep = X.Replicator(io, plan, "cpu", {gid: h for gid, h in owned.items() if gid in set(plan.send.tolist())})
        for ep in range(2):
            for gid, h in owned.items():
                r = records(table.ids[gid], ep)
                if r:
                    assert io.logs[h].append(ep, r) == 0
            rep.exchange(ep)

        def key(ds):
            return sorted((d.gid, d.offset, d.len_replica, d.len_owner, d.kind) for d in ds)

        # 1. a clean report: nothing to locate (the collectives still run, with empty slots)
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert v.clean and res == [] and res.unlocated == []

        # rank 1's replicas of rank 0's logs with at least 4 bytes: three of them go wrong
        sent0 = X.ReplicationPlan(table, -1, 0, world).send.tolist()
        full = {g: b"".join(records(table.ids[g], ep) for ep in range(2)) for g in sent0}
        picks = [g for g in sent0 if len(full[g]) >= 4][:3]
        assert len(picks) == 3
        altered, lagging, longer = picks
        want = []
        # 2. an altered replica: the owner's length, one other byte in the middle
        if rank == 1:
            b = full[altered]
            p = len(b) // 2
            other = io.O.OracleLog(SEG)
            assert other.append(0, b[:p] + bytes([b[p] ^ 0x40]) + b[p + 1:]) == 0
            io.logs[int(rep.replica_handle[altered])] = other
            want.append((altered, p, len(b), len(b), "differs"))
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert v.differs == ([altered] if rank == 1 else []) and key(res) == sorted(want) and res.unlocated == []
        # 3. a lagging replica: the owner appended after the exchange
        if rank == 0:
            assert io.logs[owned[lagging]].append(1, b"\x00\x07") == 0
        else:
            n = len(full[lagging])
            want.append((lagging, n, n, n + 2, "replica_is_prefix"))
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert v.short == ([lagging] if rank == 1 else []) and key(res) == sorted(want) and res.unlocated == []
        # two flagged gids of one owner and room for one: the other is reported, not dropped
        res = rep.locate(0, v, limit=1)
        first, second = sorted([altered, lagging])
        assert key(res) == ([w for w in want if w[0] == first] if rank == 1 else [])
        assert res.unlocated == ([second] if rank == 1 else [])
        # 4. a replica that is longer than its owner's log
        if rank == 1:
            assert io.logs[int(rep.replica_handle[longer])].append(1, b"\x00\x01\x00\x02") == 0
            n = len(full[longer])
            want.append((longer, n, n + 4, n, "owner_is_prefix"))
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert v.long == ([longer] if rank == 1 else []) and key(res) == sorted(want) and res.unlocated == []
        assert all(d.epoch is None and d.record is None for d in res)  # this stand-in offers no records
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", len(res)))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def test_replicator_locate_gloo():
    res = dict((rank, info) for rank, _, info in run_world(locate_worker, world=2))
    assert res == {0: 0, 1: 3}


def test_locate_world_1_runs_no_collective():
    from clonos_amd import dist as X
    from clonos_amd import job as J
    table = J.LogTable(J.dag(STAGES, PAR))
    plan = X.ReplicationPlan(table, -1, 0, 1)
    rep = X.Replicator(LocateIO(), plan, "cpu", {})
    res = rep.locate(0, rep.verify(0))  # (no process group exists: a collective would raise)
    assert res == [] and res.unlocated == []
