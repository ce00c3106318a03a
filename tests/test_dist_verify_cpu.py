"""CPU, world 2 over gloo: Replicator.verify and merge_responses(verify=True) of
clonos_amd/dist.py -- the protocol (owners digest what they send, one all-to-all of
(gid, len, hash) rows with the plan's static splits, receivers digest their replicas) over the
oracle's logs.  The stand-in's digest is the definition restated with Python integers:
p = 2^61 - 1, R = 2654435761, little-endian u32 words zero-padded past the end,
h = (h * R + w) mod p.  The same protocol over real engines is tests/test_gpu_dist_verify.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_dist_cpu import PAR, SEG, STAGES, OracleIO, OracleStore, records, run_world  # noqa: E402

P = (1 << 61) - 1
R = 2654435761


def py_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


def digest_rows(blobs):
    from clonos_amd import DIGEST
    out = np.zeros(len(blobs), DIGEST)
    for i, b in enumerate(blobs):
        out[i] = py_digest(b)
    return out


class DigestIO(OracleIO):
    def digest(self, handles, start_epochs):
        return digest_rows([self.logs[int(h)].get_determinants(int(e))[1] for h, e in zip(handles, start_epochs)])


def verify_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        from clonos_amd import dist as X
        from clonos_amd import job as J
        dist.init_process_group("gloo", rank=rank, world_size=world)
        g = J.dag(STAGES, PAR)
        table = J.LogTable(g)
        plan = X.ReplicationPlan(table, -1, rank, world)
        io = DigestIO()
        owned = {int(gid): io.new_log() for gid in plan.owned}
        rep = X.Replicator(io, plan, "cpu", {gid: h for gid, h in owned.items() if gid in set(plan.send.tolist())})
        for ep in range(2):
            for gid, h in owned.items():
                r = records(table.ids[gid], ep)
                if r:
                    assert io.logs[h].append(ep, r) == 0
            rep.exchange(ep)
        # 1. clean
        v = rep.verify(0)
        assert v.clean and v.short == v.long == v.differs == [] and v.checked == len(plan.wanted) > 0
        # 2. rank 1 holds one replica of the owner's length but with other bytes
        extended = int(X.ReplicationPlan(table, -1, 0, world).send[0])  # the log rank 0 extends in step 3
        altered = -1
        if rank == 1:
            for gid in plan.wanted.tolist():
                h = int(rep.replica_handle[gid])
                b = io.logs[h].get_determinants(0)[1]
                if b and gid != extended:
                    other = io.O.OracleLog(SEG)
                    assert other.append(0, b[:-1] + bytes([b[-1] ^ 0x40])) == 0
                    io.logs[h] = other
                    altered = gid
                    break
            assert altered >= 0
        v = rep.verify(0)
        assert v.differs == ([altered] if rank == 1 else []) and not v.short and not v.long
        # 3. rank 0 appends to one sent log after the exchange: its replica is short
        if rank == 0:
            assert io.logs[owned[extended]].append(1, b"\x00\x07") == 0
        v = rep.verify(0)
        assert v.short == ([extended] if rank == 1 else []) and not v.long
        assert v.differs == ([altered] if rank == 1 else [])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", v.checked))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def test_replicator_verify_gloo():
    res = run_world(verify_worker, world=2)
    assert all(info > 0 for _, _, info in res)


def test_verify_world_1_runs_no_collective():
    from clonos_amd import dist as X
    from clonos_amd import job as J
    table = J.LogTable(J.dag(STAGES, PAR))
    plan = X.ReplicationPlan(table, -1, 0, 1)
    rep = X.Replicator(DigestIO(), plan, "cpu", {})
    v = rep.verify(0)  # (no process group exists: a collective would raise)
    assert v.clean and v.checked == 0


class DigestStore(OracleStore):
    """merge_responses' copies with digests; `corrupt`: the bytes it sends differ from the
    copy it measured (one flipped bit in its first non-empty winner)."""

    def __init__(self, full, cut, rank, corrupt=False):
        super().__init__(full, cut, rank)
        self.corrupt = corrupt

    def digest(self, handles, start_epochs):
        return digest_rows([self.copies[int(h)] for h in handles])

    def digest_spans(self, tensor, offs, lens):
        b = tensor.numpy().tobytes()
        return digest_rows([b[int(o):int(o) + int(n)] for o, n in zip(offs, lens)])

    def copy_batch(self, handles, start_epochs, tensor, off):
        n = super().copy_batch(handles, start_epochs, tensor, off)
        if self.corrupt and n:
            tensor[off] ^= 1
        return n


def merge_verify_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        from clonos_amd import dist as X
        from clonos_amd import job as J
        dist.init_process_group("gloo", rank=rank, world_size=world)
        table = J.LogTable(J.dag(STAGES, PAR))
        failed = [1, 5]
        dest_of = {1: 1, 5: 0}
        full = {gid: records(table.ids[gid], 0, 200) for gid in range(len(table)) if table.vertex[gid] in failed}
        # rank 0 holds every log whole, rank 1 a shorter prefix: rank 0 wins them all
        cut = {gid: [len(b), len(b) // 2] for gid, b in full.items()}
        store = DigestStore(full, cut, rank)
        plain = X.merge_responses(store, table, failed, store.handles, {1: 0, 5: 0}, dest_of, "cpu")
        merged = X.merge_responses(store, table, failed, store.handles, {1: 0, 5: 0}, dest_of, "cpu", verify=True)
        assert merged.as_dict() == plain.as_dict()
        assert merged.as_dict() == {gid: b for gid, b in full.items() if dest_of[int(table.vertex[gid])] == rank}
        # a winner whose bytes change on the way is caught where it arrives
        bad = DigestStore(full, cut, rank, corrupt=True)
        raised = False
        try:
            X.merge_responses(bad, table, failed, bad.handles, {1: 0, 5: 0}, dest_of, "cpu", verify=True)
        except RuntimeError as e:
            raised = "differ" in str(e)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", raised))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def test_merge_verify_gloo():
    res = dict((rank, info) for rank, _, info in run_world(merge_verify_worker, world=2))
    # rank 0 wins every log and flips the first byte it sends, which belongs to the first
    # destination's part: rank 0 itself (its winners pass through the same all-to-all)
    assert res[0] is True and res[1] is False
