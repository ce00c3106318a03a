"""Launcher for tests/test_gpu_dist_locate.py: two ranks (gloo transport), one Engine each on
cuda:0, a 3-stage DAG at parallelism 8 under full sharing, two epochs.  After Replicator.verify
has flagged a replica, Replicator.locate fetches the owner's copy of that log alone and compares
it with the replica on the device (clg_diff_logs, device input):

  1. after the first epoch's exchange the report is clean and locate returns [] on both ranks;
  2. before the second exchange rank 1 feeds one replica a delta of the owner's length but with
     other bytes; the dedup rule (ThreadCausalLogImpl.java:117-154) then drops the owner's
     delta: locate names the first altered byte, epoch 1, and the record on both sides;
  3. rank 0 appends to one sent log after the exchange: its replica is a prefix of it.

The expected record fields come from the CPU oracle's decode of the two byte strings under
locate_divergence's record rule.  The launcher itself never touches the GPU; each rank is a
fresh process.
"""
import os
import socket
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gpu_dist_verify_worker import PAR, SEG, STAGES, content  # noqa: E402


def record_rule(mine: bytes, theirs: bytes, offset: int):
    """(record, record_offset, this side's determinant, the other's) for two byte strings that
    part at `offset`: k_side = the side's decoded records with off <= offset, record =
    max(k) - 1, a side's determinant its record at that index when it has one."""
    import _oracle as O
    import numpy as np
    from clonos_amd import DecodedBatch
    sides = []
    for b in (mine, theirs):
        _, r, _, _ = O.decode(b)
        n = len(r["off"])
        batch = DecodedBatch(r["off"], r["tag"], r["v0"], r["w_idx"], r["w_rc"], r["w_v1"], r["w_var_off"],
                             r["w_var_len"], r["w_sub"], np.array([0, n], np.uint64), [np.frombuffer(b, np.uint8)])
        sides.append(([int(o) for o in r["off"]], batch))
    rec = max(sum(o <= offset for o in offs) for offs, _ in sides) - 1
    dets = [batch.determinant_at(0, rec) if rec < len(offs) else None for offs, batch in sides]
    at = next(offs[rec] for offs, _ in sides if rec < len(offs))
    return rec, at, dets[0], dets[1]


def worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        import torch.distributed as dist
        from clonos_amd import Engine
        from clonos_amd import determinants as D
        from clonos_amd import dist as X
        from clonos_amd import job as J
        from clonos_amd.engine import ThreadCausalLog
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda", 0)
        table = J.LogTable(J.dag(STAGES, PAR))
        plans = [X.ReplicationPlan(table, -1, r, world) for r in range(world)]
        plan = plans[rank]
        eng = Engine(segment_bytes=SEG, pool_segments=8192, device=0, ifl_pool_segments=16)
        io = X.EngineIO(eng)
        logs = {int(gid): eng.open_log(table.ids[gid]) for gid in plan.owned}
        send = set(plan.send.tolist())
        rep = X.Replicator(io, plan, dev, {g: l.handle for g, l in logs.items() if g in send})

        def body(gid, ep):
            return content(int(gid), ep, table.ids[gid].is_main)

        def append_epoch(ep):
            for gid, l in logs.items():
                b = body(gid, ep)
                if b:
                    l.appendDeterminant(b, ep)

        # both ranks name the same two logs: the one rank 0 extends, the one rank 1 alters
        extended = int(plans[0].send[0])
        altered = next(int(g) for g in plans[1].wanted if g != extended and len(body(g, 1)) >= 2 and body(g, 0))
        # 1. clean after the first epoch: nothing to locate
        append_epoch(0)
        rep.exchange(0)
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert v.clean and res == [] and res.unlocated == [], (rank, v, res)
        # 2. a replica of the owner's length with other bytes in the second epoch
        good = body(altered, 1)
        bad = bytes(x ^ 0x10 for x in good[:-1]) + good[-1:]
        if rank == 1:
            ThreadCausalLog(eng, int(rep.replica_handle[altered]), table.ids[altered]).processUpstreamDelta(bad, 0, 1)
        append_epoch(1)
        rep.exchange(1)
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert res.unlocated == [], (rank, res.unlocated)
        if rank == 0:
            assert v.clean and res == [], (rank, v, res)
        else:
            assert v.differs == [altered] and len(res) == 1, (rank, v, res)
            (d,) = res
            e0 = body(altered, 0)
            first = next(k for k in range(len(good)) if good[k] != bad[k])
            assert (d.gid, d.kind, d.offset) == (altered, "differs", len(e0) + first), d
            assert d.len_replica == d.len_owner == len(e0 + good) and (d.epoch, d.epoch_offset) == (1, first), d
            assert (d.record, d.record_offset, d.replica, d.owner) == record_rule(e0 + bad, e0 + good, d.offset), d
            assert d.owner is not None and D.encode(d.owner) == good[:len(D.encode(d.owner))]
        # 3. the owner logs on after the exchange: the replica lags
        if rank == 0:
            logs[extended].appendDeterminant(b"\x00\x03", 1)
        v = rep.verify(0)
        res = rep.locate(0, v)
        assert res.unlocated == [], (rank, res.unlocated)
        if rank == 0:
            assert res == [], (rank, res)
        else:
            assert sorted(d.gid for d in res) == sorted([altered, extended]), (rank, res)
            d = next(x for x in res if x.gid == extended)
            whole = body(extended, 0) + body(extended, 1)
            assert (d.kind, d.offset, d.len_replica, d.len_owner) == ("replica_is_prefix", len(whole), len(whole),
                                                                      len(whole) + 2), d
            assert (d.record, d.record_offset, d.replica, d.owner) == record_rule(whole, whole + b"\x00\x03", d.offset), d
            assert d.replica is None and d.owner == D.OrderDeterminant(3), d
            # from the second epoch alone the offsets are relative to that epoch's start
            (d1,) = [x for x in rep.locate(1, rep.verify(1)) if x.gid == altered]
            assert (d1.kind, d1.offset, d1.epoch) == ("differs", first, 1), d1
        if rank == 0:
            rep.locate(1, rep.verify(1))  # (collective: both ranks call it)
        dist.barrier()
        dist.destroy_process_group()
        eng.close()
        q.put((rank, "ok", len(res)))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


if __name__ == "__main__":
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in res if r[1] != "ok"]
    for r in bad:
        print(r[2], file=sys.stderr)
    print("replicas located:", sorted((r[0], r[2]) for r in res if r[1] == "ok"))
    sys.exit(1 if bad else 0)
