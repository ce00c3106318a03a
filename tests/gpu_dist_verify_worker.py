"""Launcher for tests/test_gpu_dist_verify.py: two ranks (gloo transport), one Engine each on
cuda:0, a 3-stage DAG at parallelism 8 under full sharing, two epochs.  Replicator.verify
compares every replica with its owner's log by the device-side digest (clg_digest_logs):

  1. after the first epoch's exchange the report is clean on both ranks;
  2. before the second exchange rank 1 feeds one replica a delta of the owner's length but with
     other bytes; the dedup rule (ThreadCausalLogImpl.java:117-154) then drops the owner's
     delta, so `differs` names exactly that log on rank 1;
  3. rank 0 appends to one sent log after the exchange: `short` names it on rank 1;
  4. merge_responses(verify=True) passes on intact winners and delivers their bytes.

The launcher itself never touches the GPU; each rank is a fresh process.
"""
import os
import socket
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

STAGES, PAR, SEG = 3, 8, 256


def content(gid: int, epoch: int, is_main: bool) -> bytes:
    """Deterministic bytes of log `gid` in `epoch` (every rank can recompute them)."""
    rng = np.random.default_rng(gid * 977 + epoch)
    out = bytearray()
    if is_main:
        for _ in range(int(rng.integers(20, 90))):
            out += (bytes([0, int(rng.integers(0, 4))]) if rng.random() < 0.5 else
                    bytes([1]) + int(rng.integers(0, 1 << 40)).to_bytes(8, "big"))
    else:
        for _ in range(int(rng.integers(0, 6))):
            out += bytes([7]) + int(rng.integers(1, 1 << 15)).to_bytes(4, "big")
    return bytes(out)


def worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        import torch.distributed as dist
        from clonos_amd import Engine
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
        altered = next(int(g) for g in plans[1].wanted if g != extended and body(g, 1))
        # 1. clean after the first epoch
        append_epoch(0)
        rep.exchange(0)
        v = rep.verify(0)
        assert v.clean and v.checked == len(plan.wanted) > 0, (rank, v)
        # 2. a replica of the owner's length with other bytes in the second epoch
        if rank == 1:
            good = body(altered, 1)
            bad = bytes(x ^ 0x10 for x in good[:-1]) + good[-1:]
            ThreadCausalLog(eng, int(rep.replica_handle[altered]), table.ids[altered]).processUpstreamDelta(bad, 0, 1)
        append_epoch(1)
        rep.exchange(1)
        v = rep.verify(0)
        assert v.differs == ([altered] if rank == 1 else []) and not v.short and not v.long, (rank, v)
        v1 = rep.verify(1)  # the same from the second epoch alone
        assert v1.differs == v.differs and not v1.short and not v1.long, (rank, v1)
        # 3. the owner logs on after the exchange
        if rank == 0:
            logs[extended].appendDeterminant(b"\x00\x03", 1)
        v = rep.verify(0)
        assert v.short == ([extended] if rank == 1 else []) and not v.long, (rank, v)
        assert v.differs == ([altered] if rank == 1 else []), (rank, v)
        # 4. the cross-GPU merge with verification, on vertices whose logs are intact
        busy = {int(table.vertex[extended]), int(table.vertex[altered])}
        a = next(x for x in range(PAR) if x not in busy and x + PAR not in busy)
        failed = [a, a + PAR]
        dest_of = {a: 1, a + PAR: 0}
        fg = np.nonzero(np.isin(table.vertex, failed))[0]
        copies = {}
        for gid in fg:
            h = logs[int(gid)].handle if int(gid) in logs else int(rep.replica_handle[gid])
            if h >= 0:
                copies[int(gid)] = h
        mc = X.merge_responses(io, table, failed, copies, {a: 0, a + PAR: 0}, dest_of, dev, verify=True)
        merged = mc.as_dict()
        n = 0
        for gid in fg:
            if dest_of[int(table.vertex[gid])] == rank:
                assert merged.get(int(gid)) == body(gid, 0) + body(gid, 1), (rank, int(gid))
                n += 1
        assert n > 0
        dist.barrier()
        dist.destroy_process_group()
        eng.close()
        q.put((rank, "ok", (v.checked, n)))
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
    print("replicas checked by digest:", [r[2] for r in res if r[1] == "ok"])
    sys.exit(1 if bad else 0)
