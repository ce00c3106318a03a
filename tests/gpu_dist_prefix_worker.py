"""Launcher for tests/test_gpu_dist_prefix.py: two ranks (gloo transport), one Engine each on
cuda:0, a 3-stage DAG at parallelism 8 under full sharing, two epochs.  The prefix protocols of
clonos_amd/dist.py over the device-side prefix digests (clg_digest_prefixes / clg_digest_epochs).

The scene, five of rank 1's replicas of rank 0's main logs (altered by a delta fed to the replica
before the owner's arrives -- the dedup rule, ThreadCausalLogImpl.java:117-154, then drops the
owner's -- and by appends after the exchange):

  lagging     the owner appends after the exchange: a true prefix
  short_bad   a byte of epoch 0 changed, and the owner appends after the exchange
  long_ok     the replica got the owner's epoch 1 plus two more bytes
  long_bad    the same with a byte of epoch 1 changed
  equal_bad   the owner's length, a byte of epoch 1 changed

  1. verify(0, prefixes=True) sorts them into short / long / differs as verify(0) does and names
     short_bad and long_bad as diverged;
  2. only_diverged() feeds locate: three logs move, each parts at the changed byte;
  3. first_bad_epoch names the epoch of the changed byte (a lagging copy differs in its last);
  4. merge_responses(verify="prefixes") passes on intact vertices and, for long_bad's vertex,
     raises on the rank holding the winner (rank 1: its replica is the longest copy).

The launcher itself never touches the GPU; each rank is a fresh process.
"""
import os
import socket
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gpu_dist_verify_worker import PAR, SEG, STAGES, content  # noqa: E402


def flip(b: bytes, p: int) -> bytes:
    return b[:p] + bytes([b[p] ^ 0x10]) + b[p + 1:]


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

        def feed(gid, delta, ep):  # rank 1: into its replica before the owner's delta arrives
            ThreadCausalLog(eng, int(rep.replica_handle[gid]), table.ids[gid]).processUpstreamDelta(delta, 0, ep)

        # both ranks name the same five logs: main logs of rank 0, on five vertices, replicated on rank 1
        picks, seen = [], set()
        for g in plans[0].send.tolist():
            v = int(table.vertex[g])
            if table.ids[g].is_main and g in set(plans[1].wanted.tolist()) and v not in seen:
                picks.append(int(g))
                seen.add(v)
        lagging, short_bad, long_ok, long_bad, equal_bad = picks[:5]
        b0 = {g: body(g, 0) for g in picks[:5]}
        b1 = {g: body(g, 1) for g in picks[:5]}
        where = {}
        if rank == 1:
            p = len(b0[short_bad]) // 2
            feed(short_bad, flip(b0[short_bad], p), 0)
            where[short_bad] = p
        append_epoch(0)
        rep.exchange(0)
        if rank == 1:
            feed(long_ok, b1[long_ok] + b"\x00\x01", 1)
            p = len(b1[long_bad]) // 2
            feed(long_bad, flip(b1[long_bad], p) + b"\x00\x02", 1)
            where[long_bad] = len(b0[long_bad]) + p
            p = len(b1[equal_bad]) - 1
            feed(equal_bad, flip(b1[equal_bad], p), 1)
            where[equal_bad] = len(b0[equal_bad]) + p
        append_epoch(1)
        rep.exchange(1)
        if rank == 0:  # the owner logs on after the exchange
            logs[lagging].appendDeterminant(b"\x00\x03", 1)
            logs[short_bad].appendDeterminant(b"\x00\x03", 1)
        # 1. verify with prefixes
        plain = rep.verify(0)
        v = rep.verify(0, prefixes=True)
        assert (v.short, v.long, v.differs, v.checked) == (plain.short, plain.long, plain.differs, plain.checked), (rank, v)
        if rank == 1:
            assert sorted(v.short) == sorted([lagging, short_bad]) and sorted(v.long) == sorted([long_ok, long_bad]), v
            assert v.differs == [equal_bad] and v.short_diverged == [short_bad] and v.long_diverged == [long_bad], v
        else:
            assert v.clean and v.diverged == [], v
        v1 = rep.verify(1, prefixes=True)  # from the second epoch alone short_bad merely lags
        if rank == 1:
            assert sorted(v1.short) == sorted([lagging, short_bad]) and v1.short_diverged == [], v1
            assert v1.long_diverged == [long_bad] and v1.differs == [equal_bad], v1
        # 2. only the diverged logs move
        res = rep.locate(0, v.only_diverged())
        assert res.unlocated == [], (rank, res.unlocated)
        assert sorted((d.gid, d.offset, d.kind) for d in res) == sorted((g, p, "differs") for g, p in where.items())
        # 3. the epoch of the changed byte
        asked = picks[:5] if rank == 1 else []
        fb = rep.first_bad_epoch(0, asked)
        assert fb.unlocated == []
        if rank == 1:
            assert fb == {lagging: 1, short_bad: 0, long_ok: 1, long_bad: 1, equal_bad: 1}, fb
        else:
            assert fb == {}
        # 4. the merge: intact vertices pass ...
        busy = {int(table.vertex[g]) for g in picks[:5]}
        a = next(x for x in range(PAR) if x not in busy and x + PAR not in busy)

        def merge(failed, dest_of, mode):
            fg = np.nonzero(np.isin(table.vertex, failed))[0]
            copies = {}
            for gid in fg:
                h = logs[int(gid)].handle if int(gid) in logs else int(rep.replica_handle[gid])
                if h >= 0:
                    copies[int(gid)] = h
            return fg, X.merge_responses(io, table, failed, copies, {x: 0 for x in failed}, dest_of, dev, verify=mode)

        dest_of = {a: 1, a + PAR: 0}
        fg, mc = merge([a, a + PAR], dest_of, "prefixes")
        merged = mc.as_dict()
        n = 0
        for gid in fg:
            if dest_of[int(table.vertex[gid])] == rank:
                assert merged.get(int(gid)) == body(gid, 0) + body(gid, 1), (rank, int(gid))
                n += 1
        assert n > 0
        # ... and the vertex of long_bad does not: rank 1's replica is the longest copy and wins, and the
        # owner's copy is no prefix of it; verify=True alone sees nothing (the winner arrives intact)
        fv = int(table.vertex[long_bad])
        merge([fv], {fv: 0}, True)
        said = ""
        try:
            merge([fv], {fv: 0}, "prefixes")
        except RuntimeError as e:
            said = str(e)
        assert (f"({long_bad}, 0)" in said) == (rank == 1) and (said == "") == (rank == 0), (rank, said)
        dist.barrier()
        dist.destroy_process_group()
        eng.close()
        q.put((rank, "ok", (len(v.diverged), n)))
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
    print("replicas sorted by prefix digests:", sorted(r[2] for r in res if r[1] == "ok"))
    sys.exit(1 if bad else 0)
