"""CPU, world 2 over gloo: the prefix protocols of clonos_amd/dist.py over the oracle's logs --
Replicator.verify(prefixes=True), VerifyReport.only_diverged() into Replicator.locate,
Replicator.first_bad_epoch and merge_responses(verify="prefixes").  The stand-in's digests are
the definition restated with Python integers: p = 2^61 - 1, R = 2654435761, little-endian u32
words zero-padded past the end, h = (h * R + w) mod p; the row of a cut c over a range b is
{hash(b[:min(c, len b)]), min(c, len b)}.  The same protocols over real engines are
tests/test_gpu_dist_prefix.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_dist_cpu import PAR, SEG, STAGES, records, run_world  # noqa: E402
from test_dist_locate_cpu import LocateIO  # noqa: E402
from test_dist_verify_cpu import DigestStore, digest_rows  # noqa: E402


def prefix_rows(blobs, first, cuts):
    first = np.asarray(first, np.int64)
    assert first[0] == 0 and first[-1] == len(cuts) and len(first) == len(blobs) + 1
    out = []
    for i, b in enumerate(blobs):
        c = [int(x) for x in cuts[first[i]:first[i + 1]]]
        assert c == sorted(c), "cuts of one request must not decrease"
        out += [b[:min(x, len(b))] for x in c]
    return digest_rows(out)


class PrefixIO(LocateIO):
    """LocateIO (an OracleIO with digests, copies and a Python diff) with prefix digests."""

    def digest_prefixes(self, handles, start_epochs, first, cuts):
        return prefix_rows([self._bytes(h, e) for h, e in zip(handles, start_epochs)], first, cuts)

    def digest_epochs(self, handles, start_epochs):
        first, ids, blobs = [0], [], []
        for h, e in zip(handles, start_epochs):
            st = self.logs[int(h)].state()
            eps = sorted(st["epochs"])
            if int(e) in dict(eps):
                eps = [(i, o) for i, o in eps if i >= int(e)]
            b = self._bytes(h, e)
            if eps:
                s = eps[0][1]
                ends = [o - s for _, o in eps[1:]] + [st["writer"] - s]
                assert ends[-1] == len(b)
                ids += [i for i, _ in eps]
                blobs += [b[:x] for x in ends]
            first.append(len(ids))
        return np.array(first, np.uint64), np.array(ids, np.int64), digest_rows(blobs)


def flip(b: bytes, p: int) -> bytes:
    return b[:p] + bytes([b[p] ^ 0x40]) + b[p + 1:]


def prefix_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        from clonos_amd import dist as X
        from clonos_amd import job as J
        dist.init_process_group("gloo", rank=rank, world_size=world)
        table = J.LogTable(J.dag(STAGES, PAR))
        plan = X.ReplicationPlan(table, -1, rank, world)
        io = PrefixIO()
        owned = {int(gid): io.new_log() for gid in plan.owned}
        rep = X.Replicator(io, plan, "cpu", {gid: h for gid, h in owned.items() if gid in set(plan.send.tolist())})
        for ep in range(2):
            for gid, h in owned.items():
                r = records(table.ids[gid], ep)
                if r:
                    assert io.logs[h].append(ep, r) == 0
            rep.exchange(ep)
        v = rep.verify(0, prefixes=True)
        assert v.clean and v.diverged == [] and v.short_diverged == v.long_diverged == [] and v.checked > 0
        assert rep.first_bad_epoch(0, plan.wanted[:3].tolist()) == {int(g): None for g in plan.wanted[:3]}

        # the scene: five of rank 1's replicas of rank 0's logs, each with bytes in both epochs
        sent0 = X.ReplicationPlan(table, -1, 0, world).send.tolist()
        e0 = {g: records(table.ids[g], 0) for g in sent0}
        e1 = {g: records(table.ids[g], 1) for g in sent0}
        picks = [g for g in sent0 if len(e0[g]) >= 4 and len(e1[g]) >= 4][:5]
        assert len(picks) == 5
        lagging, short_bad, long_ok, long_bad, equal_bad = picks
        where = {}  # gid -> (first differing byte, the epoch it lies in)

        def replace(gid, b0, b1):
            log = io.O.OracleLog(SEG)
            assert log.append(0, b0) == 0 and log.append(1, b1) == 0
            io.logs[int(rep.replica_handle[gid])] = log

        if rank == 0:  # the owner appends after the exchange: its replica lags, a true prefix
            assert io.logs[owned[lagging]].append(1, b"\x00\x07") == 0
        else:
            g = short_bad  # shorter, and one byte of the common part (in epoch 0) changed
            p = len(e0[g]) // 2
            replace(g, flip(e0[g], p), e1[g][:-1])
            where[g] = (p, 0)
            g = long_ok  # longer, the common part intact
            assert io.logs[int(rep.replica_handle[g])].append(1, b"\x00\x01\x00\x02") == 0
            g = long_bad  # longer, and one byte of the common part (in epoch 1) changed
            p = len(e1[g]) // 2
            replace(g, e0[g], flip(e1[g], p) + b"\x00\x03")
            where[g] = (len(e0[g]) + p, 1)
            g = equal_bad  # the owner's length, one byte (in epoch 1) changed
            p = len(e1[g]) - 1
            replace(g, e0[g], flip(e1[g], p))
            where[g] = (len(e0[g]) + p, 1)

        plain = rep.verify(0)
        v = rep.verify(0, prefixes=True)
        assert (v.short, v.long, v.differs, v.checked) == (plain.short, plain.long, plain.differs, plain.checked)
        assert plain.short_diverged == plain.long_diverged == []  # (the default asks nothing more)
        if rank == 1:
            assert sorted(v.short) == sorted([lagging, short_bad]) and sorted(v.long) == sorted([long_ok, long_bad])
            assert v.differs == [equal_bad]
            assert v.short_diverged == [short_bad] and v.long_diverged == [long_bad]
            assert v.diverged == sorted([short_bad, long_bad, equal_bad])
        else:
            assert v.clean and v.diverged == []
        # only the diverged logs move bytes
        od = v.only_diverged()
        assert sorted(od.short + od.long + od.differs) == v.diverged
        res = rep.locate(0, od)
        assert res.unlocated == []
        assert sorted((d.gid, d.offset, d.kind) for d in res) == sorted((g, p, "differs") for g, (p, _) in where.items())
        # the epoch of the changed byte, from 24 bytes per epoch
        asked = picks if rank == 1 else []
        fb = rep.first_bad_epoch(0, asked)
        assert fb.unlocated == []
        if rank == 1:
            assert fb == {lagging: 1, short_bad: 0, long_ok: 1, long_bad: 1, equal_bad: 1}
        else:
            assert fb == {}
        few = rep.first_bad_epoch(0, asked, limit=2)
        assert few == {g: fb[g] for g in sorted(asked)[:2]} and few.unlocated == sorted(asked)[2:]
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", len(v.diverged)))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def test_replicator_prefixes_gloo():
    res = dict((rank, info) for rank, _, info in run_world(prefix_worker, world=2))
    assert res == {0: 0, 1: 3}


def test_prefixes_world_1_runs_no_collective():
    from clonos_amd import dist as X
    from clonos_amd import job as J
    table = J.LogTable(J.dag(STAGES, PAR))
    plan = X.ReplicationPlan(table, -1, 0, 1)
    rep = X.Replicator(PrefixIO(), plan, "cpu", {})
    v = rep.verify(0, prefixes=True)  # (no process group exists: a collective would raise)
    assert v.clean and v.checked == 0 and v.only_diverged().clean
    fb = rep.first_bad_epoch(0, [])
    assert fb == {} and fb.unlocated == []


def test_verify_report_fields():
    from clonos_amd.dist import VerifyReport
    v = VerifyReport([3, 9], [4], [7], 5, short_diverged=[9], long_diverged=[])
    assert v.diverged == [7, 9] and not v.clean
    od = v.only_diverged()
    assert (od.short, od.long, od.differs, od.checked) == ([9], [], [7], 5) and od.diverged == [7, 9]
    assert VerifyReport([], [], []).short_diverged == []


class PrefixStore(DigestStore):
    def digest_prefixes(self, handles, start_epochs, first, cuts):
        return prefix_rows([self.copies[int(h)] for h in handles], first, cuts)


def merge_prefix_worker(rank, world, port, q):
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
        # rank 0 holds every log whole, rank 1 a shorter prefix (one log at full length): rank 0 wins them all
        whole = max(full, key=lambda g: len(full[g]))
        cut = {gid: [len(b), len(b) if gid == whole else len(b) // 2] for gid, b in full.items()}
        args = (table, failed)
        eps = {1: 0, 5: 0}
        store = PrefixStore(full, cut, rank)
        want = {gid: b for gid, b in full.items() if dest_of[int(table.vertex[gid])] == rank}
        # every loser is a prefix: all three modes agree
        for mode in (False, True, "prefixes"):
            got = X.merge_responses(store, *args, store.handles, eps, dest_of, "cpu", verify=mode)
            assert got.as_dict() == want, mode
        # rank 1's copy of one log diverged inside its (shorter) length: only "prefixes" sees it,
        # on the rank that holds the winner
        bad_gid = next(g for g in sorted(full) if cut[g][1] >= 2 and g != whole)
        bad = PrefixStore(full, cut, rank)
        if rank == 1:
            bad.copies[bad_gid] = flip(bad.copies[bad_gid], 1)
        for mode in (False, True):
            assert X.merge_responses(bad, *args, bad.handles, eps, dest_of, "cpu", verify=mode).as_dict() == want
        said = ""
        try:
            X.merge_responses(bad, *args, bad.handles, eps, dest_of, "cpu", verify="prefixes")
        except RuntimeError as e:
            said = str(e)
        if rank == 0:
            assert f"({bad_gid}, 1)" in said and "prefix" in said
        else:
            assert said == ""
        # a copy of the winner's length with other bytes is no prefix either
        eq = PrefixStore(full, cut, rank)
        if rank == 1:
            eq.copies[whole] = flip(eq.copies[whole], len(full[whole]) - 1)
        said = ""
        try:
            X.merge_responses(eq, *args, eq.handles, eps, dest_of, "cpu", verify="prefixes")
        except RuntimeError as e:
            said = str(e)
        # (equal lengths: the higher rank wins the tie, so rank 1 holds the winner and names rank 0)
        assert (f"({whole}, 0)" in said) == (rank == 1) and (said == "") == (rank == 0)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", 1))
    except Exception:
        import traceback
        q.put((rank, "fail", traceback.format_exc()))


def test_merge_prefixes_gloo():
    run_world(merge_prefix_worker, world=2)
