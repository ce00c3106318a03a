"""GPU: the byte copy under every gather and scatter (copy_range in kernels.hip, called by
k_gather and k_scatter) at every alignment and length edge, bit-exact against plain slicing of
the bytes that were written.

What is swept (the scenes are in _copy_scenes.py; test_copy_edges_scene.py checks their coverage
without a GPU):
  1. gather, short ranges: the last L bytes of 16 epochs that end on every residue mod 16, L in
     1..33 and around 48, 64 and 80, into an output base at every residue -- every (source
     residue, destination residue, L) triple, at 64-byte segments (ranges of one to three
     pieces) and 16 KiB ones; packed in one batch (synchronous and CLG_F_ASYNC_SLICE) and one
     request per call, each into its own 256-byte slot, where a store that spills over either
     edge of a range stays visible; launches of 1..25 blocks and of 16 + r blocks, r in 0..7
     (the block-to-piece remap over the XCDs); host-planned pieces (clg_get_determinants into
     device memory).
  2. the trip loop: gather pieces of 1024 chunks (one trip) and 1025 (a second trip of one
     chunk), scatter chunks of 256, 257, 512, 513 and 1024 destination chunks (a wave's trip is
     256), at source, writer and output residues 0, 1 and 15 (7 too for the output).
  3. scatter, short ranges: a log per (writer residue, source residue, L), device input, leads
     in one batch and bodies in a second; bodies that end on a segment's last byte and bodies
     that start on a segment's first byte, so a spill past either lands in another log's
     segment; and host-staged appends flushed from packed staging offsets.
  4. the in-flight pool: buffers logged from every source residue, replayed into device memory
     at base residues 0, 1, 7 and 15.

Data bytes are 1..254; destination buffers and the gaps between source bodies hold 0xFF, so a
missing store reads 0xFF and a skipped load (copy_range zero-fills it) 0x00.  Every check reads
what is in HBM: device output, or clg_log_read_phys -- never a host-kind read the host tail
could answer.  A device-output check compares the whole buffer: 16 bytes and the base's residue
before the output, at least 64 bytes after it.

What cannot be observed: a scatter's spill past the writer inside the log's own segment (the
next append overwrites it, nothing reads it, it is harmless), and in the packed batches a spill
that a neighbouring range's block overwrites later.  Whether loads stay inside the pages of
their range is not tested here.
"""
import ctypes as C

import numpy as np
import pytest

import _copy_scenes as S
from _devbuf import DeviceBuf
from clonos_amd import CausalLogID, Engine, _lib, inflight
from clonos_amd import dist as X
from clonos_amd._lib import check, lib

pytestmark = pytest.mark.gpu

LEAD = 16  # bytes of every output buffer before the (16-byte aligned) base the residue is added to


def assert_same(got, want, what):
    """got == want; on a difference the first differing place, not two buffers."""
    got, want = bytes(got), bytes(want)
    if got == want:
        return
    assert len(got) == len(want), what
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.flatnonzero(g != w)
    i = int(bad[0])
    lo = max(i - 4, 0)
    raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {i} (..{int(bad[-1])}): got "
                         f"{got[lo:i + 20].hex()} want {want[lo:i + 20].hex()} (from {lo})")


def slice_reqs(handles, epochs):
    """Request k on channel (k + 1, 0)."""
    req = np.zeros(len(handles), X.SLICE_REQ)
    req["log"], req["epoch"] = handles, epochs
    req["ch_lo"] = np.arange(1, len(handles) + 1)
    return req


def seek(eng, req, offs):
    offs = np.ascontiguousarray(offs, np.int32)
    check(lib.clg_consumer_seek_batch(eng.handle, req.ctypes.data, offs.ctypes.data, len(req)))


def slice_device(eng, req, out, cap):
    res = np.zeros(len(req), X.SLICE_RES)
    total = C.c_uint64()
    check(lib.clg_slice_batch(eng.handle, req.ctypes.data, len(req), res.ctypes.data, out, cap, _lib.CLG_MEM_DEVICE,
                              C.byref(total)))
    eng.sync()
    return res, total.value


def check_res(res, lens, offs=None):
    """Every request served, packed in request order."""
    lens = np.asarray(lens)
    assert (res["status"] == 0).all() and (res["has_delta"] == 1).all()
    assert (res["len"] == lens).all()
    assert (res["out_off"] == np.cumsum(lens) - lens).all()
    if offs is not None:
        assert (res["offset_from_epoch"] == np.asarray(offs)).all()


def upload(buf):
    """A host array as device input (torch, as test_gpu_log.py's upstream batches)."""
    import torch
    d = torch.from_numpy(buf).to("cuda")
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    return d


def upstream_device(eng, handles, epoch, pos, lens, d):
    reqs = np.zeros(len(handles), X.DELTA_REQ)
    reqs["log"], reqs["epoch"], reqs["src_off"], reqs["len"] = handles, epoch, pos, lens
    check(lib.clg_upstream_delta_batch(eng.handle, reqs.ctypes.data, len(reqs), d.data_ptr(), _lib.CLG_MEM_DEVICE))
    assert (reqs["status"] == 0).all()


# ---- 1. gather, short ranges, every alignment ------------------------------------------------------
def short_engine(seg, **kw):
    """The log of 16 epochs, flushed; its epoch offsets as the scene has them."""
    eng = Engine(segment_bytes=seg, pool_segments=256, ifl_pool_segments=16, **kw)
    log = eng.open_log(CausalLogID.main(1))
    data, starts = S.short_log(), S.epoch_starts()
    for t in range(16):
        log.appendDeterminant(data[starts[t]:starts[t] + S.EPOCH_LENS[t]], t)
    eng.sync()
    st = log.state()
    assert st["writer"] == len(data) and st["epochs"] == list(enumerate(starts))
    return eng, log, data


@pytest.mark.parametrize("async_slice", [False, True])
@pytest.mark.parametrize("seg", [64, S.BIG_SEG])
def test_gather_packed_every_alignment(seg, async_slice):
    """All (t, L) in one batch, each request on its own channel, at every output base residue."""
    reqs = S.short_requests()
    lens = [L for _, L in reqs]
    offs = [S.EPOCH_LENS[t] - L for t, L in reqs]
    total = sum(lens)
    eng, log, data = short_engine(seg, async_slice=async_slice)
    buf = DeviceBuf(S.buffer_size(total, LEAD))
    try:
        parts = S.short_parts(data, reqs)
        req = slice_reqs([log.handle] * len(reqs), [t for t, _ in reqs])
        for d in range(16):
            buf.fill(S.FILL)
            seek(eng, req, offs)
            res, got = slice_device(eng, req, buf.at(LEAD + d), total)
            assert got == total
            check_res(res, lens, offs)
            assert_same(buf.host(), S.packed(parts, d, LEAD), f"seg {seg}, base residue {d}")
    finally:
        buf.free()
        eng.close()


@pytest.mark.parametrize("seg", [64, S.BIG_SEG])
def test_gather_isolated_every_alignment(seg):
    """One request per call into its own slot of a buffer filled once and read back once: no
    neighbouring range can repair a spill over a range's edge."""
    cases = S.isolated_cases()
    eng, log, data = short_engine(seg)
    buf = DeviceBuf(len(cases) * S.ISO_SLOT + S.SLACK, S.FILL)
    try:
        req = slice_reqs([log.handle], [0])
        for k, (t, d, L) in enumerate(cases):
            req["epoch"] = t
            seek(eng, req, [S.EPOCH_LENS[t] - L])
            res, got = slice_device(eng, req, buf.at(k * S.ISO_SLOT + d), L)
            assert got == L and res["len"][0] == L and res["out_off"][0] == 0 and res["status"][0] == 0, (t, d, L)
        assert_same(buf.host(), S.isolated_expect(data, cases), f"seg {seg}")
    finally:
        buf.free()
        eng.close()


def test_gather_piece_counts():
    """Launches of exactly n blocks, n in 1..25, and of 16 + r blocks from three requests: the
    block-to-piece remap serves every piece once, whatever the count's remainder mod 8."""
    seg, data = S.COUNT_SEG, S.count_log()
    batches = S.count_batches()
    buf = DeviceBuf(S.buffer_size(max(sum(b) for b in batches) * seg, LEAD))
    with Engine(segment_bytes=seg, pool_segments=64, ifl_pool_segments=16) as eng:
        try:
            log = eng.open_log(CausalLogID.main(1))
            log.appendDeterminant(data, 0)
            eng.sync()
            assert log.state()["epochs"] == [(0, 0)] and log.state()["n_components"] == S.COUNT_N
            for batch in batches:
                d = S.count_pieces(batch) % 16
                offs = [seg * (S.COUNT_N - n) for n in batch]
                lens = [seg * n for n in batch]
                req = slice_reqs([log.handle] * len(batch), [0] * len(batch))
                buf.fill(S.FILL)
                seek(eng, req, offs)
                res, got = slice_device(eng, req, buf.at(LEAD + d), sum(lens))
                assert got == sum(lens)
                check_res(res, lens, offs)
                want = S.packed([data[o:] for o in offs], d, LEAD)
                assert_same(buf.host(), want + bytes([S.FILL]) * (buf.n - len(want)),
                            f"{batch}: {S.count_pieces(batch)} pieces")
        finally:
            buf.free()


@pytest.mark.parametrize("seg", [64, S.BIG_SEG])
def test_gather_host_planned_pieces(seg):
    """clg_get_determinants into device memory (pieces planned on the host, add_pieces): start
    residues 0, 1, 15, lengths 1, 17, 65, every output residue, a slot per call."""
    cases = [(r, L, d) for r, L in S.PLAN_CASES for d in range(16)]
    buf = DeviceBuf(len(cases) * S.ISO_SLOT + S.SLACK, S.FILL)
    want = np.full(buf.n, S.FILL, np.uint8)
    with Engine(segment_bytes=seg, pool_segments=64, ifl_pool_segments=16) as eng:
        try:
            logs = {}
            for i, (r, L) in enumerate(S.PLAN_CASES):
                log = eng.open_log(CausalLogID.main(i))
                body = S.data(r + L, 100 + i)
                if r:
                    log.appendDeterminant(body[:r], 0)
                log.appendDeterminant(body[r:], 1)
                logs[r, L] = (log, body)
            eng.sync()
            for k, (r, L, d) in enumerate(cases):
                log, body = logs[r, L]
                assert log.state()["epochs"][-1] == (1, r) and log.state()["writer"] == r + L
                assert log.determinants_into(1, buf.at(k * S.ISO_SLOT + d), L) == L
                want[k * S.ISO_SLOT + d:k * S.ISO_SLOT + d + L] = np.frombuffer(body[r:], np.uint8)
            eng.sync()
            assert_same(buf.host(), want, f"seg {seg}")
        finally:
            buf.free()


# ---- 2. loop-trip edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("async_slice", [False, True])
def test_gather_trip_edges(async_slice):
    """Pieces of 1024 and of 1025 destination chunks: copy_range's second trip."""
    seg, data = S.BIG_SEG, S.data(S.TRIP_LOG, 21)
    lens = [S.TRIP_LOG - o for o in S.TRIP_OFFSETS]
    buf = DeviceBuf(S.buffer_size(sum(lens), LEAD))
    with Engine(segment_bytes=seg, pool_segments=64, ifl_pool_segments=16, async_slice=async_slice) as eng:
        try:
            log = eng.open_log(CausalLogID.main(1))
            log.appendDeterminant(data, 0)
            eng.sync()
            assert log.state()["epochs"] == [(0, 0)] and log.state()["writer"] == S.TRIP_LOG
            req = slice_reqs([log.handle] * len(lens), [0] * len(lens))
            seen = set()
            for d in S.TRIP_BASES:
                buf.fill(S.FILL)
                seek(eng, req, S.TRIP_OFFSETS)
                res, got = slice_device(eng, req, buf.at(LEAD + d), sum(lens))
                assert got == sum(lens)
                check_res(res, lens, S.TRIP_OFFSETS)
                for o, r in zip(S.TRIP_OFFSETS, res):  # chunk counts from what the engine reports
                    seen |= {(n, S.chunks(dst, n)) for _, dst, n in S.pieces(o, int(r["len"]), seg, d + int(r["out_off"]))}
                assert_same(buf.host(), S.packed([data[o:] for o in S.TRIP_OFFSETS], d, LEAD), f"base residue {d}")
            assert {(16384, 1024), (16384, 1025), (16383, 1024), (16383, 1025), (16369, 1024)} <= seen
        finally:
            buf.free()


def scatter_round_trip(eng, cases, seg, what):
    """A log per (w, s, L): every lead (w bytes, epoch 0) in one device-input batch, every body
    (L bytes at source residue s, epoch 1) in a second one; then every log read from HBM."""
    logs = [eng.open_log(CausalLogID.main(i)) for i in range(len(cases))]
    handles = [l.handle for l in logs]
    leads = [S.data(w, 5000 + i) for i, (w, _, _) in enumerate(cases)]
    bodies = [S.data(L, 9000 + i) for i, (_, _, L) in enumerate(cases)]
    lpos, lsize = S.place([(w, (7 * i) % 16) for i, (w, _, _) in enumerate(cases)])
    bpos, bsize = S.place([(L, s) for _, s, L in cases])
    d = upload(S.source_buffer(leads, lpos, lsize))
    upstream_device(eng, handles, 0, lpos, [w for w, _, _ in cases], d)
    d = upload(S.source_buffer(bodies, bpos, bsize))
    upstream_device(eng, handles, 1, bpos, [L for _, _, L in cases], d)
    for i, (w, s, L) in enumerate(cases):
        st = logs[i].state()
        assert st["writer"] == w + L and st["epochs"] == ([(0, 0)] if w else []) + [(1, w)], (w, s, L)
        assert st["n_components"] == (w + L + seg - 1) // seg
        assert_same(logs[i].read_phys(0, w + L), leads[i] + bodies[i], f"{what} w {w} s {s} L {L}")


def test_scatter_trip_edges():
    """Scatter chunks either side of one, two and four trips of a wave (256 chunks each), device
    input at source residues 0, 1, 15 onto writer residues 0, 1, 15."""
    cases = S.trip_scatter_cases()
    with Engine(segment_bytes=S.BIG_SEG, pool_segments=512, ifl_pool_segments=16) as eng:
        scatter_round_trip(eng, cases, S.BIG_SEG, "trip")


# ---- 3. scatter, short ranges, every alignment -----------------------------------------------------
def test_scatter_every_alignment():
    """Every (writer residue, source residue, L) at 64-byte segments.  A body that ends on its
    segment's last byte, or starts on a segment's first, would spill into another log's segment,
    which the final comparison reads.  (A spill past the writer inside the log's own segment is
    not observable and harmless: the next append overwrites it.)"""
    cases = S.scatter_cases()
    assert any(S.ends_on_segment_end(w, L) for w, _, L in cases)
    assert any(S.starts_on_segment_start(w, L) for w, _, L in cases)
    with Engine(segment_bytes=S.SCATTER_SEG, pool_segments=8192, ifl_pool_segments=16) as eng:
        scatter_round_trip(eng, cases, S.SCATTER_SEG, "short")


def test_scatter_host_staged():
    """Appends staged on the host (no host tail kept) and flushed by one scatter from packed
    staging offsets: all 16 relative shifts between staging offset and writer."""
    cases = S.staged_cases()
    assert set(S.staged_shifts(cases)) == set(range(16))
    with Engine(segment_bytes=S.SCATTER_SEG, pool_segments=2048, ifl_pool_segments=16, host_tail_bytes=0) as eng:
        logs = [eng.open_log(CausalLogID.main(i)) for i in range(len(cases))]
        h = np.array([l.handle for l in logs], np.uint32)
        for col, seed in ((0, 300), (1, 301)):  # the leads, flushed; then the bodies in one batch
            lens = np.array([c[col] for c in cases], np.uint32)
            blob = np.frombuffer(S.data(int(lens.sum()), seed), np.uint8)
            offs = (np.cumsum(lens) - lens).astype(np.uint64)
            keep = lens > 0
            eng.append_batch(h[keep], np.zeros(int(keep.sum()), np.int64), offs[keep], lens[keep], blob)
            eng.sync()
            if col == 0:
                lead, lead_offs = blob.tobytes(), offs
        body = blob.tobytes()
        for i, (w, L) in enumerate(cases):
            assert logs[i].state()["writer"] == w + L
            want = lead[int(lead_offs[i]):int(lead_offs[i]) + w] + body[int(offs[i]):int(offs[i]) + L]
            assert_same(logs[i].read_phys(0, w + L), want, f"log {i} w {w} L {L}")


# ---- 4. in-flight pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [64, S.BIG_SEG])
def test_inflight_every_alignment(seg):
    """clg_ifl_log_batch from device memory at every source residue, replayed into device memory
    at four base residues: the bytes, the sizes and the sentinels around them."""
    cases = S.ifl_cases(seg)
    bodies = [S.data(L, 700 + i) for i, (L, _) in enumerate(cases)]
    lens = np.array([L for L, _ in cases], np.uint32)
    total = int(lens.sum())
    pos, size = S.place(cases)
    need = sum((L + seg - 1) // seg for L, _ in cases)
    buf = DeviceBuf(S.buffer_size(total, LEAD))
    with Engine(segment_bytes=64, pool_segments=16, ifl_segment_bytes=seg, ifl_pool_segments=need + 8) as eng:
        try:
            f = inflight.InFlightLog(eng)
            d = upload(S.source_buffer(bodies, pos, size))
            h = np.full(len(cases), f.handle, np.uint32)
            ep = np.zeros(len(cases), np.int64)
            offs = np.array(pos, np.uint64)
            check(lib.clg_ifl_log_batch(eng.handle, h.ctypes.data, ep.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                        len(cases), d.data_ptr(), _lib.CLG_MEM_DEVICE))
            assert f.epochs() == [(0, len(cases))] and eng.ifl_pool_stats()[0] == need
            for b in S.IFL_BASES:
                buf.fill(S.FILL)
                sizes = np.zeros(len(cases), np.uint32)
                st, res, _, _, got, nbuf = inflight.replay_batch_raw(eng, [(f, 0, 0)], out=buf.at(LEAD + b), sizes=sizes,
                                                                     cap=total)
                eng.sync()
                assert st == 0 and res[0].status == 0 and got == total == res[0].len and res[0].out_off == 0
                assert nbuf == len(cases) == res[0].n_buffers and (sizes == lens).all()
                assert_same(buf.host(), S.packed(bodies, b, LEAD), f"ifl seg {seg}, base residue {b}")
        finally:
            buf.free()
