"""Developer probe: the packed payload column, on the payload columns of config 1's
epoch (every log of synth.config1_job), of config 3 (PROBE_C3_LOGS logs of one PROBE_C3_REC-record
epoch) and of config 5's shape (16 main logs of ~45 KB of config 3's mix).

  bytes   n_var against desc + bits + tail, from the CPU codec (pack_payloads_host).  With --cpu the
          columns come from the test oracle's decode and nothing else is measured: no GPU is needed.
  time    (without --cpu) clg_pack_payloads and clg_unpack_payloads, device in and device out, beside
          clg_gather_payloads of the same column from one device buffer into device memory (the plain
          copy of the same bytes), in one process and alternating, REPS repeats after WARM warm-up
          rounds, each figure as median (min - max): the host clock around synchronous calls, and the
          kernels' HIP-event time by stat.  The device's packed bytes are held against the CPU codec's
          and the unpacked column against the input.

Writes profiles/ppay_probe.json and prints it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU = "--cpu" in sys.argv
REPS, WARM = int(os.environ.get("PROBE_REPS", 20)), int(os.environ.get("PROBE_WARM", 3))
c3_logs, c3_rec = int(os.environ.get("PROBE_C3_LOGS", 16)), int(os.environ.get("PROBE_C3_REC", 250_000))

if not CPU:
    import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import _lib, pack_payloads_host, synth  # noqa: E402


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def workloads():
    rng = np.random.default_rng(synth.SEED_CONFIG1)
    _, logs = synth.config1_job(rng)
    yield "config 1 epoch: every log of synth.config1_job", [bytes(d) for _, d in sorted(logs.items(), key=lambda x: repr(x[0]))]
    c3 = bytes(synth.config3_epoch(c3_rec, np.random.default_rng(3))[0])
    yield f"config 3: {c3_logs} logs, each one epoch of {c3_rec} records", [c3] * c3_logs
    rng = np.random.default_rng(5)
    per = len(synth.config3_epoch(1000, rng)[0]) / 1000.0
    yield "config 5: 16 main logs of ~45 KB of config 3's mix", [bytes(synth.config3_epoch(int(45_000 / per), rng)[0]) for _ in range(16)]


def column_cpu(spans):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _ppay_util import payload_column_of  # (the oracle: test infrastructure, used for --cpu only)
    return payload_column_of(spans)


def column_gpu(eng, spans):
    data = np.frombuffer(b"".join(spans), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])])
    cols = eng.decode_host_columns(data, [(int(offs[i]), len(s)) for i, s in enumerate(spans)], payloads=True)
    return np.ascontiguousarray(cols.var, np.uint8), np.ascontiguousarray(cols.var_pos, np.uint64)


def sizes(label, var, pos):
    pk = pack_payloads_host(var, pos)
    packed = pk.n_bytes
    return pk, {"workload": label, "rows": int(pos.size - 1), "n_var": int(var.size),
                "packed_bytes": {"desc": int(pk.desc.nbytes), "bits": int(pk.bits.size), "tail": int(pk.tail.size), "total": packed},
                "n_var_over_packed": round(var.size / max(packed, 1), 3)}


def timed(eng, var, pos, want):
    lib = _lib.lib
    n, nv = pos.size - 1, var.size
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    room = lambda k: torch.empty(max(k, 16), dtype=torch.uint8, device="cuda")  # noqa: E731
    d_var, d_pos = dev(var) if nv else room(0), dev(pos)
    d_desc, d_bits, d_tail, d_back = room(want.desc.nbytes), room(want.bits.size), room(want.tail.size), room(nv)
    d_copy, d_cpos = room(nv), room(8 * (n + 1))
    lens = np.diff(pos.astype(np.int64)).astype(np.uint32)
    d_off, d_len = dev(pos[:-1].astype(np.uint32)), dev(lens)
    so, sl, rb = np.zeros(1, np.uint64), np.array([nv], np.uint64), np.array([0, n], np.uint64)

    p = _lib.PackedPayloadsC()
    p.desc, p.bits, p.tail = d_desc.data_ptr(), d_bits.data_ptr(), d_tail.data_ptr()
    p.cap_desc, p.cap_bits, p.cap_tail, p.out_kind = want.desc.size, want.bits.size, want.tail.size, _lib.CLG_MEM_DEVICE
    out = _lib.Payloads()
    out.var, out.cap_var, out.out_kind = d_back.data_ptr(), nv, _lib.CLG_MEM_DEVICE
    cp = _lib.Payloads()
    cp.var, cp.pos, cp.cap_var, cp.cap_pos, cp.out_kind = d_copy.data_ptr(), d_cpos.data_ptr(), nv, n + 1, _lib.CLG_MEM_DEVICE
    bad = _lib.UnpackBad()
    names = ("pack", "unpack", "copy")
    stats = {"pack": ("pack_payloads",), "unpack": ("unpack_payloads",), "copy": ("decode_payloads",)}
    wall, kern = {k: [] for k in names}, {k: [] for k in names}

    def kernel_ms(which):
        ks = eng.kernel_stats()
        return sum(ks[s]["ms"] for s in stats[which] if s in ks)

    for k in range(WARM + REPS):
        if k == WARM:
            wall, kern = {x: [] for x in names}, {x: [] for x in names}
        eng.sync()
        eng.kernel_stats_reset()
        t0 = time.perf_counter()
        st = lib.clg_pack_payloads(eng.handle, d_var.data_ptr(), d_pos.data_ptr(), n, _lib.CLG_MEM_DEVICE, C.byref(p))
        t1 = time.perf_counter()
        _lib.check(st)
        kern["pack"].append(kernel_ms("pack"))
        eng.kernel_stats_reset()
        t2 = time.perf_counter()
        st = lib.clg_unpack_payloads(eng.handle, C.byref(p), d_pos.data_ptr(), _lib.CLG_MEM_DEVICE, C.byref(out), C.byref(bad))
        t3 = time.perf_counter()
        _lib.check(st)
        kern["unpack"].append(kernel_ms("unpack"))
        eng.kernel_stats_reset()
        t4 = time.perf_counter()
        st = lib.clg_gather_payloads(eng.handle, d_var.data_ptr(), so.ctypes.data, sl.ctypes.data, 1, d_off.data_ptr(),
                                     d_len.data_ptr(), rb.ctypes.data, _lib.CLG_MEM_DEVICE, C.byref(cp))
        t5 = time.perf_counter()
        _lib.check(st)
        kern["copy"].append(kernel_ms("copy"))
        wall["pack"].append((t1 - t0) * 1e3), wall["unpack"].append((t3 - t2) * 1e3), wall["copy"].append((t5 - t4) * 1e3)

    # the device's bytes are the CPU codec's, and the way back gives the column
    assert (int(p.n_bits), int(p.n_tail)) == (want.bits.size, want.tail.size)
    assert d_desc[:want.desc.nbytes].cpu().numpy().tobytes() == want.desc.tobytes()
    assert d_bits[:want.bits.size].cpu().numpy().tobytes() == want.bits.tobytes()
    assert d_tail[:want.tail.size].cpu().numpy().tobytes() == want.tail.tobytes()
    assert d_back[:nv].cpu().numpy().tobytes() == var.tobytes() and d_copy[:nv].cpu().numpy().tobytes() == var.tobytes()
    saved = nv - want.n_bytes
    extra_ms = float(np.median(wall["pack"])) + float(np.median(wall["unpack"])) - float(np.median(wall["copy"]))
    return {"wall_ms": {k: spread(v) for k, v in wall.items()}, "kernel_ms": {k: spread(v) for k, v in kern.items()},
            "bytes_saved": int(saved), "pack_plus_unpack_minus_copy_wall_ms": round(extra_ms, 4),
            # below this link bandwidth the saved bytes take longer to send than the pack and the unpack add
            "break_even_link_GB_per_s": round(saved / (extra_ms * 1e-3) / 1e9, 3) if saved > 0 and extra_ms > 0 else None}


res = {"reps": REPS, "warmup_rounds": WARM, "workloads": [],
       "note": ("bytes: the CPU codec's.  wall: host clock around synchronous calls, device in and device out, the three calls "
                "alternating in one process; kernel ms: HIP-event time of all kernels of the call under its stat; copy: "
                "clg_gather_payloads of the same rows from one device buffer.  break_even_link_GB_per_s: the saved bytes over "
                "the wall time pack and unpack add to the copy." if not CPU else
                "bytes only (--cpu): the columns from the test oracle's decode, the sizes from the CPU codec; no time was measured.")}
if CPU:
    for label, spans in workloads():
        _, row = sizes(label, *column_cpu(spans))
        res["workloads"].append(row)
else:
    from clonos_amd import Engine
    with Engine(segment_bytes=16384, pool_segments=1024, timing=True) as eng:
        for label, spans in workloads():
            var, pos = column_gpu(eng, spans)
            want, row = sizes(label, var, pos)
            row.update(timed(eng, var, pos, want))
            res["workloads"].append(row)

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "ppay_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
