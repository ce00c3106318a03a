"""Developer probe: typed replay columns over config 2's logs (64 logs x 1 M records in 16 KiB
segments), in one process and alternating, 10 repeats after 3 warm-up rounds, each figure as
median (min - max):

  (a) soa_decode_device     clg_decode_logs into device SoA (HIP events: decode_pipeline; its
                            emit pass alone: decode_emit)
  (b) columns_kernels       clg_columnize of that device SoA into device columns: the
                            decode_columns kernels alone (HIP events)
  (c) soa_to_host           clg_decode_logs delivered to registered host memory, against
      columns_to_host       clg_decode_logs_columns delivered to registered host memory: the
                            host clock around calls that end in a synchronise, and the bytes
                            each delivers

and, when PROBE_PARENT_LIB names the parent commit's library (tools/ab_build.sh), the decode time
of tools/c2_decode_probe.py for this tree and for the parent, each in a fresh process on the
same box.  Writes profiles/columns_probe.json and prints it."""
import ctypes as C
import json
import mmap
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 10, 3
n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 64)), int(os.environ.get("PROBE_REC", 1_000_000))


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def c2_decode(lib_path):
    """tools/c2_decode_probe.py in a fresh process (before this one opens the GPU)."""
    env = dict(os.environ)
    if lib_path:
        env["CLONOS_LIB"] = lib_path
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "c2_decode_probe.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    return json.loads(r.stdout.strip().splitlines()[-1])


res = {"reps": REPS, "warmup_rounds": WARM}
parent = os.environ.get("PROBE_PARENT_LIB")
if parent:
    ab = {"tree": [], "parent": []}
    for _ in range(2):  # alternating
        ab["tree"].append(c2_decode(None))
        ab["parent"].append(c2_decode(os.path.abspath(parent)))
    res["c2_decode_probe_ms"] = {
        side: {k: [r[k] for r in runs] for k in ("decode_pipeline", "decode_count", "decode_emit") if k in runs[0]}
        for side, runs in ab.items()}
else:
    res["c2_decode_probe_ms"] = "not measured (PROBE_PARENT_LIB not set)"

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402

rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
pool = sum(int(b.size) // seg + 2 for b in bufs) + 64
total = sum(int(b.size) for b in bufs)
n = n_logs * n_rec


def registered(nbytes):
    buf = np.frombuffer(mmap.mmap(-1, (nbytes + 4095) & ~4095), np.uint8)
    buf[:] = 0  # fault the pages in before they are pinned
    _lib.check(_lib.lib.clg_host_register(buf.ctypes.data, buf.size))
    return buf


def carve(buf, sizes):
    at, out = 0, []
    for s in sizes:
        out.append(buf.ctypes.data + at)
        at = (at + s + 255) & ~255
    return out, at


with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    h = np.array([lg.handle for lg in logs], np.uint32)
    ep = np.ones(n_logs, np.int64)
    base = np.zeros(n_logs + 1, np.uint64)

    # device SoA, and device columns of exactly the batch's sizes
    o = [torch.empty(n, dtype=t, device="cuda") for t in (torch.int32, torch.uint8, torch.int64)]
    w = [torch.empty(1024, dtype=t, device="cuda") for t in
         (torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.uint8)]
    d = _lib.Decoded()
    d.off, d.tag, d.v0 = [x.data_ptr() for x in o]
    d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [x.data_ptr() for x in w]
    d.cap, d.wcap, d.out_kind = n, 1024, _lib.CLG_MEM_DEVICE
    eng.decode_logs_device(h, ep, d, base)
    sizes = _lib.Columns()
    eng.columnize(d, base, sizes)  # sizes only
    n_class = [int(x) for x in sizes.n_class]
    assert int(sizes.n_rec) == n and n_class[4] == 0
    dcol = [torch.empty(max(k, 1), dtype=t, device="cuda") for k, t in
            ((n, torch.uint8), (n_class[0], torch.int8), (n_class[1], torch.int64), (n_class[2], torch.int32),
             (n_class[3], torch.int32))]
    sb_dev = np.zeros((n_logs + 1) * 5, np.uint64)

    def columns_struct(ptrs, kind, sb):
        c = _lib.Columns()
        c.tag, c.order, c.timestamp, c.rng, c.buffer_built = ptrs
        c.cap_tag, c.cap_order, c.cap_timestamp, c.cap_rng, c.cap_buffer_built = n, *n_class[:4]
        c.span_base, c.out_kind = sb.ctypes.data, kind
        return c

    cdev = columns_struct([x.data_ptr() for x in dcol], _lib.CLG_MEM_DEVICE, sb_dev)

    # registered host memory for the SoA rows and for the columns
    soa_sizes = [4 * n, n, 8 * n, 4096, 4096, 8192, 4096, 4096, 1024]
    hsoa = registered(carve(np.zeros(1, np.uint8), soa_sizes)[1] + 4096)
    sp, _ = carve(hsoa, soa_sizes)
    dh = _lib.Decoded()
    dh.off, dh.tag, dh.v0, dh.w_idx, dh.w_rc, dh.w_v1, dh.w_var_off, dh.w_var_len, dh.w_sub = sp
    dh.cap, dh.wcap, dh.out_kind = n, 1024, _lib.CLG_MEM_MAPPED
    col_sizes = [n, n_class[0], 8 * n_class[1], 4 * max(n_class[2], 1), 4 * max(n_class[3], 1)]
    hcol = registered(carve(np.zeros(1, np.uint8), col_sizes)[1] + 4096)
    cp, _ = carve(hcol, col_sizes)
    sb_host = np.zeros((n_logs + 1) * 5, np.uint64)
    chost = columns_struct(cp, _lib.CLG_MEM_MAPPED, sb_host)
    base_h = np.zeros(n_logs + 1, np.uint64)

    ms = {k: [] for k in ("soa_decode_device", "soa_decode_emit", "columns_kernels", "soa_to_host", "columns_to_host")}

    def stat_ms(*names):
        st = eng.kernel_stats()
        return [st[k]["ms"] if k in st else float("nan") for k in names]

    for k in range(WARM + REPS):
        if k == WARM:
            ms = {name: [] for name in ms}
        eng.sync()
        eng.kernel_stats_reset()
        eng.decode_logs_device(h, ep, d, base)                       # (a)
        eng.sync()
        a, emit = stat_ms("decode_pipeline", "decode_emit")
        ms["soa_decode_device"].append(a)
        ms["soa_decode_emit"].append(emit)
        eng.kernel_stats_reset()
        eng.columnize(d, base, cdev)                                 # (b)
        ms["columns_kernels"].append(stat_ms("decode_columns")[0])
        t0 = time.perf_counter()                                     # (c)
        _lib.check(_lib.lib.clg_decode_logs(eng.handle, h.ctypes.data, ep.ctypes.data, n_logs, dh, base_h.ctypes.data))
        t1 = time.perf_counter()
        assert eng.decode_logs_columns_raw(h, ep, chost) == 0
        t2 = time.perf_counter()
        ms["soa_to_host"].append((t1 - t0) * 1e3)
        ms["columns_to_host"].append((t2 - t1) * 1e3)

    # the two deliveries hold the same records
    tag_soa = np.frombuffer(C.string_at(sp[1], n), np.uint8)
    tag_col = np.frombuffer(C.string_at(cp[0], n), np.uint8)
    assert (tag_soa == tag_col).all() and (sb_host == sb_dev).all() and int(sb_host[-5:].sum()) == n
    v0 = np.frombuffer(C.string_at(sp[2], 8 * n), np.int64)
    assert (np.frombuffer(C.string_at(cp[2], 8 * n_class[1]), np.int64) == v0[tag_soa == 1]).all()
    assert (np.frombuffer(C.string_at(cp[1], n_class[0]), np.int8) == v0[tag_soa == 0]).all()

    soa_bytes = 13 * n
    col_bytes = n + n_class[0] + 8 * n_class[1] + 4 * n_class[2] + 4 * n_class[3]
    res.update({
        "workload": f"config 2: {n_logs} logs x {n_rec} records, {total} bytes in {seg}-byte segments",
        "records": n, "class_totals": n_class,
        "a_soa_decode_device_ms": spread(ms["soa_decode_device"]),
        "a_soa_decode_emit_ms": spread(ms["soa_decode_emit"]),
        "b_columns_kernels_ms": spread(ms["columns_kernels"]),
        "b_columns_over_emit": round(float(np.median(ms["columns_kernels"]) / np.median(ms["soa_decode_emit"])), 3),
        "c_soa_to_host_ms": spread(ms["soa_to_host"]),
        "c_columns_to_host_ms": spread(ms["columns_to_host"]),
        "c_soa_bytes_delivered": soa_bytes, "c_columns_bytes_delivered": col_bytes,
        "c_bytes_ratio": round(soa_bytes / col_bytes, 3),
        "c_wall_ratio": round(float(np.median(ms["soa_to_host"]) / np.median(ms["columns_to_host"])), 3),
        "note": ("(a), (b): HIP-event time of all kernels of a call under one stat; (c): host clock around "
                 "synchronous calls into host memory registered with clg_host_register."),
    })
    _lib.lib.clg_host_unregister(hsoa.ctypes.data)
    _lib.lib.clg_host_unregister(hcol.ctypes.data)

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "columns_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
