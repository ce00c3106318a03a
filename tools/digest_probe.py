"""Developer probe: the log digest over config 2's logs (64 logs x 1 M records in 16 KiB
segments), beside the gather of the same ranges into device memory (clg_get_determinants_batch,
which reads the same bytes and also writes them), both timed by the engine's HIP events in one
process.  Writes profiles/digest_probe.json and prints it."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, digest_host, synth  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (MI355X specification)
REPS = 10

n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 64)), int(os.environ.get("PROBE_REC", 1_000_000))
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
pool = sum(int(b.size) // seg + 2 for b in bufs) + 64
total = sum(int(b.size) for b in bufs)
with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    h = np.array([lg.handle for lg in logs], np.uint32)
    ep = np.ones(n_logs, np.int64)
    out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    ln = np.zeros(n_logs, np.uint32)
    tot = C.c_uint64()

    def gather():
        _lib.check(_lib.lib.clg_get_determinants_batch(eng.handle, h.ctypes.data, ep.ctypes.data, n_logs, out.data_ptr(),
                                                       out.numel(), _lib.CLG_MEM_DEVICE, None, ln.ctypes.data,
                                                       C.byref(tot)))

    for k in range(3 + REPS):  # alternating, so neither kernel finds the other's bytes any warmer
        if k == 3:
            eng.sync()
            eng.kernel_stats_reset()
        dg = eng.digest_logs(h, ep)
        gather()
    eng.sync()
    st = eng.kernel_stats()
    assert tot.value == total and int(dg["len"].sum()) == total
    assert (int(dg["hash"][0]), int(dg["len"][0])) == digest_host(bufs[0])  # (one log against the CPU)
    d, g = st["log_digest"], st["slice_gather"]
    d_ms, g_ms = d["ms"] / d["launches"], g["ms"] / g["launches"]
    res = {
        "workload": f"config 2: {n_logs} logs x {n_rec} records, {total} bytes in {seg}-byte segments",
        "reps": REPS,
        "log_digest_ms": round(d_ms, 4),
        "log_digest_bytes_read": d["bytes"] // d["launches"],
        "log_digest_tb_per_s": round(total / d_ms / 1e9, 3),
        "log_digest_fraction_of_hbm_peak": round(total / (d_ms * 1e-3) / HBM_PEAK, 3),
        "slice_gather_ms": round(g_ms, 4),
        "slice_gather_bytes_read_and_written": g["bytes"] // g["launches"],
        "digest_over_gather": round(d_ms / g_ms, 3),
        "note": "HIP-event time of both digest kernels under one stat; the gather reads the same bytes and writes "
                "them to device memory.  8.0 TB/s is the specified HBM peak.",
    }
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "digest_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
