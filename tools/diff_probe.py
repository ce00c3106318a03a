"""Developer probe: the log comparison over config 2's logs (64 logs x 1 M records in 16 KiB
segments) against a device copy of the same ranges (made with clg_get_determinants_batch), beside
the log digest and the gather of those ranges into device memory.  The inputs are equal, so no
piece stops early.  All three are timed by the engine's HIP events, alternating in one process
after a warm-up, one figure per repeat.  Writes profiles/diff_probe.json and prints it."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, lcp_host, synth  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (MI355X specification)
WARMUP, REPS = 3, 10

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
    ref = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    ln = np.zeros(n_logs, np.uint32)
    off = np.zeros(n_logs, np.uint64)
    tot = C.c_uint64()

    def gather(dst):
        _lib.check(_lib.lib.clg_get_determinants_batch(eng.handle, h.ctypes.data, ep.ctypes.data, n_logs, dst.data_ptr(),
                                                       dst.numel(), _lib.CLG_MEM_DEVICE, off.ctypes.data, ln.ctypes.data,
                                                       C.byref(tot)))

    gather(ref)  # the reference: a device copy of the same ranges, packed back to back
    eng.sync()
    offs, lens = off.copy(), ln.astype(np.uint64)
    assert tot.value == total

    ms = {"log_diff": [], "log_digest": [], "slice_gather": []}
    for k in range(WARMUP + REPS):  # alternating, so no kernel finds the others' bytes any warmer
        eng.sync()
        eng.kernel_stats_reset()
        df = eng.diff_logs(h, ep, ref.data_ptr(), offs, lens, device=True)
        eng.digest_logs(h, ep)
        gather(out)
        eng.sync()
        st = eng.kernel_stats()
        if k >= WARMUP:
            for name in ms:
                assert st[name]["launches"] == 1
                ms[name].append(st[name]["ms"])
    assert (df["lcp"] == lens).all() and (df["len_log"] == lens).all() and (df["len_ref"] == lens).all()
    assert st["log_diff"]["bytes"] == 2 * total
    # one divergent reference against the CPU: a byte flipped three quarters into the last log
    at = int(offs[-1]) + 3 * int(lens[-1]) // 4
    ref[at] ^= 0x20
    bad = eng.diff_logs(h[-1:], ep[-1:], ref.data_ptr(), offs[-1:], lens[-1:], device=True)
    host = bufs[-1].copy()
    host[at - int(offs[-1])] ^= 0x20
    assert int(bad["lcp"][0]) == lcp_host(bufs[-1], host) == at - int(offs[-1])

    def stat(v):
        return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "max_ms": round(float(np.max(v)), 4)}

    d, g, c = (float(np.median(ms[n])) for n in ("log_digest", "slice_gather", "log_diff"))
    res = {
        "workload": f"config 2: {n_logs} logs x {n_rec} records, {total} bytes in {seg}-byte segments, against an "
                    "equal device copy of the same ranges",
        "warmup": WARMUP,
        "reps": REPS,
        "log_diff": stat(ms["log_diff"]),
        "log_digest": stat(ms["log_digest"]),
        "slice_gather": stat(ms["slice_gather"]),
        "log_diff_bytes_read": 2 * total,
        "log_diff_tb_per_s": round(2 * total / c / 1e9, 3),
        "log_diff_fraction_of_hbm_peak": round(2 * total / (c * 1e-3) / HBM_PEAK, 3),
        "slice_gather_bytes_read_and_written": 2 * total,
        "slice_gather_tb_per_s": round(2 * total / g / 1e9, 3),
        "log_digest_bytes_read": total,
        "diff_over_gather": round(c / g, 3),
        "diff_over_digest": round(c / d, 3),
        "note": "HIP-event time per call, the median of the repeats with their extremes; log_diff and log_digest "
                "each cover both of their kernels.  The comparison reads the log's bytes and as many reference "
                "bytes; the gather reads the log's bytes and writes as many.  8.0 TB/s is the specified HBM peak.",
    }
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "diff_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
