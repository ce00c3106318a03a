"""CPU: bench.py's options and its --dump-outputs writer (no GPU: the writer is handed host
tensors).  A plain run has every secondary leg off (--full turns them on), and a dump is
float32 / float64 only, the same from call to call, whole below the sample sizes and a fixed
sample above them."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _args(monkeypatch, "--full", "--dump-outputs", "d", "--no-config3")
    assert a.full is True and a.dump_outputs == "d" and a.no_config3


def _dump(path, n_rec, n_slice, n_wide=0):
    import torch
    dec = types.SimpleNamespace(n_rec=n_rec, n_wide=n_wide, err_status=0)
    cap = n_rec + 5  # (outputs are allocated past what a decode fills)
    tens = [torch.arange(cap, dtype=torch.int32), (torch.arange(cap) % 7).to(torch.uint8),
            torch.arange(cap, dtype=torch.int64) + 1_700_000_000_000]
    tens += [torch.arange(8).to(t) for t in (torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.uint8)]
    o_slice = (torch.arange(n_slice + 64) % 251).to(torch.uint8)
    cres = [types.SimpleNamespace(status=0, has_delta=1, offset_from_epoch=3 * k, len=10 * k, out_off=100 * k)
            for k in range(4)]
    bench.dump_outputs(str(path), torch, dec, np.arange(3, dtype=np.uint64), tens, o_slice, n_slice, cres, 4)
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_small_is_whole(tmp_path):
    d = _dump(tmp_path / "a", 1000, 5000, n_wide=2)
    assert set(d) == {"decode_off", "decode_tag", "decode_v0", "decode_base", "decode_counts", "slice_bytes",
                      "slice_res", "decode_w_idx", "decode_w_rc", "decode_w_v1", "decode_w_var_off",
                      "decode_w_var_len", "decode_w_sub"}
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert (d["decode_off"] == np.arange(1000)).all() and (d["decode_tag"] == np.arange(1000) % 7).all()
    assert (d["decode_v0"] == np.arange(1000) + 1_700_000_000_000).all()  # exact in float64
    assert (d["slice_bytes"] == np.arange(5000) % 251).all()
    assert d["decode_counts"].tolist() == [1000, 2, 0] and d["decode_w_v1"].tolist() == [0, 1]
    assert d["slice_res"].shape == (4, 5) and d["slice_res"][3].tolist() == [0, 1, 9, 30, 300]


def test_dump_large_is_a_fixed_sample(tmp_path):
    n_rec, n_slice = bench.DUMP_RECORDS + 12345, bench.DUMP_SLICE_BYTES + 777
    a, b = _dump(tmp_path / "a", n_rec, n_slice), _dump(tmp_path / "b", n_rec, n_slice)
    assert "decode_w_idx" not in a  # no wide records: no side arrays
    assert set(a) == set(b) and all((a[k] == b[k]).all() for k in a)
    off = a["decode_off"].astype(np.int64)  # (the fake decode's offset is the record's index)
    assert 0 < len(off) <= bench.DUMP_RECORDS and (np.diff(off) > 0).all() and off[-1] < n_rec
    assert (a["decode_tag"] == off % 7).all() and (a["decode_v0"] == off + 1_700_000_000_000).all()
    assert 0 < len(a["slice_bytes"]) <= bench.DUMP_SLICE_BYTES
    # at the real shape every array is sampled: that total stays under 64 MB
    assert bench.DUMP_RECORDS * (8 + 4 + 8) + bench.DUMP_SLICE_BYTES * 4 < 60e6
