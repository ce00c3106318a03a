"""GPU, world_size 2 (gloo transport, both ranks on cuda:0): Replicator.verify(prefixes=True),
only_diverged() into locate, first_bad_epoch and merge_responses(verify="prefixes") over real
engines -- lagging replicas told from diverged ones by the device-side prefix digests
(tests/gpu_dist_prefix_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_prefix_protocols_engines_world2():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_dist_prefix_worker.py")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # (diverged replicas, merged logs delivered) per rank: none diverged on rank 0, three on rank 1
    assert "replicas sorted by prefix digests: [(0, " in r.stdout and "(3, " in r.stdout
