"""GPU, world_size 2 (gloo transport, both ranks on cuda:0): Replicator.locate over real
engines -- the replicas that verify flags compared with their owners' copies on the device, and
the divergence named by byte, epoch and record (tests/gpu_dist_locate_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_locate_engines_world2():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_dist_locate_worker.py")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "replicas located: [(0, 0), (1, 2)]" in r.stdout
