"""GPU, world_size 2 (gloo transport, both ranks on cuda:0): Replicator.verify and
merge_responses(verify=True) over real engines -- replicas and merged winners compared with
their owners' logs by the device-side digest (tests/gpu_dist_verify_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_verify_engines_world2():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_dist_verify_worker.py")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "replicas checked by digest:" in r.stdout
