"""GPU: a Serializable batch on the three passes, compared with the oracle.

The last case of the removed one-pass decode's tests ("One pass"), under
the id it has always had; the others are the test_fused_* cases at the end of
test_gpu_fused.py, whose engine factory it shares.
"""
import numpy as np
import pytest

from clonos_amd import synth
from test_gpu_decode import assert_span_equal
from test_gpu_fused import three_pass  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_one_pass_serializable_goes_to_tables(three_pass):  # noqa: F811
    eng = three_pass()
    rng = np.random.default_rng(7)
    buf = synth.config3_epoch(30_000, rng)[0].tobytes()
    dec = eng.decode_host(buf)
    assert_span_equal(dec, 0, buf)
