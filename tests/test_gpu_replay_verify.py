"""GPU: clonos_amd.replay.verify_replay -- the regenerated main log against the recovered copy
by content (device-side digests), where LogReplayerImpl.checkFinished
(LogReplayerImpl.java:126-128) compares lengths only.

The reference digest is the definition restated with Python integers: p = 2^61 - 1,
R = 2654435761, little-endian u32 words zero-padded past the end, h = (h * R + w) mod p.
"""
import numpy as np
import pytest

from clonos_amd import CausalLogID, Engine
from clonos_amd import determinants as D
from clonos_amd import synth
from clonos_amd.replay import verify_replay

pytestmark = pytest.mark.gpu

P = (1 << 61) - 1
R = 2654435761


def ref_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


@pytest.fixture(scope="module")
def recovered():
    """Three epochs of encoded determinants, as a recovered response would carry them."""
    rng = np.random.default_rng(71)
    return [[D.encode(synth.random_determinant(rng)) for _ in range(120)] for _ in range(3)]


def test_reappended_log_matches_and_swap_does_not(recovered):
    whole = b"".join(b"".join(e) for e in recovered)
    with Engine(segment_bytes=256, pool_segments=2048) as eng:
        src = eng.open_log(CausalLogID.main(1))
        for ep, recs in enumerate(recovered):
            src.appendDeterminant(b"".join(recs), ep)
        # the replay: decode the recovered log and re-append its own records
        dec = eng.decode_logs([src], [0], keep_bytes=True)
        dets = dec.determinants(0)
        assert len(dets) == 360
        regen = eng.open_log(CausalLogID.main(2))
        for i, d in enumerate(dets):
            regen.appendDeterminant(d, i // 120)
        (ok,) = verify_replay(eng, [(regen.handle, 0, whole)])
        assert ok.matches and ok.regenerated == ok.recovered == ref_digest(whole)
        # a replay that diverged: two records of one length swapped in epoch 1 -- the same
        # number of bytes, so the reference's length assertion passes
        enc = [D.encode(d) for d in dets]
        i = next(k for k in range(120, 239) if len(enc[k]) == len(enc[k + 1]) and enc[k] != enc[k + 1])
        enc[i], enc[i + 1] = enc[i + 1], enc[i]
        div = eng.open_log(CausalLogID.main(3))
        for ep in range(3):
            div.appendDeterminant(b"".join(enc[120 * ep:120 * ep + 120]), ep)
        (bad,) = verify_replay(eng, [(div.handle, 0, whole)])
        assert not bad.matches and bad.regenerated[1] == bad.recovered[1] == len(whole)
        assert bad.regenerated == ref_digest(b"".join(enc)) and bad.recovered == ref_digest(whole)
        # the suffixes from each epoch, in one batch, localise the divergence: epoch 2's suffix
        # matches, epochs 1 and 0 do not -> it diverged in epoch 1
        starts = np.cumsum([0] + [len(b"".join(e)) for e in recovered])
        res = verify_replay(eng, [(div.handle, ep, whole[int(starts[ep]):]) for ep in range(3)])
        assert [r.matches for r in res] == [False, False, True]
        both = verify_replay(eng, [(regen.handle, ep, whole[int(starts[ep]):]) for ep in range(3)])
        assert all(r.matches for r in both)
        assert verify_replay(eng, []) == []
