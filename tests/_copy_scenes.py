"""Scenes of the byte-copy edge tests (test_gpu_copy_edges.py), free of engine calls: positions,
residues, lengths, piece counts and chunk counts, and the bytes a correct copy leaves behind.
test_copy_edges_scene.py checks the coverage these scenes claim without a GPU.

Conventions: data bytes are drawn from 1..254; destination buffers and the gaps of source
buffers hold FILL (0xFF), so a store that did not happen shows as 0xFF and a load that
copy_range skipped (it zero-fills) shows as 0x00.  Segments, the engine's pools and every
buffer base are 16-byte aligned, so a residue is a position mod 16.
"""
import numpy as np

FILL = 0xFF
SLACK = 64  # bytes past the last byte written that every device-output check still compares

SHORT_L = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 79, 80, 81]  # packed gather
ISO_L = [1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 64, 65]  # isolated gather
SCATTER_L = [1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65]  # scatter, in-flight pool
BIG_SEG = 16384


def data(n, seed):
    """n bytes from 1..254."""
    return np.random.default_rng(seed).integers(1, 255, n, dtype=np.uint8).tobytes()


def chunks(dst, n):
    """16-byte destination chunks copy_range walks for [dst, dst + n)."""
    return ((dst + n + 15) // 16) - dst // 16 if n else 0


def trips(nch, nt):
    """Trips of copy_range's loop (kCopyK = 4 chunks per thread and trip, nt threads)."""
    return (nch + 4 * nt - 1) // (4 * nt)


def pieces(phys, n, seg, dst):
    """[phys, phys + n) of a log cut at segment boundaries (add_pieces, k_expand_pieces):
    (position in the log, place in the output, length) per piece."""
    out = []
    while n > 0:
        take = min(n, seg - phys % seg)
        out.append((phys, dst, take))
        phys, dst, n = phys + take, dst + take, n - take
    return out


def place(items):
    """Bodies in one source buffer: item (length, residue) goes to the first position past the
    previous body whose residue mod 16 is `residue`.  Returns (positions, buffer size); the
    buffer ends with at least 16 fill bytes."""
    pos, at = [], 0
    for n, s in items:
        p = (at + 15) // 16 * 16 + s
        pos.append(p)
        at = p + n
    return pos, (at + 15) // 16 * 16 + 16


def source_buffer(bodies, pos, size):
    buf = np.full(size, FILL, np.uint8)
    for b, p in zip(bodies, pos):
        buf[p:p + len(b)] = np.frombuffer(b, np.uint8)
    return buf


def packed(parts, d, lead=16):
    """The device buffer after a gather of `parts` back to back at residue d of a buffer that
    held FILL: `lead` bytes before the output base's chunk are part of it, SLACK after."""
    body = b"".join(parts)
    before = lead + d
    return bytes([FILL]) * before + body + bytes([FILL]) * (buffer_size(len(body), lead) - before - len(body))


def buffer_size(total, lead=16):
    """Room for `lead` bytes, any residue below 16, the output and SLACK."""
    return lead + 16 + total + SLACK


# ---- part 1: gather, short ranges --------------------------------------------------------------
EPOCH_LENS = [96] + [97] * 15  # epoch t ends at a log position congruent to t mod 16


def epoch_starts():
    return [int(x) for x in np.cumsum([0] + EPOCH_LENS[:-1])]


def short_log():
    return data(sum(EPOCH_LENS), 11)


def short_requests():
    """(t, L) in batch order: the consumer of request k (channel k + 1) stands at len_t - L of
    epoch t and receives that epoch's last L bytes."""
    return [(t, L) for t in range(16) for L in SHORT_L]


def short_range(t, L):
    """(log position, length) of request (t, L)."""
    return epoch_starts()[t] + EPOCH_LENS[t] - L, L


def short_parts(log, reqs):
    return [log[p:p + n] for p, n in (short_range(t, L) for t, L in reqs)]


def short_triples(reqs, d):
    """(source residue, destination residue, L) of every request of a packed batch at base
    residue d."""
    out, off = set(), 0
    for t, L in reqs:
        out.add((short_range(t, L)[0] % 16, (d + off) % 16, L))
        off += L
    return out


def isolated_cases():
    """(t, d, L): case k owns slot k (256 bytes) of one buffer and writes at slot + d."""
    return [(t, d, L) for t in range(16) for d in range(16) for L in ISO_L]


ISO_SLOT = 256


def isolated_expect(log, cases):
    buf = np.full(len(cases) * ISO_SLOT + SLACK, FILL, np.uint8)
    for k, (t, d, L) in enumerate(cases):
        p, n = short_range(t, L)
        buf[k * ISO_SLOT + d:k * ISO_SLOT + d + n] = np.frombuffer(log[p:p + n], np.uint8)
    return buf.tobytes()


# piece counts (segments of 64 bytes): one epoch of 25 segments; a consumer at 1600 - 64 n
# receives n whole segments, n pieces, n blocks
COUNT_SEG, COUNT_N = 64, 25


def count_log():
    return data(COUNT_SEG * COUNT_N, 12)


def count_batches():
    """Batches of segment counts: every n alone, then three requests whose pieces total 16 + r."""
    return [[n] for n in range(1, COUNT_N + 1)] + [[2, 5, 9 + r] for r in range(8)]


def count_pieces(batch):
    return sum(len(pieces(COUNT_SEG * (COUNT_N - n), COUNT_SEG * n, COUNT_SEG, 0)) for n in batch)


# host-planned pieces (clg_get_determinants into device memory): a lead of r bytes in epoch 0
# (none for r = 0), L bytes in epoch 1; getDeterminants(1) is the range [r, r + L)
PLAN_CASES = [(r, L) for r in (0, 1, 15) for L in (1, 17, 65)]


# ---- part 2: loop-trip edges ---------------------------------------------------------------------
TRIP_LOG = 3 * BIG_SEG + 5
TRIP_OFFSETS = [0, 1, 15, 16, 16383, 16384, 16385]
TRIP_BASES = [0, 1, 7, 15]


def trip_pieces(d):
    """(length, destination residue, chunks) of every piece of the batch at base residue d."""
    out, off = [], 0
    for o in TRIP_OFFSETS:
        for _, dst, n in pieces(o, TRIP_LOG - o, BIG_SEG, d + off):
            out.append((n, dst % 16, chunks(dst, n)))
        off += TRIP_LOG - o
    return out


TRIP_SCATTER_L = [4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 3 * 16384 + 5]
TRIP_RES = [0, 1, 15]


def trip_scatter_cases():
    """(writer residue w, source residue s, L): a log with a lead of w bytes, then L bytes."""
    return [(w, s, L) for w in TRIP_RES for s in TRIP_RES for L in TRIP_SCATTER_L]


def scatter_chunks(writer, n, seg):
    """Chunk lengths and chunk counts of a write of n bytes at log position `writer`
    (upstream_batch, flush): (destination position, length, 16-byte chunks) per segment."""
    return [(p, k, chunks(p, k)) for p, _, k in pieces(writer, n, seg, 0)]


# ---- part 3: scatter, short ranges ----------------------------------------------------------------
SCATTER_SEG = 64


def scatter_cases():
    return [(w, s, L) for w in range(16) for s in range(16) for L in SCATTER_L]


def ends_on_segment_end(w, L, seg=SCATTER_SEG):
    return (w + L) % seg == 0


def starts_on_segment_start(w, L, seg=SCATTER_SEG):
    """The body, or its part in the next segment, starts on a segment's first byte."""
    return w % seg == 0 or w + L > seg


def staged_cases():
    """Host-staged appends: log i has a flushed lead of i mod 16 bytes, then one append_batch
    gives every log one body, lengths cycling through SCATTER_L out of step with the leads."""
    return [(i % 16, SCATTER_L[(i // 3) % len(SCATTER_L)]) for i in range(16 * len(SCATTER_L) * 2)]


def staged_shifts(cases):
    """(source - destination) & 15 of every body: the flush packs the pending bytes back to
    back in the staging buffer in the order the logs became dirty; the destination is the
    log's writer."""
    out, at = [], 0
    for w, L in cases:
        out.append((at - w) & 15)
        at += L
    return out


# ---- part 4: in-flight pool ---------------------------------------------------------------------
IFL_BASES = [0, 1, 7, 15]


def ifl_cases(seg):
    """(length, source residue) of the buffers logged, in order."""
    ls = SCATTER_L + ([BIG_SEG, BIG_SEG + 1] if seg == BIG_SEG else [])
    return [(L, s) for L in ls for s in range(16)]
