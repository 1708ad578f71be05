"""A small LZO1X token assembler and a hand-built match grid for the decoder
core's tests (tests/test_unlzo_grid.py): valid streams made token by token, so
that the match forms (M2, M3, M4), the extended lengths and the distances and
lengths around 64 bytes -- one copy step of a wave-wide sink, the replicating
k % dist form on both sides of it -- are hit on purpose, not by what a
compressor happens to emit.  liblzo2's lzo1x_decompress_safe decodes every
stream for the expectation; a stream it rejects is a bug here.

The format (lzo1x_d.ch of liblzo2 2.10; zc_lzo_dec.h walks the same):
  first byte 17 + L (L <= 238)      a literal run of L bytes
  t = 1..15 / 0 + zero run          a literal run of t + 3 bytes (0: 18 + 255 * zeros + last byte)
  M2  t >= 64                       len 3..8, dist 1..2048
  M3  32 <= t < 64                  len 2 + (t & 31) (0: extended by 31 + ...), dist 1..16384
  M4  16 <= t < 32                  len 2 + (t & 7) (0: extended by 7 + ...), dist 16385..49151
  the low two bits of a match's distance byte = 0-3 trailing literals, which follow it
  17 0 0                            the end marker (an M4 of distance 0)
"""
import numpy as np

from tests.unlzo_inputs import frame_stream

DISTS = [1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2048, 2049, 16384, 16385, 49151]
LENS = [3, 4, 63, 64, 65, 127, 128, 129, 1000]
TRAILS = [0, 1, 2, 3]


def _ext(n):
    """n >= 1 as a run of zero bytes (255 each) and a last byte of 1..255."""
    out = bytearray()
    while n > 255:
        out.append(0)
        n -= 255
    out.append(n)
    return bytes(out)


def literal_run(data, first):
    """A literal run of len(data) >= 4 bytes; `first`: at the start of the stream."""
    L = len(data)
    assert L >= 4
    if first and L <= 238:
        return bytes([17 + L]) + data
    t = L - 3
    head = bytes([t]) if t <= 15 else b"\0" + _ext(t - 15)
    return head + data


def match(dist, length, trail=b""):
    """One match of `length` >= 3 bytes from `dist` back, then 0-3 trailing
    literals; returns (token bytes, its kind)."""
    assert length >= 3 and 1 <= dist <= 49151 and len(trail) <= 3
    if length <= 8 and dist <= 2048:
        d = dist - 1
        return bytes([(length - 1) << 5 | (d & 7) << 2 | len(trail), d >> 3]) + trail, "M2"
    if dist <= 16384:
        d, t = dist - 1, length - 2
        head = bytes([32 | t]) if t <= 31 else bytes([32]) + _ext(t - 31)
        return head + bytes([(d & 63) << 2 | len(trail), d >> 6]) + trail, "M3"
    d, t = dist - 0x4000, length - 2
    hb = 16 | (d >> 14 & 1) << 3
    head = bytes([hb | t]) if t <= 7 else bytes([hb]) + _ext(t - 7)
    return head + bytes([(d & 63) << 2 | len(trail), d >> 6 & 0xFF]) + trail, "M4"


END = bytes([17, 0, 0])


def grid_cases(seed=5):
    """[(framed, decoded size, (dist, len, trailing, kind))]: a literal run of
    at least `dist` random bytes, one match (dist, len) with 0-3 trailing
    literals, a second match whose distance is the bytes just written (the
    first match and its trailing literals: the freshest stores), the end."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (dist, length, ntrail) in enumerate((d, n, t) for d in DISTS for n in LENS for t in TRAILS):
        run = bytes(rng.integers(0, 256, max(dist, 4) + i % 5, dtype=np.uint8))
        trail = bytes(rng.integers(0, 256, ntrail, dtype=np.uint8))
        m1, kind = match(dist, length, trail)
        len2 = (3, 8, 67, 200)[i % 4]
        m2, _ = match(length + ntrail, len2)
        z = literal_run(run, True) + m1 + m2 + END
        out.append((frame_stream(len(run) + length + ntrail + len2, z), len(run) + length + ntrail + len2,
                    (dist, length, ntrail, kind)))
    return out
