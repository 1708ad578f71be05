"""The inputs of tests/test_gpu_scan_outputs.py, built without a GPU, so that
tests/test_scan_ref.py can pin on the CPU what each one reaches: the anchors a
planted input holds, the path each wave-tile takes, the boundaries the random
input's anchors straddle.

Planted inputs are zero backgrounds with scan_ref.plant()ed anchors.  Two plants
of one parity must be 32 bytes or more apart (an anchor's window is the 31 bytes
ending at it); plants of different parity never see each other, so q and q + 1
are two anchors in one 16-byte piece, and pieces 16 bytes apart can each hold
one when their parities alternate."""
import functools

import numpy as np

from oracle import oracle
from tests import scan_ref as sr

KIB, MIB = 1 << 10, 1 << 20
WT, LSPAN, HALF, STILE = sr.WT, sr.LSPAN, sr.HALF, sr.STILE

# splitmix64 seed of the random input: its first 6 MiB hold an anchor (at rate
# 1/4096) within 31 bytes after a wave-tile start that is not a wave's first
# under ZC_TEST_SCAN_WGS = 1 or 3 (wave-tile 12), and after lane-span and
# half-span starts (pinned in test_scan_ref.py)
RANDOM_SEED = 11
RANDOM_BYTES = 8 * MIB + 300 * KIB


@functools.lru_cache(maxsize=None)
def random_bytes():
    oracle.build()
    buf = oracle.splitmix64(RANDOM_BYTES, RANDOM_SEED)
    buf.setflags(write=False)
    return buf


def random_input(n):
    return random_bytes()[:n]


# --- lengths (random bytes, W = 65536) ----------------------------------------
LENGTHS = [1, 62, 63, 64, 65, 1023, 1024, 1025, 256 * KIB - 1, 256 * KIB, 256 * KIB + 1,
           2 * MIB - 1, 2 * MIB, 2 * MIB + 1, 4 * MIB + 300 * KIB + 17]

# --- chunk sizes (random bytes, 6 MiB + 5) ------------------------------------
W_CASE_BYTES = 6 * MIB + 5
# W -> the regimes of its full wave-tiles
W_CASES = {4096: {"rescan"}, 256: {"rescan"}, 32768: {"fast", "rescan"}, 65536: {"fast"}, 262144: {"fast"},
           12288: {"rescan"}, 1 << 20: {"fast"}}

# --- planted edges -------------------------------------------------------------
EDGE_BYTES = 4 * MIB + 256 * KIB
EDGE_D = [0, 1, 2, 13, 14, 15, 16, 29, 30, 31, 32]
EDGE_WS = [65536, 4096]
_EVEN = [2 + 2 * i for i in range(11)]    # lanes 2 .. 22
_ODD = [23 + 2 * i for i in range(11)]    # lanes 23 .. 43


def _lane(wt, lane, off=0):
    return wt * WT + lane * LSPAN + off


# kind -> its 11 instances (one per d): every boundary in an even and an odd lane
# (odd lanes take their span's halves in the other order)
EDGE_BASES = {
    "lane span start, even lane": [_lane(1, L) for L in _EVEN],
    "lane span start, odd lane": [_lane(1, L) for L in _ODD],
    "half span start, even lane": [_lane(2, L, HALF) for L in _EVEN],
    "half span start, odd lane": [_lane(2, L, HALF) for L in _ODD],
    "1 KiB boundary, even lane": [_lane(3, L, KIB if i & 1 else 3 * KIB) for i, L in enumerate(_EVEN)],
    "1 KiB boundary, odd lane": [_lane(3, L, KIB if i & 1 else 3 * KIB) for i, L in enumerate(_ODD)],
    "128 B boundary, even lane": [_lane(4, L, 5 * 128 if i & 1 else HALF + 3 * 128) for i, L in enumerate(_EVEN)],
    "128 B boundary, odd lane": [_lane(4, L, 5 * 128 if i & 1 else HALF + 3 * 128) for i, L in enumerate(_ODD)],
    "16 B boundary, even lane": [_lane(5, L, 9 * 128 + 48 if i & 1 else HALF + 128 + 80)
                                 for i, L in enumerate(_EVEN)],
    "16 B boundary, odd lane": [_lane(5, L, 9 * 128 + 48 if i & 1 else HALF + 128 + 80) for i, L in enumerate(_ODD)],
    # wave-tile starts other than a 2 MiB tile's, in both full tiles
    "wave-tile start": [t * WT for t in (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 15)],
}
# boundaries a stream has one of: stream j plants d = EDGE_D[j] there
EDGE_SINGLE = {"2 MiB tile start": 2 * MIB, "tail's first byte": 4 * MIB}


def edge_plants(j, W):
    """Stream j of 11: {position: what} of its plants.  Instance i of
    every kind gets d = EDGE_D[(i + j) % 11], so each stream holds every d at
    every kind of boundary, and the 11 streams hold every d at every instance."""
    plants = {}
    for kind, bases in EDGE_BASES.items():
        for i, base in enumerate(bases):
            d = EDGE_D[(i + j) % 11]
            plants[base + d] = f"{kind} + {d}"
    for kind, base in EDGE_SINGLE.items():
        plants[base + EDGE_D[j]] = f"{kind} + {EDGE_D[j]}"
    plants[EDGE_BYTES - 1] = "the stream's last byte"
    # the first position that may be an anchor, and the last that may not
    plants[63 if j % 2 == 0 else 62] = "position 63" if j % 2 == 0 else "position 62 (no anchor)"
    return plants


@functools.lru_cache(maxsize=None)
def edge_input(j, W):
    """(data, the positions planted that may be anchors, {position: what})."""
    return _planted(EDGE_BYTES, edge_plants(j, W), W)


def _planted(n, plants, W):
    buf = np.zeros(n, dtype=np.uint8)
    for q in plants:
        sr.plant(buf, q, W)
    buf.setflags(write=False)
    return buf, np.array(sorted(q for q in plants if q >= sr.MIN_OFF), dtype=np.uint64), plants


# --- capacity edges (W = 65536: list of 144 pieces, pool share of 192) ---------
CAP_W = 65536
CAP_BYTES = 4 * MIB + 256 * KIB + 100


def singles(wt, count):
    """`count` pieces of wave-tile wt with one anchor each, spread over its lanes."""
    return [_lane(wt, (7 * k) % 64, 16 * (20 + 2 * (k // 64)) + 14) for k in range(count)]


def pairs(wt, count):
    """`count` pieces with two anchors each (q and q + 1)."""
    out = []
    for q in singles(wt, count):
        out += [q, q + 1]
    return out


def one_lane(wt, lane, count):
    """`count` consecutive pieces of one lane span with one anchor each, centred
    on the span's middle (so in both halves): parities alternate piece by piece."""
    first = 128 - count // 2
    return [_lane(wt, lane, 16 * (first + k) + 14 + (k & 1)) for k in range(count)]


def spread(wt, count):
    """`count` one-anchor pieces, count // 64 or one more per lane (144 entries
    cannot be one or two per lane: 64 lanes hold 128 that way; they are two or
    three), a lane's entries alternating between its halves."""
    return [_lane(wt, k % 64, (HALF if (k // 64) & 1 else 0) + 16 * (9 + k // 64) + 14) for k in range(count)]


def _few(wt):
    return [_lane(wt, 5, 700), _lane(wt, 40, HALF + 333), _lane(wt, 63, LSPAN - 1)]


# name -> (the plants of the wave-tile under test, its index, its expected regime, side-pool flag)
CAP_FULL, CAP_TAIL = 3, 16
CAP_CASES = {
    "143 pieces": (singles, 143, "fast", False),
    "144 pieces": (singles, 144, "fast", False),
    "145 pieces": (singles, 145, "rescan", True),
    "96 pairs": (pairs, 96, "fast", False),
    "97 pairs": (pairs, 97, "rescan", True),
    "144 in one even lane": (lambda wt, c: one_lane(wt, 20, c), 144, "fast", False),
    "144 in one odd lane": (lambda wt, c: one_lane(wt, 21, c), 144, "fast", False),
    "145 in one lane": (lambda wt, c: one_lane(wt, 20, c), 145, "rescan", True),
    "144 spread": (spread, 144, "fast", False),
}
# the counts again in the tail's first wave-tile: no list there, only the pool share
CAP_TAIL_CASES = {
    "143 pieces": (singles, 143, False),
    "144 pieces": (singles, 144, False),
    "145 pieces": (singles, 145, False),
    "96 pairs": (pairs, 96, False),
    "97 pairs": (pairs, 97, True),
}


@functools.lru_cache(maxsize=None)
def cap_input(name, tail):
    if tail:
        make, count, _ = CAP_TAIL_CASES[name]
        wt = CAP_TAIL
    else:
        make, count, _, _ = CAP_CASES[name]
        wt = CAP_FULL
    qs = make(wt, count) + _few(wt - 1) + (_few(wt + 1) if not tail else [CAP_BYTES - 1])
    return _planted(CAP_BYTES, {q: name for q in qs}, CAP_W)


@functools.lru_cache(maxsize=None)
def two_overflows_input():
    """Wave-tiles 3 (list overflow), 4 (fast, between them), 9 (pool share
    overflow) and the tail's first (pool share overflow): three shares in the
    side pool."""
    qs = singles(3, 145) + singles(4, 144) + pairs(9, 97) + pairs(CAP_TAIL, 100) + _few(2) + _few(10)
    return _planted(CAP_BYTES, {q: "two overflows" for q in qs}, CAP_W)


TWO_OVERFLOWS_SIDE = {3, 9, CAP_TAIL}

# --- several wave-tiles per wave (ZC_TEST_SCAN_WGS) ----------------------------
WGS_PATTERN = [0, 1, 144, 145]   # anchor pieces of wave-tile t: WGS_PATTERN[t % 4]


@functools.lru_cache(maxsize=None)
def wgs_planted_input(n, W):
    """Wave-tiles alternate between 0, 1, 144 and 145 one-anchor pieces: the tile
    end's store count differs from tile to tile, and a rescanned wave-tile (which
    stores nothing) lies between fast ones."""
    qs = []
    for t in range(n // WT):
        qs += singles(t, WGS_PATTERN[t % 4])
    return _planted(n, {q: "pattern" for q in qs}, W)
