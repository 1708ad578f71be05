"""A plain reference for every word the scan leaves behind (numpy and Python
ints, no GPU): content anchors with their gear words, the 1 KiB span digests,
the scan-written grid keys, and which path a wave-tile takes.  The geometry and
the anchor rate restate zbackup_amd/csrc/zc_device.h; nothing here is derived
from the kernels' own arithmetic (no packed states, no folded span digests).

    st(q) = sum_{j<16} b[q - 2j] * 2^j  mod 2^16      (bytes before the stream: 0)
    q is an anchor  iff  (int16) st(q) >= anchor_lo(W)  and  q >= 63
    gear(q) = st(q - 1) | st(q) << 16
"""
import numpy as np

SPAN = 1024            # digest granularity
LSPAN = 4096           # a scan lane's span
HALF = LSPAN // 2      # odd lanes take their two halves in the other order
WT = 64 * LSPAN        # wave-tile: 256 KiB, one scan wave
STILE = 8 * WT         # 2 MiB tile: the scan kernel's unit; the rest is the tail kernel's
PIECE = 16             # the scan tests and lists anchors per 16-byte piece
WLIST = 144            # pieces a wave's LDS list holds (ZC_WLIST)
MIN_OFF = 63           # ZC_ANCHOR_MIN_OFF
M64 = (1 << 64) - 1


def anchor_rate_inv(W):
    r = 16
    while r < 4096 and r * 2 <= W // 16:
        r *= 2
    return r


def anchor_lo(W):
    return 0x8000 - 0x10000 // anchor_rate_inv(W)


def wave_tile_cap(W):
    """A wave-tile's share of the anchor pool."""
    return 2 * (WT // anchor_rate_inv(W)) + 64


def states(data):
    """st(q) of every position, as uint16."""
    b = np.asarray(data, dtype=np.uint8).astype(np.uint32)
    st = np.zeros(b.size, dtype=np.uint32)
    for j in range(16):
        if b.size > 2 * j:
            st[2 * j:] += b[:b.size - 2 * j] << np.uint32(j)
    return (st & 0xFFFF).astype(np.uint16)


def _hits(st, W):
    """st(q) passes the anchor test (positions below 63 included)."""
    return st.view(np.int16) >= anchor_lo(W)


def model_anchors(data, W):
    """The anchor positions of `data` at chunk size W (a bool per position)."""
    hit = _hits(states(data), W)
    hit[:MIN_OFF] = False
    return hit


def anchors(data, W):
    """(positions uint64, gear words uint32) of every anchor, in position order."""
    r = analyse(data, W)
    return r.pos, r.gear


def _horner_rows(rows):
    """acc = acc * 257 + b (mod 2^64) along each row of a 2-d uint8 array."""
    acc = np.zeros(rows.shape[0], dtype=np.uint64)
    m = np.uint64(257)
    with np.errstate(over="ignore"):
        for k in range(rows.shape[1]):
            acc = acc * m + rows[:, k]
    return acc


def span_digests(data):
    """The Horner value of every 1 KiB span from 0; the partial last span is
    that of the bytes present."""
    data = np.asarray(data, dtype=np.uint8)
    full = data.size // SPAN
    out = _horner_rows(data[:full * SPAN].reshape(full, SPAN))
    if data.size % SPAN:
        acc = 0
        for b in data[full * SPAN:].tolist():
            acc = (acc * 257 + b) & M64
        out = np.append(out, np.uint64(acc))
    return out


def grid_keys(data, W):
    """257^W + the Horner value (mod 2^64) of every whole W-byte grid chunk
    [i W, (i + 1) W) inside the stream's full 2 MiB tiles."""
    data = np.asarray(data, dtype=np.uint8)
    cnt = data.size // STILE * STILE // W
    acc = _horner_rows(data[:cnt * W].reshape(cnt, W))
    with np.errstate(over="ignore"):
        return acc + np.uint64(pow(257, W, 1 << 64))


def scan_writes_keys(W):
    """The scan writes grid keys when a chunk is whole lane spans of one wave."""
    return W >= LSPAN and W % LSPAN == 0 and WT % W == 0


class Analysis:
    """pos, gear: anchors(); regime, side_pool: per wave-tile (see those functions)."""


def analyse(data, W):
    """Everything below from one pass over the states."""
    data = np.asarray(data, dtype=np.uint8)
    n = data.size
    st = states(data)
    raw = _hits(st, W)
    anc = raw.copy()
    anc[:MIN_OFF] = False
    r = Analysis()
    pos = np.flatnonzero(anc)
    r.pos = pos.astype(np.uint64)
    r.gear = st[pos - 1].astype(np.uint32) | (st[pos].astype(np.uint32) << np.uint32(16))
    full, cap = n // STILE * STILE, wave_tile_cap(W)
    r.regime, r.side_pool = [], []
    for t in range(-(-n // WT)):
        a, b = t * WT, min((t + 1) * WT, n)
        count = int(anc[a:b].sum())
        if a >= full:
            r.regime.append("tail")
            r.side_pool.append(count > cap)
            continue
        pieces = int(raw[a:b].reshape(-1, PIECE).any(axis=1).sum())
        r.regime.append("fast" if pieces <= WLIST and count <= cap else "rescan")
        r.side_pool.append(r.regime[-1] == "rescan")
    return r


def regime(data, W):
    """Per wave-tile t < ceil(n / 256 KiB): "tail" (the partial last 2 MiB tile:
    zc_scan_tail_kernel), "fast" (the scan kernel's own tile end stores the
    anchors) or "rescan" (its list or its pool share overflowed: the exact
    rescan).  The scan lists a piece when any st(q) in it passes the test --
    the stream's first 63 positions included, which are no anchors -- so
    pieces are counted by that, anchors by the definition."""
    return analyse(data, W).regime


def side_pool(data, W):
    """Whether each wave-tile's directory entry points into the side pool: where
    it was rescanned; in the tail (wave_tile_block) where its anchors exceed the
    pool share, which marks it overflowed for the same rescan."""
    return analyse(data, W).side_pool


def plant(buf, q, W):
    """One anchor at q on a zero background: st(q) = 0x7F80 from buf[q - 14] =
    0xFF (j = 7), and at rates above 256 (anchor_lo above 0x7F00) buf[q - 8] = 7
    (j = 4) makes it 0x7FF0.  st(q + 2k) has bit 15 set until the bytes leave
    the window, st(q - 2k) is below 0x4000, and the other parity sees none of
    it: the plant is a lone anchor.  Returns its gear word (st(q - 1) = 0 when
    nothing else is near)."""
    buf[q - 14] = 0xFF
    if anchor_rate_inv(W) > 256:
        buf[q - 8] = 7
        return 0x7FF0 << 16
    return 0x7F80 << 16


def where(pos):
    """A position as the scan sees it, for failure messages."""
    pos = int(pos)
    in_span = pos % LSPAN
    return (f"position {pos}: wave-tile {pos // WT}, lane span {pos % WT // LSPAN} "
            f"({'odd' if pos % WT // LSPAN & 1 else 'even'} lane), half {in_span // HALF}, "
            f"round {in_span // 128}, piece {in_span % 128 // PIECE}, offset {pos % PIECE} in the piece")
