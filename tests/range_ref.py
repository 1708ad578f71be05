"""TEST INFRASTRUCTURE: numpy restatements of the range index's host side.

`needs` is zc_range_needs: the distinct slots a batch of reads touches, found
with searchsorted over the cumulative sizes.  `read` is one read served from
host copies of the slots (the slice of the concatenated stream, without ever
building the stream)."""
import numpy as np


def positions(sizes):
    """pos[e] = the stream position of entry e's first byte; pos[n] = the total."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)


def entries_of(pos, offset, size):
    """The non-empty entries that overlap [offset, offset + size), ascending."""
    if size == 0:
        return np.zeros(0, dtype=np.int64)
    first = int(np.searchsorted(pos, np.uint64(offset), side="right")) - 1
    last = int(np.searchsorted(pos, np.uint64(offset + size), side="left"))  # the first entry at or past the end
    e = np.arange(first, min(last, len(pos) - 1), dtype=np.int64)
    return e[pos[e + 1] > pos[e]]


def needs(slot, sizes, reads):
    pos = positions(sizes)
    slot = np.asarray(slot)
    seen = set()
    for offset, size in reads:
        seen.update(int(s) for s in slot[entries_of(pos, int(offset), int(size))])
    return sorted(seen)


def read(slots, slot, off, sizes, offset, size):
    """bytes [offset, offset + size) of the stream; slots[k] = a numpy uint8 array."""
    pos = positions(sizes)
    out = []
    for e in entries_of(pos, offset, size):
        a, b = max(int(pos[e]), offset), min(int(pos[e + 1]), offset + size)
        o = int(off[e]) + a - int(pos[e])
        out.append(slots[int(slot[e])][o:o + b - a])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)
