"""TEST INFRASTRUCTURE: the chunk metadata record (zc_chunk_meta) restated in
plain Python, independent of zbackup_amd/csrc/zc_meta_core.h: hashlib's SHA-1
and integers mod 2^64.

For a chunk b[0, size) under a context with chunk.max_size W:
  rolling      257^size + sum b[i] 257^(size-1-i)  mod 2^64   (RollingHash::digest)
  sha1         the first 16 bytes of SHA-1(b)
  anchor       the smallest q in [63, W-1] with (int16) st(q) >= anchor_lo(W), where
               st(q) = sum_{j<16} b[q-2j] 2^j mod 2^16 -- only when size == W > 63
  gear         st(q-1) | st(q) << 16
  fingerprint  b[q-7 .. q] as a little-endian 64-bit word
"""
import hashlib

import numpy as np

M64 = (1 << 64) - 1
NO_ANCHOR = 0xFFFFFFFF
ANCHOR_MIN_OFF = 63
BAD_SHA1, BAD_ROLLING, BAD_SIZE = 1, 2, 4

META_DTYPE = np.dtype([("sha1", np.uint8, 16), ("rolling", "<u8"), ("size", "<u4"), ("anchor_def", "<u4"),
                       ("anchor", "<u4"), ("gear", "<u4"), ("fingerprint", "<u8")])


def anchor_rate_inv(W):
    r = 16
    while r < 4096 and r * 2 <= W // 16:
        r *= 2
    return r


def anchor_lo(W):
    return 0x8000 - 0x10000 // anchor_rate_inv(W)


def anchor_def(W):
    return 0x5A410000 | (2 << 8) | (anchor_rate_inv(W).bit_length() - 1)


def rolling(b):
    acc = 0
    for x in bytes(b):
        acc = (acc * 257 + x) & M64
    return (pow(257, len(b), 1 << 64) + acc) & M64


def st(b, q):
    """The 16-bit gear at position q of b (q >= 30)."""
    return sum(b[q - 2 * j] << j for j in range(16)) & 0xFFFF


def is_anchor(b, q, W):
    v = st(b, q)
    return (v - 0x10000 if v & 0x8000 else v) >= anchor_lo(W)


def first_anchor(b, W):
    """(anchor, gear, fingerprint) of chunk b under W."""
    b = bytes(b)
    if len(b) != W or W <= ANCHOR_MIN_OFF:
        return NO_ANCHOR, 0, 0
    arr = np.frombuffer(b, dtype=np.uint8).astype(np.int64)
    # st at every q >= 30, sixteen shifted adds
    n = len(b)
    s = np.zeros(n, dtype=np.int64)
    for j in range(16):
        s[30:] += arr[30 - 2 * j:n - 2 * j] << j
    s &= 0xFFFF
    signed = np.where(s & 0x8000, s - 0x10000, s)
    hits = np.nonzero(signed[ANCHOR_MIN_OFF:] >= anchor_lo(W))[0]
    if not len(hits):
        return NO_ANCHOR, 0, 0
    q = int(hits[0]) + ANCHOR_MIN_OFF
    assert int(s[q]) == st(b, q) and is_anchor(b, q, W)
    return q, st(b, q - 1) | st(b, q) << 16, int.from_bytes(b[q - 7:q + 1], "little")


def record(b, W):
    """The record of chunk b under W as a META_DTYPE scalar array (shape (1,))."""
    b = bytes(b)
    r = np.zeros(1, dtype=META_DTYPE)
    r["sha1"][0] = np.frombuffer(hashlib.sha1(b).digest()[:16], dtype=np.uint8)
    r["rolling"] = rolling(b)
    r["size"] = len(b)
    r["anchor_def"] = anchor_def(W)
    r["anchor"], r["gear"], r["fingerprint"] = first_anchor(b, W)
    return r


def records(chunks, W):
    return np.concatenate([record(c, W) for c in chunks]) if len(chunks) else np.zeros(0, dtype=META_DTYPE)


def status(rec, expect_sha1, expect_rolling, expect_size):
    """What differs between a record and the id a bundle claims."""
    return ((BAD_SHA1 if bytes(rec["sha1"]) != bytes(expect_sha1) else 0) |
            (BAD_ROLLING if int(rec["rolling"]) != int(expect_rolling) else 0) |
            (BAD_SIZE if int(rec["size"]) != int(expect_size) else 0))

