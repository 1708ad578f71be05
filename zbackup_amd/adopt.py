"""Adopting an existing repository: the chunk metadata (zc_chunk_meta) and the
full ChunkId of every chunk, recomputed from decoded bundle payloads.

  Bundle::Reader::Reader / get  -> where each chunk lies      bundle.cc:220-251
  ChunkId (cryptoHash, rollingHash) of the bytes read back    chunk_id.hh:16-32

A repository stock zbackup wrote is known to the engine by chunk id only, so
its ids go through the exact screen at every byte.  The metadata record that
moves an id to the anchor path is a pure function of the chunk's bytes:
`Adopter.adopt` computes it for every chunk of the bundles given, compares the
recomputed id with the one each bundle claims (a scrub zbackup does not have),
and `write_sidecar` stores the result where the zbackup-side binding reads it
(GpuChunkMetaSidecar, integration/gpu_backup_creator.hh).  Decoding the bundles
(LZMA or lzo1x) is the caller's step, as for `Restorer`; so is reading the
BundleInfo records.  All hashing runs in libzchunk.so on the GPU
(zc_chunk_meta_compute); there is no CPU fallback.
"""
import ctypes
import hashlib
import os
import struct
import time

import numpy as np

from . import _lib
from .chunker import META_DTYPE, SEED_DTYPE, _check

SIDECAR_MAGIC = b"ZCMETA01"
assert META_DTYPE.itemsize == ctypes.sizeof(_lib.ZcChunkMeta) == 48


class AdoptReport:
    """What one adoption found.  `meta`: the records of the size-W chunks whose
    recomputed id equals the bundle's (what zc_seed_index_meta takes), in bundle
    order; `bad`: (bundle, index in the bundle, status) of every chunk whose id
    or size differs (ZC_META_BAD_* bits); `chunks`, `bytes`: what was read."""
    __slots__ = ("meta", "bad", "chunks", "bytes")


def bundle_layout(bundles, payloads):
    """Where the chunks of `bundles[b] = [(24-byte id blob, size), ...]` lie once
    `payloads[b]` are put back to back: (off uint64, size uint32, expect
    SEED_DTYPE, bundle_first).  Raises ZcError naming the bundle whose payload
    is not the sum of its chunk sizes."""
    if len(bundles) != len(payloads):
        raise _lib.ZcError(f"adopt: {len(bundles)} bundles, {len(payloads)} payloads")
    return chunk_layout(bundles, [len(p) for p in payloads])


def chunk_layout(bundles, payload_sizes=None):
    """bundle_layout from sizes alone: payload_sizes[b] = the bytes of bundle
    b's payload (None: whatever its chunks take)."""
    n = sum(len(b) for b in bundles)
    off, size = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    expect = np.zeros(n, dtype=SEED_DTYPE)
    bundle_first, pos, i = [0], 0, 0
    for b, chunks in enumerate(bundles):
        total = 0
        for blob, sz in chunks:
            blob = bytes(blob)
            if len(blob) != 24:
                raise _lib.ZcError(f"adopt: bundle {b}: a chunk id of {len(blob)} bytes")
            off[i], size[i] = pos + total, int(sz)
            expect["sha1"][i] = np.frombuffer(blob[:16], dtype=np.uint8)
            expect["rolling"][i] = struct.unpack("<Q", blob[16:])[0]
            expect["size"][i] = int(sz)
            total += int(sz)
            i += 1
        if payload_sizes is not None and payload_sizes[b] != total:
            raise _lib.ZcError(f"adopt: bundle {b} decoded to {payload_sizes[b]} bytes, its chunks take {total}")
        pos += total
        bundle_first.append(i)
    return off, size, expect, bundle_first


def build_report(bundle_first, meta, status, chunk_max_size):
    """The AdoptReport of one call's records and statuses."""
    meta, status = np.asarray(meta), np.asarray(status)
    r = AdoptReport()
    keep = (status == 0) & (meta["size"] == chunk_max_size)
    r.meta = meta[keep].copy()
    r.bad = []
    first = np.asarray(bundle_first, dtype=np.int64)
    for i in np.nonzero(status)[0]:
        b = int(np.searchsorted(first, i, side="right")) - 1
        r.bad.append((b, int(i - first[b]), int(status[i])))
    r.chunks = int(len(meta))
    r.bytes = int(meta["size"].astype(np.uint64).sum())
    return r


class Adopter:
    """zc_chunk_meta_compute on a context of its own with chunk.max_size
    `chunk_max_size` (the anchor rate and which chunks carry an anchor follow it)."""

    def __init__(self, chunk_max_size, device=0):
        self._L = _lib.load()
        self.chunk_max_size = int(chunk_max_size)
        ctx = ctypes.c_void_p()
        rc = self._L.zc_create(ctypes.byref(ctx), self.chunk_max_size, device, 0)
        if rc != _lib.ZC_OK:
            raise _lib.ZcError(f"zc_create failed ({rc})")
        self._ctx = ctx
        self._call_ms = 0.0
        self.n_bad = 0
        self.xz_stats = None  # BundleDecompressor.last_stats() of the last adopt_bodies

    def _run(self, fn, what, payload, payload_bytes, off, size, expect):
        off = np.ascontiguousarray(off, dtype=np.uint64)
        size = np.ascontiguousarray(size, dtype=np.uint32)
        n = len(off)
        if len(size) != n:
            raise _lib.ZcError(f"{what}: {n} offsets, {len(size)} sizes")
        if expect is not None:
            expect = np.ascontiguousarray(expect, dtype=SEED_DTYPE)
            if len(expect) != n:
                raise _lib.ZcError(f"{what}: {n} chunks, {len(expect)} expected ids")
        meta = np.zeros(n, dtype=META_DTYPE)
        status = np.zeros(n, dtype=np.uint8)
        bad = ctypes.c_size_t()
        t = time.perf_counter()
        rc = fn(self._ctx, payload, int(payload_bytes), off.ctypes.data if n else None,
                size.ctypes.data if n else None, n, expect.ctypes.data if expect is not None and n else None,
                meta.ctypes.data if n else None, status.ctypes.data if n else None, ctypes.byref(bad))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, what)
        self.n_bad = int(bad.value)
        return meta, status

    def chunk_meta(self, d_payload, payload_bytes, off, size, expect=None):
        """The records of chunks d_payload[off[i] ..+ size[i]) (a device
        pointer, e.g. a torch uint8 tensor's data_ptr()) and, with `expect` (a
        SEED_DTYPE array: the ids the bundles claim), what differs per chunk:
        (META_DTYPE array, uint8 status array).  `n_bad` holds the count."""
        return self._run(self._L.zc_chunk_meta_compute, "zc_chunk_meta_compute", ctypes.c_void_p(d_payload),
                         payload_bytes, off, size, expect)

    def chunk_meta_host(self, payload, off, size, expect=None):
        """The same with the payload in host memory (bytes-like or a uint8 array)."""
        buf = np.ascontiguousarray(np.frombuffer(memoryview(payload), dtype=np.uint8))
        keep = buf if buf.size else np.zeros(1, dtype=np.uint8)
        return self._run(self._L.zc_chunk_meta_compute_host, "zc_chunk_meta_compute_host",
                         ctypes.c_void_p(keep.ctypes.data), buf.size, off, size, expect)

    def adopt(self, bundles, payloads):
        """bundles[b] = [(24-byte id blob, size), ...] (the shape Restorer.plan
        takes), payloads[b] = bundle b's decoded payload: one call over all of
        them laid back to back, the bundles' ids as the expected ones."""
        off, size, expect, bundle_first = bundle_layout(bundles, payloads)
        image = np.frombuffer(b"".join(bytes(p) for p in payloads) or b"\0", dtype=np.uint8)
        meta, status = self._run(self._L.zc_chunk_meta_compute_host, "zc_chunk_meta_compute_host",
                                 ctypes.c_void_p(image.ctypes.data), int(size.astype(np.uint64).sum()), off, size,
                                 expect)
        return build_report(bundle_first, meta, status, self.chunk_max_size)

    def adopt_bodies(self, bundles, bodies):
        """adopt() for LZMA bundles as they lie on disk: bodies[b] = bundle b's
        xz stream (zc_bundle_unseal's body).  The compressed bodies cross to the
        device, are decoded there back to back (zc_xz_decode; a stream that is
        not exactly its bundle's payload raises ZcError naming the bundle) and
        hashed where they land: the payloads never touch the host."""
        from .bundle import BundleDecompressor
        totals = [sum(int(s) for _, s in chunks) for chunks in bundles]
        off, size, expect, bundle_first = chunk_layout(bundles)
        if len(bodies) != len(bundles):
            raise _lib.ZcError(f"adopt: {len(bundles)} bundles, {len(bodies)} bodies")
        dec = BundleDecompressor(ctx=self._ctx)
        pay = (sum(totals) + 15) & ~15
        buf = dec.alloc(pay + dec.stage_size(bodies))
        try:
            out_off = np.concatenate([[0], np.cumsum(totals)[:-1]]).astype(np.uint64) if totals else []
            dec.decode_bodies(bodies, buf + pay, buf, out_off, totals)
            self.xz_stats = dec.last_stats()
            meta, status = self.chunk_meta(buf, sum(totals), off, size, expect)
        finally:
            dec.free(buf)
        return build_report(bundle_first, meta, status, self.chunk_max_size)

    def last_stats(self):
        """Device times (ms) of the last call's two hashing kernels and the
        whole call's wall clock (zc_meta_last_stats); call_ms: the same seen
        from Python."""
        d = [ctypes.c_double() for _ in range(3)]
        rc = self._L.zc_meta_last_stats(self._ctx, *[ctypes.byref(x) for x in d])
        _check(self._L, self._ctx, rc, "zc_meta_last_stats")
        return {"meta_ms": d[0].value, "sha1_ms": d[1].value, "total_ms": d[2].value, "call_ms": self._call_ms}

    def close(self):
        if self._ctx:
            self._L.zc_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sidecar_bytes(meta):
    """The ZCMETA01 file of a META_DTYPE array: magic, LE32 record size, LE32 0,
    LE64 count, the records, the SHA-256 of everything before it."""
    meta = np.ascontiguousarray(meta, dtype=META_DTYPE)
    body = SIDECAR_MAGIC + struct.pack("<IIQ", META_DTYPE.itemsize, 0, len(meta)) + meta.tobytes()
    return body + hashlib.sha256(body).digest()


def write_sidecar(directory, meta):
    """One new chunk-metadata file of `directory` (made if missing), named by
    its trailing SHA-256, written under a temporary name and renamed; returns
    its path, or None when there is nothing to write."""
    if not len(meta):
        return None
    data = sidecar_bytes(meta)
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, data[-32:].hex())
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(data)
            f.flush()
            os.fsync(f.fileno())
        os.rename(tmp, path)
    except OSError:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return path


def read_sidecar(path):
    """The records of one chunk-metadata file; ZcError when it is not a valid one."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 24 + 32 or data[:8] != SIDECAR_MAGIC:
        raise _lib.ZcError(f"{path}: not a chunk-metadata file")
    rec_size, _, count = struct.unpack("<IIQ", data[8:24])
    if rec_size != META_DTYPE.itemsize or len(data) != 24 + count * rec_size + 32:
        raise _lib.ZcError(f"{path}: {count} records of {rec_size} bytes do not fill {len(data)} bytes")
    if hashlib.sha256(data[:-32]).digest() != data[-32:]:
        raise _lib.ZcError(f"{path}: checksum mismatch")
    return np.frombuffer(data[24:-32], dtype=META_DTYPE).copy()
