"""Index files: a repository's chunk records from the files on disk -- the host
mirror of ChunkIndex::loadIndex.

  IndexFile::Reader (index_file.cc:44-76)   -> IndexLoader.load         zc_index_load_host
  Bundle::Reader's BundleInfo (bundle.cc)   -> IndexLoader.bundle_infos zc_bundle_info_parse_host
  IndexFile::Writer (index_file.cc:18-42)   -> write_index              zc_index_serialize + CBC encrypt

`IndexLoader.load` takes the files' bytes and returns an `IndexSet` whose numpy
views carry the names of zc_gc_input's fields, so `Collector.plan_index` can
plan a garbage collection straight from the files; `bundle_infos` does the same
for the BundleInfo bodies of unsealed bundle files and returns what
`Restorer.plan` and `Adopter.adopt` take.  Decrypting, checking and parsing all
run on the GPU (include/zchunk.h has the format and the status codes).  There
is no CPU fallback.
"""
import collections.abc
import ctypes
import struct
import time
import zlib

import numpy as np

from . import _lib
from .bundle import BundleCompressor, _host_check, _key16
from .chunker import _check


def _blobs(a, what):
    blobs = [bytes(b) for b in a]
    if any(len(b) != 24 for b in blobs):
        raise _lib.ZcError(f"{what} is 24 bytes")
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(len(blobs), 24)


class IndexSet:
    """The records of a set of index files: `ids` (n x 24), `sizes`,
    `bundle_first`, `bundle_ids` (B x 24), `index_first` -- zc_gc_input's
    fields -- and one `status` per file (ZC_INDEX_*; `status_names` spells them
    out).  A file whose status is not 0 contributes nothing."""
    __slots__ = ("ids", "sizes", "bundle_first", "bundle_ids", "index_first", "status")

    @property
    def status_names(self):
        return [_lib.INDEX_STATUS_NAMES.get(int(s), str(int(s))) for s in self.status]

    def bundles(self, i=None):
        """[(bundle id, [(chunk id, size), ...]), ...] of file i (None: one
        such list per file): the shape Collector.plan takes."""
        if i is None:
            return [self.bundles(k) for k in range(len(self.status))]
        out = []
        for b in range(int(self.index_first[i]), int(self.index_first[i + 1])):
            r0, r1 = int(self.bundle_first[b]), int(self.bundle_first[b + 1])
            out.append((self.bundle_ids[b].tobytes(),
                        [(self.ids[r].tobytes(), int(self.sizes[r])) for r in range(r0, r1)]))
        return out


class BundleInfos(collections.abc.Sequence):
    """The records of n BundleInfo bodies: `ids`, `sizes`, `bundle_first` and
    one `status` per bundle; as a sequence, bundle b is [(chunk id blob, size),
    ...] -- what Restorer.plan, IndexedRestorer and Adopter.adopt take."""

    def __init__(self, ids, sizes, bundle_first, status):
        self.ids, self.sizes, self.bundle_first, self.status = ids, sizes, bundle_first, status

    def __len__(self):
        return len(self.status)

    def __getitem__(self, b):
        if isinstance(b, slice):
            return [self[k] for k in range(*b.indices(len(self)))]
        if b < 0:
            b += len(self)
        if not 0 <= b < len(self):
            raise IndexError(b)
        r0, r1 = int(self.bundle_first[b]), int(self.bundle_first[b + 1])
        return [(self.ids[r].tobytes(), int(self.sizes[r])) for r in range(r0, r1)]


class IndexLoader:
    """zc_index_load / zc_bundle_info_parse on a context of its own, or on
    another object's (`ctx=comp._ctx`); key: the repository's 16-byte AES key,
    None for an unencrypted one."""

    def __init__(self, device=0, ctx=None, key=None):
        self._comp = BundleCompressor(device=device, ctx=ctx)
        self._L, self._ctx = self._comp._L, self._comp._ctx
        self._key = _key16(key, none_ok=True)
        self._call_ms = 0.0

    @staticmethod
    def _pack(files):
        """The files back to back at 16-byte aligned offsets."""
        files = [bytes(f) for f in files]
        size = np.array([len(f) for f in files], dtype=np.uint64)
        cap = (size + np.uint64(15)) // np.uint64(16) * np.uint64(16)
        off = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64) if len(files) else size
        src = np.zeros(int(cap.sum()) or 16, dtype=np.uint8)
        for o, f in zip(off, files):
            src[int(o):int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return src, off, size

    def _fetch_arrays(self, handle):
        nf, nb, nr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _host_check(self._L, self._L.zc_index_set_counts(handle, ctypes.byref(nf), ctypes.byref(nb),
                                                         ctypes.byref(nr)), "zc_index_set_counts")
        s = IndexSet()
        s.ids = np.zeros((nr.value, 24), dtype=np.uint8)
        s.sizes = np.zeros(nr.value, dtype=np.uint32)
        s.bundle_first = np.zeros(nb.value + 1, dtype=np.uint64)
        s.bundle_ids = np.zeros((nb.value, 24), dtype=np.uint8)
        s.index_first = np.zeros(nf.value + 1, dtype=np.uint64)
        s.status = np.zeros(nf.value, dtype=np.int32)
        rc = self._L.zc_index_set_fetch(handle, s.ids.ctypes.data, s.sizes.ctypes.data,
                                        s.bundle_first.ctypes.data, s.bundle_ids.ctypes.data,
                                        s.index_first.ctypes.data, s.status.ctypes.data)
        _host_check(self._L, rc, "zc_index_set_fetch")
        return s

    def _fetch(self, handle):
        try:
            return self._fetch_arrays(handle)
        finally:
            self._L.zc_index_set_destroy(handle)

    def load_resident(self, files):
        """load() without the host trip: returns a ResidentIndexSet, which
        keeps the zc_index_set -- the records in HBM -- alive until it is
        closed.  ChunkIndex.from_index_set builds on it."""
        src, off, size = self._pack(files)
        handle = ctypes.c_void_p()
        t = time.perf_counter()
        rc = self._L.zc_index_load_host(self._ctx, self._key, src.ctypes.data, off.ctypes.data, size.ctypes.data,
                                        len(size), ctypes.byref(handle))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, "zc_index_load_host")
        return ResidentIndexSet(self, handle)

    def load_resident_device(self, d_files, file_off, file_size):
        """load_device() without the host trip (see load_resident)."""
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        size = np.ascontiguousarray(file_size, dtype=np.uint64)
        if len(off) != len(size):
            raise _lib.ZcError("zc_index_load: file_off and file_size differ in length")
        handle = ctypes.c_void_p()
        t = time.perf_counter()
        rc = self._L.zc_index_load(self._ctx, self._key, ctypes.c_void_p(d_files), off.ctypes.data, size.ctypes.data,
                                   len(size), ctypes.byref(handle))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, "zc_index_load")
        return ResidentIndexSet(self, handle)

    def load(self, files):
        """files: the index files' bytes, in the order their records are to
        appear.  Returns an IndexSet; a bad file gets a status, not an error."""
        src, off, size = self._pack(files)
        handle = ctypes.c_void_p()
        t = time.perf_counter()
        rc = self._L.zc_index_load_host(self._ctx, self._key, src.ctypes.data, off.ctypes.data, size.ctypes.data,
                                        len(size), ctypes.byref(handle))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, "zc_index_load_host")
        return self._fetch(handle)

    def load_device(self, d_files, file_off, file_size):
        """The same for files already in device memory: file i is
        d_files[file_off[i] ..+ file_size[i]) (16-byte aligned with a key)."""
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        size = np.ascontiguousarray(file_size, dtype=np.uint64)
        if len(off) != len(size):
            raise _lib.ZcError("zc_index_load: file_off and file_size differ in length")
        handle = ctypes.c_void_p()
        t = time.perf_counter()
        rc = self._L.zc_index_load(self._ctx, self._key, ctypes.c_void_p(d_files), off.ctypes.data, size.ctypes.data,
                                   len(size), ctypes.byref(handle))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, "zc_index_load")
        return self._fetch(handle)

    def bundle_infos(self, layouts, plain):
        """The records of unsealed bundle files: `layouts` is what
        BundleCompressor.unseal returned (LAYOUT_DTYPE; only info_off /
        info_len are read, offsets into `plain`, so add each bundle's plain_off
        first when they share a buffer) or a list of (info_off, info_len);
        `plain` the host bytes they index.  Returns a BundleInfos."""
        if isinstance(layouts, np.ndarray) and layouts.dtype.names:
            off, length = layouts["info_off"], layouts["info_len"]
        else:
            off, length = [a for a, _ in layouts], [b for _, b in layouts]
        buf = np.ascontiguousarray(np.frombuffer(memoryview(plain), dtype=np.uint8))
        keep = buf if buf.size else np.zeros(1, dtype=np.uint8)
        off, length = np.asarray(off, dtype=np.uint64), np.asarray(length, dtype=np.uint64)
        if len(off) and int((off + length).max()) > buf.size:
            raise _lib.ZcError("zc_bundle_info_parse_host: a BundleInfo ends past the plaintext")
        return self._infos(self._L.zc_bundle_info_parse_host, "zc_bundle_info_parse_host", keep.ctypes.data, off,
                           length)

    def bundle_infos_device(self, d_plain, info_off, info_len):
        """The same for plaintexts in device memory (zc_bundle_unseal's
        d_plain): bundle i's BundleInfo is d_plain[info_off[i] ..+ info_len[i])."""
        return self._infos(self._L.zc_bundle_info_parse, "zc_bundle_info_parse", ctypes.c_void_p(d_plain), info_off,
                           info_len)

    def _infos(self, fn, what, plain, off, length):
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        if len(off) != len(length):
            raise _lib.ZcError(f"{what}: info_off and info_len differ in length")
        n = len(off)
        cap = int((length // np.uint64(30)).sum())  # a record takes at least 30 bytes
        ids, sizes = np.zeros((max(cap, 1), 24), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint32)
        first, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
        nrec = ctypes.c_uint64()
        t = time.perf_counter()
        rc = fn(self._ctx, plain, off.ctypes.data, length.ctypes.data, n, ids.ctypes.data, sizes.ctypes.data, cap,
                first.ctypes.data, status.ctypes.data, ctypes.byref(nrec))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, what)
        return BundleInfos(ids[:nrec.value].copy(), sizes[:nrec.value].copy(), first, status[:n])

    def last_stats(self):
        """Stream times (ms) of the last call's decrypt, Adler-32, frame and
        record passes and the call's wall clock (zc_index_last_stats);
        call_ms: the same seen from here."""
        d = [ctypes.c_double() for _ in range(5)]
        rc = self._L.zc_index_last_stats(self._ctx, *[ctypes.byref(x) for x in d])
        _check(self._L, self._ctx, rc, "zc_index_last_stats")
        out = {k: v.value for k, v in zip(("decrypt_ms", "adler_ms", "frame_ms", "records_ms", "total_ms"), d)}
        out["call_ms"] = self._call_ms
        return out

    def close(self):
        self._comp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ResidentIndexSet:
    """A live zc_index_set: the records of a set of index files, kept in HBM
    (IndexLoader.load_resident).  `n_files`, `n_bundles`, `n_records`;
    `fetch()` copies the arrays out as an IndexSet; `close()` frees them."""

    def __init__(self, loader, handle):
        self._loader, self._L, self._handle = loader, loader._L, handle
        nf, nb, nr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _host_check(self._L, self._L.zc_index_set_counts(handle, ctypes.byref(nf), ctypes.byref(nb),
                                                         ctypes.byref(nr)), "zc_index_set_counts")
        self.n_files, self.n_bundles, self.n_records = nf.value, nb.value, nr.value

    def fetch(self):
        if self._handle is None:
            raise _lib.ZcError("ResidentIndexSet: closed")
        return self._loader._fetch_arrays(self._handle)

    def close(self):
        if self._handle is not None:
            self._L.zc_index_set_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ResolvedStream:
    """zc_restore_resolve's plan on the host: the counts (`n_entries`,
    `n_used`, `length`, `n_missing`, `first_missing`, `n_dup_used`,
    `first_dup`), `used` / `used_size` per used bundle (ascending bundle
    number), and per entry `slot`, `off`, `size`, `dst`.  Slot k is bundle
    used[k], slot n_used the instruction stream, ZC_NO_BUNDLE a missing id."""
    COUNTS = ("n_entries", "n_used", "length", "n_missing", "first_missing", "n_dup_used", "first_dup")
    __slots__ = COUNTS + ("used", "used_size", "slot", "off", "size", "dst")


class ChunkIndex:
    """A zc_chunk_index: ChunkIndex::findChunk for a whole repository in HBM.
    The owner of an id is its first registration in loadIndex order; a bundle
    that holds an id twice is flagged.  Made from a live set
    (`from_index_set`), from arrays in zc_gc_input's layout (`from_arrays`) or
    from bundles' record lists (`from_bundles`: a BundleInfos, or
    [[(chunk id, size), ...], ...]); on a context of its own, or on another
    object's (`ctx=comp._ctx`)."""

    def __init__(self, device=0, ctx=None):
        self._comp = BundleCompressor(device=device, ctx=ctx)
        self._L, self._ctx = self._comp._L, self._comp._ctx
        self._idx = None

    @classmethod
    def from_index_set(cls, resident, device=0, ctx=None):
        if not isinstance(resident, ResidentIndexSet) or resident._handle is None:
            raise _lib.ZcError("ChunkIndex.from_index_set takes a live ResidentIndexSet (IndexLoader.load_resident)")
        self = cls(device=device, ctx=ctx if ctx is not None else resident._loader._ctx)
        try:
            idx = ctypes.c_void_p()
            rc = self._L.zc_chunk_index_create(self._ctx, resident._handle, ctypes.byref(idx))
            _check(self._L, self._ctx, rc, "zc_chunk_index_create")
            self._idx = idx
        except Exception:
            self.close()
            raise
        return self

    @classmethod
    def from_arrays(cls, ids, sizes, bundle_first, device=0, ctx=None):
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 24)
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        bundle_first = np.ascontiguousarray(bundle_first, dtype=np.uint64)
        if len(ids) != len(sizes) or len(bundle_first) < 1:
            raise _lib.ZcError("ChunkIndex.from_arrays: ids and sizes differ in length, or bundle_first is empty")
        self = cls(device=device, ctx=ctx)
        try:
            idx = ctypes.c_void_p()
            rc = self._L.zc_chunk_index_create_arrays(self._ctx, ids.ctypes.data if len(ids) else None,
                                                      sizes.ctypes.data if len(ids) else None, len(ids),
                                                      bundle_first.ctypes.data, len(bundle_first) - 1,
                                                      ctypes.byref(idx))
            _check(self._L, self._ctx, rc, "zc_chunk_index_create_arrays")
            self._idx = idx
        except Exception:
            self.close()
            raise
        return self

    @classmethod
    def from_bundles(cls, bundles, device=0, ctx=None):
        if isinstance(bundles, BundleInfos):
            return cls.from_arrays(bundles.ids, bundles.sizes, bundles.bundle_first, device=device, ctx=ctx)
        recs = [r for rs in bundles for r in rs]
        ids = _blobs([c for c, _ in recs], "a chunk id")
        sizes = np.array([int(s) for _, s in recs], dtype=np.uint32)
        first = np.concatenate([[0], np.cumsum([len(rs) for rs in bundles])]).astype(np.uint64)
        return cls.from_arrays(ids, sizes, first, device=device, ctx=ctx)

    def _live(self):
        if self._idx is None:
            raise _lib.ZcError("ChunkIndex: closed")
        return self._idx

    def counts(self):
        """{records, bundles, ids (distinct), flagged (bundles holding an id twice)}"""
        c = [ctypes.c_uint64() for _ in range(4)]
        _host_check(self._L, self._L.zc_chunk_index_counts(self._live(), *[ctypes.byref(x) for x in c]),
                    "zc_chunk_index_counts")
        return dict(zip(("records", "bundles", "ids", "flagged"), (x.value for x in c)))

    def bundles(self):
        """(payload size of every bundle, uint64; whether it holds an id twice, bool)"""
        nb = self.counts()["bundles"]
        size, dup = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint8)
        rc = self._L.zc_chunk_index_bundles(self._live(), size.ctypes.data if nb else None,
                                            dup.ctypes.data if nb else None)
        _host_check(self._L, rc, "zc_chunk_index_bundles")
        return size, dup.astype(bool)

    def lookup(self, ids):
        """Batch findChunk: (bundle, off, size) arrays for ids (n x 24 array or
        a list of 24-byte blobs); bundle ZC_NO_BUNDLE where the index has no such id."""
        if not isinstance(ids, np.ndarray):
            ids = _blobs(ids, "a chunk id")
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 24)
        n = len(ids)
        bundle, off = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        size = np.zeros(n, dtype=np.uint32)
        rc = self._L.zc_chunk_index_lookup(self._ctx, self._live(), ids.ctypes.data if n else None, n,
                                           bundle.ctypes.data if n else None, off.ctypes.data if n else None,
                                           size.ctypes.data if n else None)
        _check(self._L, self._ctx, rc, "zc_chunk_index_lookup")
        return bundle, off, size

    def resolve(self, ins, instr_bytes):
        """zc_restore_resolve over parse_backup_data's array; returns a
        ResolvedStream.  A missing id or a flagged used bundle is reported in
        its counts, not raised (Restorer.plan_index raises)."""
        from .bundle import INSTRUCTION_DTYPE
        ins = np.ascontiguousarray(ins, dtype=INSTRUCTION_DTYPE)
        n = len(ins)
        plan = ctypes.c_void_p()
        rc = self._L.zc_restore_resolve(self._ctx, self._live(), ins.ctypes.data if n else None, n,
                                        int(instr_bytes), ctypes.byref(plan))
        _check(self._L, self._ctx, rc, "zc_restore_resolve")
        try:
            c = [ctypes.c_uint64() for _ in ResolvedStream.COUNTS]
            _host_check(self._L, self._L.zc_restore_plan_counts(plan, *[ctypes.byref(x) for x in c]),
                        "zc_restore_plan_counts")
            r = ResolvedStream()
            for name, x in zip(ResolvedStream.COUNTS, c):
                setattr(r, name, x.value)
            r.used, r.used_size = np.zeros(r.n_used, dtype=np.uint32), np.zeros(r.n_used, dtype=np.uint64)
            r.slot = np.zeros(n, dtype=np.uint32)
            r.off, r.size, r.dst = (np.zeros(n, dtype=np.uint64) for _ in range(3))
            rc = self._L.zc_restore_plan_fetch(plan, *[a.ctypes.data if len(a) else None
                                                       for a in (r.used, r.used_size, r.slot, r.off, r.size, r.dst)])
            _host_check(self._L, rc, "zc_restore_plan_fetch")
            return r
        finally:
            self._L.zc_restore_plan_destroy(plan)

    def last_stats(self):
        """{build_ms, resolve_ms, table_slots, max_probe} of the context's
        last build and last resolve or lookup (zc_resolve_last_stats)."""
        b, r, slots, probe = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.zc_resolve_last_stats(self._ctx, ctypes.byref(b), ctypes.byref(r), ctypes.byref(slots),
                                           ctypes.byref(probe))
        _check(self._L, self._ctx, rc, "zc_resolve_last_stats")
        return {"build_ms": b.value, "resolve_ms": r.value, "table_slots": slots.value, "max_probe": probe.value}

    def close(self):
        if self._idx is not None:
            self._L.zc_chunk_index_destroy(self._idx)
            self._idx = None
        if self._comp is not None:
            self._comp.close()
            self._comp = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def serialize_index(bundles):
    """The plaintext between R and the Adler-32 (zc_index_serialize) for
    bundles = [(bundle id, [(chunk id, size), ...]), ...]."""
    bids = _blobs([b for b, _ in bundles], "a bundle id")
    recs = [r for _, rs in bundles for r in rs]
    ids = _blobs([c for c, _ in recs], "a chunk id")
    sizes = np.array([int(s) for _, s in recs], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(rs) for _, rs in bundles])]).astype(np.uint64)
    return serialize_index_arrays(ids, sizes, first, bids)


def serialize_index_arrays(ids, sizes, bundle_first, bundle_ids):
    L = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    bundle_ids = np.ascontiguousarray(bundle_ids, dtype=np.uint8)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    bundle_first = np.ascontiguousarray(bundle_first, dtype=np.uint64)
    nb = len(bundle_first) - 1
    need = ctypes.c_uint64()
    L.zc_index_serialize(ids.ctypes.data, sizes.ctypes.data, bundle_first.ctypes.data, bundle_ids.ctypes.data, nb,
                         None, 0, ctypes.byref(need))
    out = np.zeros(max(need.value, 1), dtype=np.uint8)
    rc = L.zc_index_serialize(ids.ctypes.data, sizes.ctypes.data, bundle_first.ctypes.data, bundle_ids.ctypes.data,
                              nb, out.ctypes.data, len(out), ctypes.byref(need))
    _host_check(L, rc, "zc_index_serialize")
    return out[:need.value].tobytes()


def index_file_size(body_len, keyed):
    return int(_lib.load().zc_index_file_size(int(body_len), 1 if keyed else 0))


def write_index(bundles, key=None, r=None, comp=None):
    """IndexFile::Writer's whole file for bundles = [(bundle id, [(chunk id,
    size), ...]), ...]: zc_index_serialize, then R, the Adler-32 and the
    padding here, then the CBC encrypt on the GPU (key None: no R, no padding,
    no cipher).  The caller draws the 16 random bytes `r`, as for
    BundleCompressor.seal; comp: a BundleCompressor to encrypt on."""
    body = serialize_index(bundles)
    key = _key16(key, none_ok=True)
    if key is None:
        return body + struct.pack("<I", zlib.adler32(body))
    if r is None or len(bytes(r)) != 16:
        raise ValueError("write_index: with a key, r is the file's 16 random bytes")
    p = bytes(r) + body
    p += struct.pack("<I", zlib.adler32(p))
    n = 16 - len(p) % 16
    p += bytes([n]) * n
    assert len(p) == index_file_size(len(body), True)
    own = comp is None
    comp = comp or BundleCompressor()
    try:
        src = np.frombuffer(p, dtype=np.uint8)
        out = np.zeros(len(p), dtype=np.uint8)
        z, ln = np.zeros(1, dtype=np.uint64), np.array([len(p)], dtype=np.uint64)
        rc = comp._L.zc_aes128_cbc_encrypt_host(comp._ctx, key, src.ctypes.data, z.ctypes.data, ln.ctypes.data, 1,
                                                None, out.ctypes.data, z.ctypes.data)
        _check(comp._L, comp._ctx, rc, "zc_aes128_cbc_encrypt_host")
        return out.tobytes()
    finally:
        if own:
            comp.close()
