"""Garbage collection: which chunks the backups use, which bundles go, what is
repacked where -- the host mirror of `zbackup gc`.

  ZCollector::gc                 -> Collector.mark per backup, then plan   zutils.cc:450-505
  BundleCollector::processChunk  -> the id table on the GPU               backup_collector.cc:51-67
  BundleCollector::finishBundle  -> GcPlan.bundle_action                  backup_collector.cc:69-127
  BundleCollector::copyUsedChunks -> GcPlan.copy, Collector.repack        backup_collector.cc:129-144

`Collector.plan` runs zc_gc_plan (include/zchunk.h has the semantics line by
line); `Collector.repack` assembles every new bundle's payload on the device
with zc_bundle_gather from the decoded payloads of the bundles being repacked.
Decoding those (liblzo2's lzo1x_decompress_safe) is the caller's step between
the two, exactly as for `Restorer`; compressing and sealing the new payloads is
`BundleCompressor.compress` / `.seal`.  There is no CPU fallback.
"""
import ctypes
import time

import numpy as np

from . import _lib
from .bundle import MAX_PAYLOAD_SIZE, BundleCompressor, parse_backup_data
from .chunker import _check

GC_INDEX_DTYPE = np.dtype([("total", "<u8"), ("used", "<u8"), ("kept", "<u4"), ("modified_bundles", "<u4"),
                           ("removed", "<u4"), ("modified", "u1"), ("necessary", "u1"), ("unlink", "u1"),
                           ("reserved", "u1")])
assert GC_INDEX_DTYPE.itemsize == ctypes.sizeof(_lib.ZcGcIndex)


def _ids(a):
    """n x 24 uint8, contiguous, from an array or a list of 24-byte blobs."""
    if isinstance(a, np.ndarray):
        out = np.ascontiguousarray(a, dtype=np.uint8)
    else:
        blobs = [bytes(b) for b in a]
        if any(len(b) != 24 for b in blobs):
            raise _lib.ZcError("a chunk id is 24 bytes (ChunkId::toBlob)")
        out = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    if out.size % 24:
        raise _lib.ZcError("a chunk id is 24 bytes (ChunkId::toBlob)")
    return out.reshape(out.size // 24, 24)


class GcPlan:
    """zc_gc_plan's outputs as numpy arrays (the names of zc_gc_output), with
    the inputs they index: `ids` / `sizes` per record, `bundle_first`,
    `bundle_ids`, `index_first`."""
    __slots__ = ("ids", "sizes", "bundle_first", "bundle_ids", "index_first", "record_flags", "bundle_total",
                 "bundle_used", "bundle_action", "indexes", "copy", "copy_bundle", "copy_off", "new_bundle_index",
                 "new_bundle_size")

    def files_to_unlink(self):
        """(bundle numbers, index file numbers) the collection unlinks: the
        REMOVE and REPACK bundles' files, the index files finishIndex drops."""
        act = self.bundle_action
        bundles = np.nonzero((act == _lib.ZC_GC_ACT_REMOVE) | (act == _lib.ZC_GC_ACT_REPACK))[0]
        return bundles.tolist(), np.nonzero(self.indexes["unlink"])[0].tolist()


class Collector:
    """`zbackup gc` over a repository's index files on the GPU."""

    def __init__(self, device=0, ctx=None):
        self._comp = BundleCompressor(device=device, ctx=ctx)
        self._L, self._ctx = self._comp._L, self._comp._ctx
        self._used = []
        self._call_ms = 0.0

    def mark(self, backup_data):
        """Adds the chunk_to_emit ids of one BackupInstruction stream
        (restore() with a usedChunkSet, backup_restorer.cc:59-70)."""
        ins = parse_backup_data(backup_data)
        self.mark_ids(ins["id"][ins["kind"] == _lib.ZC_INSTR_CHUNK])

    def mark_ids(self, ids):
        ids = _ids(ids)
        if len(ids):
            self._used.append(ids)

    def used_ids(self):
        if len(self._used) > 1:
            self._used = [np.concatenate(self._used)]
        return self._used[0] if self._used else np.zeros((0, 24), dtype=np.uint8)

    def plan(self, indexes, deep=False, repack=False, concat=False, max_payload=MAX_PAYLOAD_SIZE):
        """indexes[i] = [(bundle id, [(chunk id blob, size), ...]), ...]: the
        index files as read, bundle by bundle."""
        ids, sizes, bundle_ids, bundle_first, index_first = [], [], [], [0], [0]
        for bundles in indexes:
            for bundle_id, records in bundles:
                bundle_ids.append(bytes(bundle_id))
                for cid, size in records:
                    ids.append(bytes(cid))
                    sizes.append(int(size))
                bundle_first.append(len(ids))
            index_first.append(len(bundle_ids))
        return self.plan_arrays(_ids(ids), sizes, bundle_first, _ids(bundle_ids), index_first, deep=deep,
                                repack=repack, concat=concat, max_payload=max_payload)

    def plan_index(self, index_set, **kw):
        """The same from an IndexSet (IndexLoader.load): the records of the
        index files as read from disk.  Files whose status is not 0 contribute
        nothing, so the caller decides first whether to go on without them."""
        return self.plan_arrays(index_set.ids, index_set.sizes, index_set.bundle_first, index_set.bundle_ids,
                                index_set.index_first, **kw)

    def plan_arrays(self, ids, sizes, bundle_first, bundle_ids, index_first, deep=False, repack=False, concat=False,
                    max_payload=MAX_PAYLOAD_SIZE, copy_cap=None):
        """The same over flat arrays (zc_gc_input's fields)."""
        p = GcPlan()
        p.ids, p.bundle_ids = _ids(ids), _ids(bundle_ids)
        p.sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        p.bundle_first = np.ascontiguousarray(bundle_first, dtype=np.uint64)
        p.index_first = np.ascontiguousarray(index_first, dtype=np.uint64)
        used = self.used_ids()
        N, B, I = len(p.ids), len(p.bundle_ids), len(p.index_first) - 1
        if len(p.sizes) != N or len(p.bundle_first) != B + 1 or I < 0:
            raise _lib.ZcError("gc: ids, sizes, bundle_first and bundle_ids differ in length")
        cap = N if copy_cap is None else int(copy_cap)
        # Writer::add may finish an empty bundle before a chunk over max_payload: two per entry at most
        nb_cap = 2 * cap + I
        p.record_flags = np.zeros(N, dtype=np.uint8)
        p.bundle_total, p.bundle_used = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        p.bundle_action = np.zeros(B, dtype=np.uint8)
        p.indexes = np.zeros(I, dtype=GC_INDEX_DTYPE)
        copy, copy_bundle = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        copy_off = np.zeros(cap, dtype=np.uint64)
        nb_index, nb_size = np.zeros(nb_cap, dtype=np.uint32), np.zeros(nb_cap, dtype=np.uint64)
        flags = (_lib.ZC_GC_DEEP if deep else 0) | (_lib.ZC_GC_REPACK if repack else 0) | \
            (_lib.ZC_GC_CONCAT if concat else 0)
        gin = _lib.ZcGcInput(p.ids.ctypes.data, p.sizes.ctypes.data, N, p.bundle_first.ctypes.data,
                             p.bundle_ids.ctypes.data, B, p.index_first.ctypes.data, I, used.ctypes.data, len(used),
                             flags, 0, int(max_payload))
        out = _lib.ZcGcOutput(p.record_flags.ctypes.data, p.bundle_total.ctypes.data, p.bundle_used.ctypes.data,
                              p.bundle_action.ctypes.data, p.indexes.ctypes.data, copy.ctypes.data,
                              copy_bundle.ctypes.data, copy_off.ctypes.data, cap, 0, nb_index.ctypes.data,
                              nb_size.ctypes.data, nb_cap, 0)
        t = time.perf_counter()
        rc = self._L.zc_gc_plan(self._ctx, ctypes.byref(gin), ctypes.byref(out))
        self._call_ms = (time.perf_counter() - t) * 1e3
        _check(self._L, self._ctx, rc, "zc_gc_plan")
        m, nb = int(out.n_copy), int(out.n_new_bundles)
        p.copy, p.copy_bundle, p.copy_off = copy[:m].copy(), copy_bundle[:m].copy(), copy_off[:m].copy()
        p.new_bundle_index, p.new_bundle_size = nb_index[:nb].copy(), nb_size[:nb].copy()
        return p

    def last_stats(self):
        """Device and host times (ms) of the last plan, the table's slots and
        the longest probe run (zc_gc_last_stats, zc_gc_last_times); call_ms:
        the whole zc_gc_plan call, wall clock."""
        d = [ctypes.c_double() for _ in range(6)]
        slots, probe = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.zc_gc_last_stats(self._ctx, ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(slots),
                                      ctypes.byref(probe))
        _check(self._L, self._ctx, rc, "zc_gc_last_stats")
        rc = self._L.zc_gc_last_times(self._ctx, *[ctypes.byref(x) for x in d[2:]])
        _check(self._L, self._ctx, rc, "zc_gc_last_times")
        names = ("build_ms", "probe_ms", "upload_ms", "host_ms", "copy_ms", "readback_ms")
        out = {k: v.value for k, v in zip(names, d)}
        out.update(table_slots=slots.value, max_probe=probe.value, call_ms=self._call_ms)
        return out

    def repack(self, plan, d_work, pay_off, d_payloads):
        """copyUsedChunks for every REPACK bundle: the decoded payload of
        bundle b lies at d_work + pay_off[b] (pay_off: one entry per bundle, or
        a dict; only the REPACK bundles' are read).  Every new bundle's payload
        is assembled at d_payloads, back to back in copy order, by one
        zc_bundle_gather.  Returns (new_bundles, new_pay_off, new_pay_size):
        new_bundles[j] = [(chunk id blob, size), ...] of new bundle j (its
        BundleInfo), whose payload is d_payloads[new_pay_off[j] ..+
        new_pay_size[j])."""
        rec = plan.copy.astype(np.int64)
        sizes = plan.sizes.astype(np.uint64)
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)  # payload bytes before each record
        bundle = np.searchsorted(plan.bundle_first, rec, side="right") - 1
        if len(rec) and not (plan.bundle_action[bundle] == _lib.ZC_GC_ACT_REPACK).all():
            raise _lib.ZcError("gc: the copy list names a bundle that is not repacked")
        base = np.array([int(pay_off[int(b)]) for b in bundle], dtype=np.uint64)
        src_off = base + start[rec] - start[plan.bundle_first[bundle].astype(np.int64)]
        if len(rec):
            self._comp.gather(d_work, src_off, sizes[rec], d_payloads)
        new_size = plan.new_bundle_size.astype(np.uint64)
        new_off = np.concatenate([[0], np.cumsum(new_size)[:-1]]).astype(np.uint64) if len(new_size) else new_size
        new_bundles = [[] for _ in range(len(new_size))]
        for r, j in zip(rec, plan.copy_bundle):
            new_bundles[int(j)].append((plan.ids[r].tobytes(), int(plan.sizes[r])))
        return new_bundles, new_off, new_size

    def close(self):
        self._comp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
