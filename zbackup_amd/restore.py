"""Restore: replaying a BackupInstruction stream over decoded bundles on the GPU.

  restore()                  -> instruction replay        backup_restorer.cc:38-107
  Bundle::Reader::Reader     -> id -> chunk map           bundle.cc:220-232
  Bundle::Reader::get        -> the chunk's bytes         bundle.cc:235-251

`Restorer.plan` is host bookkeeping: the parse (zc_parse_instructions), the id
map, which bundles the stream references and where their decoded payloads go in
one scratch buffer, and one scatter list over both the chunk extents and the
bytes_to_emit runs.  `Restorer.replay` runs that list in one zc_bundle_scatter
call, HBM to HBM.  Decoding the referenced bundles' lzo1x streams into the
scratch buffer is the caller's step between the two (liblzo2's
lzo1x_decompress_safe, as the reference calls it, compression.cc:472-490;
`bundle.frame_info` reads the frame): the instruction stream travels to the
device in the same buffer, so there is one upload (`RestorePlan.host_image`;
`RestorePlan.instruction_image` is the instruction stream's share of it alone).
LZMA bundles, zbackup's default, need no host decoder: `Restorer.replay_bodies`
takes their xz bodies and decodes them into the scratch buffer on the device
(zc_xz_decode), as `IndexedRestorer.decode_payload` does for one slot.

  IndexedRestorer::saveData  -> any byte range            backup_restorer.cc:182-316

`IndexedRestorer` serves batches of (offset, size) reads from the payloads that
are resident at the time (zc_range_read): the same plan, kept as a
`RangeIndex` of (position, slot, offset) entries in HBM, one slot per
referenced bundle and one for the instruction stream.
"""
import ctypes

import numpy as np

from . import _lib
from .bundle import BundleCompressor, BundleDecompressor, _u64, parse_backup_data


def chunk_map(bundles):
    """id blob -> (bundle, offset in its payload, size), as Bundle::Reader::Reader
    builds it per bundle (bundle.cc:220-232): chunks lie back to back in the
    order of the bundle's BundleInfo.  `bundles[b]` = [(chunk id blob, size), ...].
    An id twice in one bundle is an error, as there; an id in two bundles
    keeps the first."""
    out = {}
    for b, chunks in enumerate(bundles):
        pos, seen = 0, set()
        for blob, size in chunks:
            blob = bytes(blob)
            if len(blob) != 24:
                raise _lib.ZcError(f"bundle {b}: a chunk id of {len(blob)} bytes")
            if blob in seen:
                raise _lib.ZcError(f"bundle {b}: chunk id {blob.hex()} twice in one bundle")
            seen.add(blob)
            out.setdefault(blob, (b, pos, int(size)))
            pos += int(size)
    return out


class RestorePlan:
    """What one restore does: `length` bytes out; the decoded payload of bundle
    `used[k]` (`pay_size[k]` bytes) belongs at `pay_off[k]` of a scratch buffer
    of `work_size` bytes, the instruction stream `data` at `instr_off`; the
    scatter list is src_off / sizes / dst_off."""
    __slots__ = ("data", "length", "used", "pay_off", "pay_size", "instr_off", "work_size", "src_off", "sizes",
                 "dst_off", "slot", "off")  # slot / off: plan_index's fetched arrays (RangeIndex's form)

    def host_image(self, payloads):
        """The scratch buffer's contents as one host array, for one upload:
        `payloads[k]` = the decoded payload of bundle `used[k]`."""
        img = np.zeros(max(self.work_size, 1), dtype=np.uint8)
        for k, p in enumerate(payloads):
            if len(p) != self.pay_size[k]:
                raise _lib.ZcError(f"restore: bundle {self.used[k]} decoded to {len(p)} bytes, its chunks take "
                                   f"{self.pay_size[k]}")
            img[self.pay_off[k]:self.pay_off[k] + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        img[self.instr_off:self.instr_off + len(self.data)] = np.frombuffer(self.data, dtype=np.uint8)
        return img


    def instruction_image(self):
        """(offset in the scratch buffer, the bytes that belong there): the
        instruction stream alone, whose bytes_to_emit runs the scatter list
        reads.  All of the scratch buffer that has to come from the host when
        the payloads are put at pay_off[k] on the device; host_image() is
        this plus the payloads."""
        return self.instr_off, np.frombuffer(self.data, dtype=np.uint8)

    def bodies_work_size(self, bodies):
        """The scratch buffer's size when the bundles' compressed bodies are
        decoded on the device (Restorer.replay_bodies): work_size plus the
        bodies, each 16-byte aligned."""
        return ((self.work_size + 15) & ~15) + BundleDecompressor.stage_size(bodies)


class Restorer:
    """Replays a BackupInstruction stream over decoded bundle payloads on the GPU."""

    def __init__(self, device=0, ctx=None):
        self._comp = BundleCompressor(device=device, ctx=ctx)

    @staticmethod
    def plan(backup_data, bundles):
        """Raises ZcError naming the id when the stream names a chunk no
        bundle holds (and on a malformed stream, or an id twice in a bundle)."""
        backup_data = bytes(backup_data)
        ins = parse_backup_data(backup_data)
        ids = chunk_map(bundles)
        p = RestorePlan()
        p.data = backup_data
        # the bundles the stream references, in first-use order, back to back (16-byte aligned)
        slot, p.used, p.pay_off, p.pay_size = {}, [], [], []
        pos = 0
        entries = []
        for e in ins:
            if e["kind"] == _lib.ZC_INSTR_CHUNK:
                blob = e["id"].tobytes()
                hit = ids.get(blob)
                if hit is None:
                    raise _lib.ZcError(f"restore: chunk id {blob.hex()} is in none of the {len(bundles)} bundles")
                b, off, size = hit
                if b not in slot:
                    slot[b] = len(p.used)
                    p.used.append(b)
                    p.pay_off.append(pos)
                    total = sum(int(s) for _, s in bundles[b])
                    p.pay_size.append(total)
                    pos += (total + 15) & ~15
                entries.append((p.pay_off[slot[b]] + off, size))
            else:
                entries.append((-1 - int(e["data_off"]), int(e["size"])))
        p.instr_off = pos
        p.work_size = pos + len(backup_data)
        p.src_off = np.array([s if s >= 0 else p.instr_off + (-1 - s) for s, _ in entries], dtype=np.uint64)
        p.sizes = np.array([n for _, n in entries], dtype=np.uint64)
        p.dst_off = (np.concatenate([[0], np.cumsum(p.sizes)[:-1]]).astype(np.uint64) if len(entries)
                     else np.zeros(0, dtype=np.uint64))
        p.length = int(p.sizes.sum())
        return p

    @staticmethod
    def plan_index(backup_data, chunk_index):
        """plan() against a resident ChunkIndex (zc_restore_resolve): the
        caller names no bundles, the index says which ones the stream needs.
        The fields mean what plan()'s mean, with `used` -- bundle numbers in
        the index's input order -- ascending, not in first-use order.  Raises
        ZcError naming the id when the index has no such chunk, and naming the
        bundle when a used bundle holds an id twice (exDuplicateChunks)."""
        backup_data = bytes(backup_data)
        ins = parse_backup_data(backup_data)
        r = chunk_index.resolve(ins, len(backup_data))
        if r.n_missing:
            blob = ins[r.first_missing]["id"].tobytes()
            raise _lib.ZcError(f"restore: chunk id {blob.hex()} is in none of the "
                               f"{chunk_index.counts()['bundles']} bundles ({r.n_missing} entries miss)")
        if r.n_dup_used:
            b = int(r.used[r.slot[r.first_dup]])
            raise _lib.ZcError(f"restore: bundle {b}: a chunk id twice in one bundle (entry {r.first_dup})")
        p = RestorePlan()
        p.data = backup_data
        p.used = [int(b) for b in r.used]
        p.pay_size = [int(s) for s in r.used_size]
        aligned = (r.used_size + np.uint64(15)) & ~np.uint64(15)
        ends = np.cumsum(aligned, dtype=np.uint64)
        p.pay_off = [0] + [int(x) for x in ends[:-1]] if r.n_used else []
        p.instr_off = int(ends[-1]) if r.n_used else 0
        p.work_size = p.instr_off + len(backup_data)
        base = np.array(p.pay_off + [p.instr_off], dtype=np.uint64)
        p.slot, p.off = r.slot, r.off
        p.src_off = base[r.slot] + r.off
        p.sizes = r.size
        p.dst_off = r.dst
        p.length = r.length
        return p

    def replay(self, plan, d_work, d_out, out_cap):
        """d_work: the device copy of the plan's scratch buffer (see
        RestorePlan.host_image).  Writes the restored stream to d_out (room
        out_cap) in one scatter call and returns its length."""
        if plan.length > out_cap:
            raise _lib.ZcError(f"restore: {plan.length} bytes to restore, room for {out_cap}")
        keep = plan.sizes > 0
        if keep.any():
            self._comp.scatter(d_work, plan.src_off[keep], plan.sizes[keep], d_out, plan.dst_off[keep])
        return plan.length

    def replay_bodies(self, plan, bodies, d_work, d_out, out_cap):
        """The same from LZMA bundles as they lie on disk: bodies[k] = the xz
        stream of bundle plan.used[k] (zc_bundle_unseal's body).  The
        instruction stream and the compressed bodies go to d_work (device
        memory of plan.bodies_work_size(bodies) bytes), body k is decoded on
        the device to d_work + plan.pay_off[k] (zc_xz_decode; a stream that is
        not exactly its payload raises ZcError naming the bundle), then
        replay().  The decoded payloads never touch the host."""
        if len(bodies) != len(plan.used):
            raise _lib.ZcError(f"restore: {len(bodies)} bodies for {len(plan.used)} referenced bundles")
        if plan.length > out_cap:
            raise _lib.ZcError(f"restore: {plan.length} bytes to restore, room for {out_cap}")
        dec = BundleDecompressor(ctx=self._comp._ctx)
        off, img = plan.instruction_image()
        dec.upload(d_work + off, img)
        stage = (plan.work_size + 15) & ~15
        dec.decode_bodies(bodies, d_work + stage, d_work, plan.pay_off, plan.pay_size)
        return self.replay(plan, d_work, d_out, out_cap)

    def close(self):
        self._comp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _range_check(L, ctx, rc, what):
    if rc != _lib.ZC_OK:
        msg = L.zc_last_error(ctx) or b""
        raise _lib.ZcError(f"{what} failed ({rc}): {msg.decode(errors='replace')}")


class RangeIndex:
    """A zc_range_index: entry e of the stream is sizes[e] bytes at off[e] of
    slot[e]; a slot is one resident payload of slot_sizes[k] bytes.  `comp`, a
    BundleCompressor, gives the context whose device holds the index and whose
    stream runs the reads; without one the index is host only (`total`,
    `needs` and every argument check work)."""

    def __init__(self, slot_sizes, slot, off, sizes, comp=None):
        self._L = _lib.load()
        self._ctx = comp._ctx if comp is not None else None
        slot_sizes, off, sizes = _u64(slot_sizes), _u64(off), _u64(sizes)
        slot = np.ascontiguousarray(np.asarray(slot, dtype=np.uint32))
        if not len(slot) == len(off) == len(sizes):
            raise ValueError("RangeIndex: slot, off and sizes differ in length")
        self._idx = ctypes.c_void_p()
        rc = self._L.zc_range_index_create(self._ctx, slot_sizes.ctypes.data, len(slot_sizes), slot.ctypes.data,
                                           off.ctypes.data, sizes.ctypes.data, len(sizes), ctypes.byref(self._idx))
        _range_check(self._L, self._ctx, rc, "zc_range_index_create")
        total = ctypes.c_uint64()
        self._L.zc_range_index_total(self._idx, ctypes.byref(total))
        self.total = total.value
        self.n_slots = len(slot_sizes)

    def set_slot(self, slot, d_ptr):
        """Caller-owned device memory of the slot's size; None clears it."""
        _range_check(self._L, None, self._L.zc_range_set_slot(self._idx, int(slot), d_ptr), "zc_range_set_slot")

    def upload_slot(self, slot, payload):
        """A copy of host bytes the index owns; their length must be the slot's size."""
        payload = bytes(payload)
        buf = np.frombuffer(payload or b"\0", dtype=np.uint8)
        rc = self._L.zc_range_slot_upload(self._idx, int(slot), buf.ctypes.data, len(payload))
        _range_check(self._L, None, rc, "zc_range_slot_upload")

    def drop_slot(self, slot):
        _range_check(self._L, None, self._L.zc_range_slot_drop(self._idx, int(slot)), "zc_range_slot_drop")

    @staticmethod
    def _reads(reads):
        if not isinstance(reads, np.ndarray):
            reads = list(reads)
        r = np.asarray(reads, dtype=np.uint64).reshape(-1, 2)
        return np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])

    def needs(self, reads):
        """The distinct slots the reads [(offset, size), ...] touch, ascending."""
        offset, size = self._reads(reads)
        out = np.zeros(max(self.n_slots, 1), dtype=np.uint32)
        n = ctypes.c_size_t()
        rc = self._L.zc_range_needs(self._idx, offset.ctypes.data, size.ctypes.data, len(offset), out.ctypes.data,
                                    self.n_slots, ctypes.byref(n))
        _range_check(self._L, None, rc, "zc_range_needs")
        return [int(s) for s in out[:n.value]]

    def read(self, reads, d_out, dst_off):
        """One batch: read i's bytes to d_out + dst_off[i] (device memory)."""
        offset, size = self._reads(reads)
        dst_off = _u64(dst_off)
        if len(dst_off) != len(offset):
            raise ValueError("RangeIndex.read: reads and dst_off differ in length")
        rc = self._L.zc_range_read(self._ctx, self._idx, offset.ctypes.data, size.ctypes.data, len(offset), d_out,
                                   dst_off.ctypes.data)
        _range_check(self._L, self._ctx, rc, "zc_range_read")

    def read_host(self, reads):
        """The reads' bytes, one bytes object each, through the pinned staging buffer."""
        offset, size = self._reads(reads)
        dst_off = (np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64) if len(size)
                   else np.zeros(0, dtype=np.uint64))
        out = np.zeros(max(int(size.sum()), 1), dtype=np.uint8)
        rc = self._L.zc_range_read_host(self._ctx, self._idx, offset.ctypes.data, size.ctypes.data, len(offset),
                                        out.ctypes.data, dst_off.ctypes.data)
        _range_check(self._L, self._ctx, rc, "zc_range_read_host")
        return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(dst_off, size)]

    def last_stats(self):
        """(upload ms, kernel ms, pieces) of the context's last read."""
        up, kern, pieces = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        rc = self._L.zc_range_last_stats(self._ctx, ctypes.byref(up), ctypes.byref(kern), ctypes.byref(pieces))
        _range_check(self._L, self._ctx, rc, "zc_range_last_stats")
        return up.value, kern.value, pieces.value

    def close(self):
        if self._idx:
            self._L.zc_range_index_destroy(self._idx)
            self._idx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class IndexedRestorer:
    """Any byte range of a backup from the bundle payloads resident at the
    time: BackupRestorer::IndexedRestorer on the GPU.  Built on Restorer.plan's
    parse and id map: slot k is the decoded payload of bundle `plan.used[k]`,
    the last slot the instruction stream, uploaded here.  Reads are
    (offset, size) pairs; `needs` tells which bundles a batch wants resident.
    device=None makes a host-only object (`size`, `needs`), for planning."""

    def __init__(self, backup_data, bundles, device=0, ctx=None):
        plan = Restorer.plan(backup_data, bundles)
        pay_off = np.asarray(plan.pay_off, dtype=np.uint64)
        in_instr = plan.src_off >= np.uint64(plan.instr_off)
        k = np.searchsorted(pay_off, plan.src_off, side="right").astype(np.int64) - 1
        k[in_instr] = len(plan.used)
        base = np.concatenate([pay_off, [plan.instr_off]]).astype(np.uint64)
        self._setup(plan, k, plan.src_off - base[k], device, ctx)

    @classmethod
    def from_index(cls, backup_data, chunk_index, device=0, ctx=None):
        """The same from a resident ChunkIndex: Restorer.plan_index's plan,
        whose fetched (slot, offset) arrays are the RangeIndex's entries as
        they are.  `needs` and the payload calls speak in the index's bundle
        numbers.  ctx None: the chunk index's context."""
        self = cls.__new__(cls)
        plan = Restorer.plan_index(backup_data, chunk_index)
        if device is not None and ctx is None:
            ctx = chunk_index._ctx
        self._setup(plan, plan.slot, plan.off, device, ctx)
        return self

    def _setup(self, plan, k, off, device, ctx):
        self.plan = plan
        self._comp = BundleCompressor(device=device, ctx=ctx) if device is not None or ctx is not None else None
        self._slot_of = {b: i for i, b in enumerate(plan.used)}
        self._decoded = {}  # slot -> device buffer of a payload decoded here
        self._index = None
        try:
            self._index = RangeIndex(list(plan.pay_size) + [len(plan.data)], k, off, plan.sizes, comp=self._comp)
            self.size = self._index.total
            if self._comp is not None:
                self._index.upload_slot(len(plan.used), plan.data)
        except Exception:
            self.close()  # the context made above does not outlive a failed construction
            raise

    def _slot(self, bundle):
        if bundle not in self._slot_of:
            raise _lib.ZcError(f"bundle {bundle} is not one the stream references")
        return self._slot_of[bundle]

    def needs(self, reads):
        """The bundles (indices into `bundles`) whose payloads the reads touch."""
        return [self.plan.used[s] for s in self._index.needs(reads) if s < len(self.plan.used)]

    def set_payload(self, bundle, d_ptr):
        """The bundle's decoded payload in caller-owned device memory."""
        slot = self._slot(bundle)
        self._index.set_slot(slot, d_ptr)
        self._free_decoded(slot)

    def upload_payload(self, bundle, payload):
        slot = self._slot(bundle)
        self._index.upload_slot(slot, payload)
        self._free_decoded(slot)

    def _free_decoded(self, slot):
        old = self._decoded.pop(slot, None)
        if old is not None:
            BundleDecompressor(ctx=self._comp._ctx).free(old)

    def decode_payload(self, bundle, body):
        """The bundle's payload from its LZMA body (host bytes: the xz stream),
        decoded on the device into a buffer this object owns, beside
        upload_payload: the compressed bytes cross, the payload does not."""
        slot = self._slot(bundle)
        if self._comp is None:
            raise _lib.ZcError("decode_payload: a host-only IndexedRestorer has no device")
        dec = BundleDecompressor(ctx=self._comp._ctx)
        size = int(self.plan.pay_size[slot])
        out_bytes = (size + 15) & ~15
        buf = dec.alloc(out_bytes + dec.stage_size([body]))
        try:
            dec.decode_bodies([body], buf + out_bytes, buf, [0], [size])
            self._index.set_slot(slot, buf)
        except Exception:
            dec.free(buf)
            raise
        old = self._decoded.pop(slot, None)
        self._decoded[slot] = buf
        if old is not None:
            dec.free(old)

    def drop_payload(self, bundle):
        slot = self._slot(bundle)
        self._index.drop_slot(slot)
        self._free_decoded(slot)

    def read(self, reads, d_out, dst_off):
        self._index.read(reads, d_out, dst_off)

    def read_host(self, offset, size):
        return self._index.read_host([(offset, size)])[0]

    def last_stats(self):
        return self._index.last_stats()

    def close(self):
        if self._index is not None:
            self._index.close()
            self._index = None
        if self._comp is not None:
            for buf in self._decoded.values():
                BundleDecompressor(ctx=self._comp._ctx).free(buf)
            self._decoded = {}
            self._comp.close()
            self._comp = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
