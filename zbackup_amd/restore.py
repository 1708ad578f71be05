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

  restoreIterations          -> iterations in HBM         backup_restorer.cc:109-136

`Restorer.restore_iterations` keeps every intermediate instruction stream on the
device: `parse_device` (zc_parse_instructions_device), `plan_device`
(zc_restore_resolve_device, a `DevicePlan` whose per-entry lists stay in HBM)
and `replay_device` (zc_restore_replay) per round, each round's output the next
round's stream; `XzBodiesPayloads` serves the rounds' bundles from xz bodies.

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

    # ---- the same with the stream, the entries and the plan in HBM (restoreIterations) ----

    def parse_device(self, d_stream, n):
        """zc_parse_instructions_device: the stream's n bytes at d_stream
        (device memory) to an InstructionSet in HBM.  Raises ZcError with the
        host parser's text on a malformed stream."""
        L, ctx = self._comp._L, self._comp._ctx
        handle = ctypes.c_void_p()
        rc = L.zc_parse_instructions_device(ctx, d_stream if n else None, int(n), ctypes.byref(handle))
        _range_check(L, ctx, rc, "zc_parse_instructions_device")
        return InstructionSet(L, handle)

    def plan_device(self, instr_set, chunk_index):
        """zc_restore_resolve_device: a DevicePlan whose per-entry lists stay
        in HBM.  Raises what plan_index raises, in the same words, for a
        missing id (naming it) and for a used bundle that holds an id twice
        (naming the bundle): one entry is fetched for the name, no more."""
        L, ctx = self._comp._L, self._comp._ctx
        handle = ctypes.c_void_p()
        rc = L.zc_restore_resolve_device(ctx, chunk_index._live(), instr_set._live(), ctypes.byref(handle))
        _range_check(L, ctx, rc, "zc_restore_resolve_device")
        plan = DevicePlan(L, handle)
        try:
            if plan.n_missing:
                blob = instr_set.fetch(plan.first_missing, 1)[0]["id"].tobytes()
                raise _lib.ZcError(f"restore: chunk id {blob.hex()} is in none of the "
                                   f"{chunk_index.counts()['bundles']} bundles ({plan.n_missing} entries miss)")
            if plan.n_dup_used:
                b = int(plan.used[plan.entry(plan.first_dup)[0]])
                raise _lib.ZcError(f"restore: bundle {b}: a chunk id twice in one bundle (entry {plan.first_dup})")
        except Exception:
            plan.close()
            raise
        return plan

    def replay_device(self, plan, slot_ptrs, d_out, out_cap):
        """zc_restore_replay: slot_ptrs[k] = the device pointer of the decoded
        payload of bundle plan.used[k], slot_ptrs[n_used] = the instruction
        stream the plan was parsed from.  Returns the restored length."""
        L, ctx = self._comp._L, self._comp._ctx
        ptrs = (ctypes.c_void_p * max(len(slot_ptrs), 1))(*[int(p) if p else None for p in slot_ptrs])
        rc = L.zc_restore_replay(ctx, plan._live(), ptrs, len(slot_ptrs), d_out, int(out_cap))
        _range_check(L, ctx, rc, "zc_restore_replay")
        return plan.length

    def restore_iterations(self, backup_data, iterations, chunk_index, payloads, out_cap):
        """restoreIterations (backup_restorer.cc:109-136): backup_data restores
        to the instruction stream of the iteration below, `iterations` times,
        and that to the user data.  backup_data is uploaded once; then
        iterations + 1 rounds of parse, plan, payloads(used, used_size) -- a
        list of device pointers, one per used bundle -- and replay, each
        round's output buffer the next round's stream.  Nothing per entry
        crosses to the host.  Returns (device buffer, length): the user data,
        the caller's to free (`free`); out_cap bounds every round's length."""
        dec = BundleDecompressor(ctx=self._comp._ctx)
        backup_data = bytes(backup_data)
        d_stream, n = dec.alloc(max(len(backup_data), 1)), len(backup_data)
        try:
            dec.upload(d_stream, backup_data)
            for _ in range(int(iterations) + 1):
                with self.parse_device(d_stream, n) as ins, self.plan_device(ins, chunk_index) as plan:
                    if plan.length > out_cap:
                        raise _lib.ZcError(f"restore: {plan.length} bytes to restore, room for {out_cap}")
                    ptrs = list(payloads(plan.used, plan.used_size))
                    d_out = dec.alloc(max(plan.length, 1))
                    try:
                        # the round's bytes_to_emit runs are read from d_stream: it lives until the replay is done
                        self.replay_device(plan, ptrs + [d_stream], d_out, plan.length)
                    except Exception:
                        dec.free(d_out)
                        raise
                    length = plan.length
                dec.free(d_stream)
                d_stream, n = d_out, length
            out, d_stream = d_stream, None
            return out, n
        finally:
            if d_stream is not None:
                dec.free(d_stream)

    def free(self, d_ptr):
        """Frees a buffer restore_iterations returned."""
        BundleDecompressor(ctx=self._comp._ctx).free(d_ptr)

    def parse_last_stats(self):
        """dict(hop_ms, exit_ms, chain_ms, emit_ms, tiles, chain_hops) of the last parse_device."""
        L, ctx = self._comp._L, self._comp._ctx
        ms = [ctypes.c_double() for _ in range(4)]
        cnt = [ctypes.c_uint64() for _ in range(2)]
        rc = L.zc_instr_last_stats(ctx, *[ctypes.byref(x) for x in ms + cnt])
        _range_check(L, ctx, rc, "zc_instr_last_stats")
        return dict(zip(("hop_ms", "exit_ms", "chain_ms", "emit_ms", "tiles", "chain_hops"),
                        [x.value for x in ms + cnt]))

    def close(self):
        self._comp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class InstructionSet:
    """A zc_instr_set: a parsed BackupInstruction stream's entries in HBM
    (`n_entries`, `n_messages`, `bytes_total`); fetch() is for tests and for
    naming one entry in an error."""

    def __init__(self, L, handle):
        self._L, self._handle = L, handle
        c = [ctypes.c_uint64() for _ in range(3)]
        rc = L.zc_instr_set_counts(handle, *[ctypes.byref(x) for x in c])
        if rc != _lib.ZC_OK:
            raise _lib.ZcError(f"zc_instr_set_counts failed ({rc})")
        self.n_entries, self.n_messages, self.bytes_total = (x.value for x in c)

    def _live(self):
        if self._handle is None:
            raise _lib.ZcError("InstructionSet: closed")
        return self._handle

    def fetch(self, first=0, count=None):
        """Entries [first, first + count) as parse_backup_data's array."""
        from .bundle import INSTRUCTION_DTYPE
        count = self.n_entries - first if count is None else count
        out = np.zeros(max(count, 0), dtype=INSTRUCTION_DTYPE)
        rc = self._L.zc_instr_set_fetch(self._live(), int(first), int(count), out.ctypes.data if count else None)
        if rc != _lib.ZC_OK:
            msg = self._L.zc_last_error(None) or b""
            raise _lib.ZcError(f"zc_instr_set_fetch failed ({rc}): {msg.decode(errors='replace')}")
        return out

    def close(self):
        if self._handle is not None:
            self._L.zc_instr_set_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DevicePlan:
    """A zc_restore_plan whose per-entry lists lie in HBM: the counters
    (ResolvedStream's names), `used` / `used_size` per used bundle; `entry(e)`
    gives one entry's (slot, off, size, dst); `slot`, `off`, `size`, `dst`
    download all of them on first use."""
    COUNTS = ("n_entries", "n_used", "length", "n_missing", "first_missing", "n_dup_used", "first_dup")

    def __init__(self, L, handle):
        self._L, self._handle, self._lists = L, handle, None
        c = [ctypes.c_uint64() for _ in self.COUNTS]
        rc = L.zc_restore_plan_counts(handle, *[ctypes.byref(x) for x in c])
        if rc != _lib.ZC_OK:
            raise _lib.ZcError(f"zc_restore_plan_counts failed ({rc})")
        for name, x in zip(self.COUNTS, c):
            setattr(self, name, x.value)
        self.used, self.used_size = np.zeros(self.n_used, dtype=np.uint32), np.zeros(self.n_used, dtype=np.uint64)
        if self.n_used:
            rc = L.zc_restore_plan_used(handle, self.used.ctypes.data, self.used_size.ctypes.data)
            if rc != _lib.ZC_OK:
                raise _lib.ZcError(f"zc_restore_plan_used failed ({rc})")

    def _live(self):
        if self._handle is None:
            raise _lib.ZcError("DevicePlan: closed")
        return self._handle

    def _fetch(self, *arrays):
        rc = self._L.zc_restore_plan_fetch(self._live(), *[a.ctypes.data if a is not None and len(a) else None
                                                           for a in arrays])
        if rc != _lib.ZC_OK:
            msg = self._L.zc_last_error(None) or b""
            raise _lib.ZcError(f"zc_restore_plan_fetch failed ({rc}): {msg.decode(errors='replace')}")

    def entry(self, e):
        """(slot, off, size, dst) of entry e (zc_restore_plan_entry)."""
        slot = ctypes.c_uint32()
        v = [ctypes.c_uint64() for _ in range(3)]
        rc = self._L.zc_restore_plan_entry(self._live(), int(e), ctypes.byref(slot), *[ctypes.byref(x) for x in v])
        if rc != _lib.ZC_OK:
            msg = self._L.zc_last_error(None) or b""
            raise _lib.ZcError(f"zc_restore_plan_entry failed ({rc}): {msg.decode(errors='replace')}")
        return (slot.value,) + tuple(x.value for x in v)

    def _list(self, k):
        if self._lists is None:
            n = self.n_entries
            lists = (np.zeros(n, dtype=np.uint32),) + tuple(np.zeros(n, dtype=np.uint64) for _ in range(3))
            self._fetch(None, None, *lists)
            self._lists = lists
        return self._lists[k]

    slot = property(lambda self: self._list(0))
    off = property(lambda self: self._list(1))
    size = property(lambda self: self._list(2))
    dst = property(lambda self: self._list(3))

    def close(self):
        if self._handle is not None:
            self._L.zc_restore_plan_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class XzBodiesPayloads:
    """A ready-made `payloads` of Restorer.restore_iterations for LZMA bundles
    held in host memory: bodies[bundle number] = the bundle's xz stream
    (zc_bundle_unseal's body).  A bundle is decoded on the device the first
    time a round uses it (BundleDecompressor.decode_bodies) and its payload is
    kept, so a bundle two iterations use is decoded once (`decodes` counts
    them).  close() frees the payloads."""

    def __init__(self, bodies, device=0, ctx=None):
        self._bodies = bodies
        self._dec = BundleDecompressor(device=device, ctx=ctx)
        self._resident = {}  # bundle -> device pointer of its payload
        self._buffers = []   # one device buffer per call that decoded something
        self.decodes = 0

    def __call__(self, used, used_size):
        new = [(int(b), int(s)) for b, s in zip(used, used_size) if int(b) not in self._resident]
        for b, _ in new:
            if b not in self._bodies:
                raise _lib.ZcError(f"restore: no body for bundle {b}")
        if new:
            bodies = [self._bodies[b] for b, _ in new]
            out_off, pos = [], 0
            for _, s in new:
                out_off.append(pos)
                pos += (s + 15) & ~15
            # the payloads first, the staged bodies behind them
            buf = self._dec.alloc(pos + max(self._dec.stage_size(bodies), 1))
            try:
                self._dec.decode_bodies(bodies, buf + pos, buf, out_off, [s for _, s in new])
            except Exception:
                self._dec.free(buf)
                raise
            self._buffers.append(buf)
            for (b, _), o in zip(new, out_off):
                self._resident[b] = buf + o
            self.decodes += len(new)
        return [self._resident[int(b)] for b in used]

    def close(self):
        if self._dec is not None:
            for p in self._buffers:
                self._dec.free(p)
            self._buffers, self._resident = [], {}
            self._dec.close()
            self._dec = None

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
