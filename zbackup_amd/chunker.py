"""Python host mirror of zbackup's BackupCreator on the MI355X engine.

Names, argument meaning and error behaviour follow the reference:
  BackupCreator(config, chunkIndex, writer)      backup_creator.hh:83
    getInputBuffer / getInputBufferSize          backup_creator.cc:40-54
    handleMoreData(added)                        backup_creator.cc:56-108
    finish()                                     backup_creator.cc:147-172
    getBackupData(string &)  -- callable once    backup_creator.cc:275-280
  ChunkId::toBlob  (16-byte SHA-1 prefix + LE rolling hash)   chunk_id.cc:19-27
  Message::serialize (varint32 length + BackupInstruction)    message.cc:16-23

All work runs in libzchunk.so on the GPU; there is no CPU fallback.
"""
import ctypes
import struct

import numpy as np

from . import _lib

RECORD_DTYPE = np.dtype([("offset", "<u8"), ("size", "<u4"), ("kind", "<u4"),
                         ("rolling", "<u8"), ("sha1", "u1", (16,))])
KIND_CHAR = "NDB"
SEED_DTYPE = np.dtype([("sha1", np.uint8, 16), ("rolling", np.uint64), ("size", np.uint32), ("reserved", np.uint32)])
# zc_chunk_meta (ABI 5): a chunk's content-anchor metadata, keyed by its ChunkId
META_DTYPE = np.dtype([("sha1", np.uint8, 16), ("rolling", "<u8"), ("size", "<u4"), ("anchor_def", "<u4"),
                       ("anchor", "<u4"), ("gear", "<u4"), ("fingerprint", "<u8")])


def _check(L, ctx, rc, what):
    if rc != _lib.ZC_OK:
        msg = L.zc_last_error(ctx) if ctx else b""
        raise _lib.ZcError(f"{what} failed ({rc}): {(msg or b'').decode(errors='replace')}")


def chunk_id_blob(sha1_16, rolling):
    """ChunkId::toBlob (chunk_id.cc:19-27)."""
    return bytes(sha1_16) + struct.pack("<Q", rolling)


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def serialize_instruction(chunk_blob=None, raw=None):
    """Message::serialize of one BackupInstruction (zbackup.proto:149-159)."""
    body = b""
    if chunk_blob is not None:
        body += b"\x0a" + _varint(len(chunk_blob)) + chunk_blob
    if raw is not None:
        body += b"\x12" + _varint(len(raw)) + raw
    return _varint(len(body)) + body


def _seed_array(sha1, rolling, size):
    """(sha1 (n, 16) uint8, rolling (n,) uint64, size scalar or (n,)) -> SEED_DTYPE array (zc_seed)."""
    rolling = np.ascontiguousarray(rolling, dtype=np.uint64).reshape(-1)
    n = rolling.size
    rec = np.zeros(n, dtype=SEED_DTYPE)
    assert rec.dtype.itemsize == ctypes.sizeof(_lib.ZcSeed)
    if n:
        rec["sha1"] = np.asarray(sha1, dtype=np.uint8).reshape(n, 16)
        rec["rolling"] = rolling
        rec["size"] = size
    return rec


def serialized_size(recs):
    """zc_serialized_size: the length of the BackupInstruction stream of a
    RECORD_DTYPE array (host bookkeeping: no context, no device)."""
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    need = ctypes.c_uint64()
    L = _lib.load()
    rc = L.zc_serialized_size(recs.ctypes.data if len(recs) else None, len(recs), ctypes.byref(need))
    if rc != _lib.ZC_OK:  # a call without a context: the message is the thread's
        raise _lib.ZcError(f"zc_serialized_size failed ({rc}): {L.zc_last_error(None).decode(errors='replace')}")
    return need.value


def anchor_def(chunk_max_size):
    """zc_anchor_def: the anchor definition this build's metadata carries for W."""
    return int(_lib.load().zc_anchor_def(int(chunk_max_size)))


class BackupCreator:
    """One stream through the engine.  `seeds` are (sha1_16, rolling, size)
    entries of an existing index (ChunkIndex::loadIndex).  `window`: bytes of
    the feed held in HBM (None: the library's default, 1 GiB; 0: the whole
    stream, resolved at finish()); see zc_set_window."""

    def __init__(self, chunk_max_size=65536, seeds=(), device=0, sha1=True, timing=False, staged_screen=True,
                 window=None):
        self._L = _lib.load()
        self.chunk_max_size = int(chunk_max_size)
        flags = (_lib.ZC_FLAG_SHA1 if sha1 else 0) | (_lib.ZC_FLAG_TIMING if timing else 0)
        if not staged_screen:  # diagnostics: the lane-per-KiB exact screen only
            flags |= _lib.ZC_FLAG_NO_STAGED_SCREEN
        ctx = ctypes.c_void_p()
        rc = self._L.zc_create(ctypes.byref(ctx), self.chunk_max_size, device, flags)
        if rc != _lib.ZC_OK:
            raise _lib.ZcError(f"zc_create failed ({rc})")
        self._ctx = ctx
        self._new_stream()
        if window is not None:
            _check(self._L, self._ctx, self._L.zc_set_window(self._ctx, int(window)), "zc_set_window")
        self.seed_index(seeds)

    def seed_index(self, seeds):
        """Add (sha1_16, rolling, size) ids to the context's index (zc_seed_index:
        what ChunkIndex::loadIndex registers, chunk_index.cc:26-79,163-182)."""
        seeds = list(seeds)
        if seeds:
            arr = (_lib.ZcSeed * len(seeds))()
            for i, (sha, rolling, size) in enumerate(seeds):
                arr[i].sha1[:] = list(sha[:16])
                arr[i].rolling = rolling
                arr[i].size = size
            _check(self._L, self._ctx, self._L.zc_seed_index(self._ctx, arr, len(seeds)), "zc_seed_index")

    def seed_index_arrays(self, sha1, rolling, size):
        """seed_index for ids given as arrays: sha1 (n, 16) uint8, rolling (n,)
        uint64, size a scalar or (n,) -- one copy into the ZcSeed array (an
        index file's worth of ids without a Python loop)."""
        rec = _seed_array(sha1, rolling, size)
        if rec.size == 0:
            return
        arr = (_lib.ZcSeed * rec.size).from_buffer(rec)
        _check(self._L, self._ctx, self._L.zc_seed_index(self._ctx, arr, rec.size), "zc_seed_index")

    def seed_index_meta(self, sha1, rolling, size, meta):
        """zc_seed_index_meta: the ids of an existing index (arrays as in
        seed_index_arrays) with the anchor metadata kept for them (a META_DTYPE
        array, e.g. from export_chunk_meta of the backups that wrote them).  Ids
        whose metadata matches join the anchor-probed historic index, the rest
        are seeded by value; metadata of ids not given is ignored."""
        rec = _seed_array(sha1, rolling, size)
        meta = np.ascontiguousarray(meta, dtype=META_DTYPE)
        assert META_DTYPE.itemsize == ctypes.sizeof(_lib.ZcChunkMeta)
        _check(self._L, self._ctx,
               self._L.zc_seed_index_meta(self._ctx, rec.ctypes.data if rec.size else None, rec.size,
                                          meta.ctypes.data if meta.size else None, meta.size),
               "zc_seed_index_meta")

    def export_chunk_meta(self):
        """zc_export_chunk_meta: the anchor metadata of the W-byte chunks this
        context's streams added to its index (ZC_FLAG_SHA1), as a META_DTYPE
        array in the order they were added."""
        need = ctypes.c_size_t()
        self._L.zc_export_chunk_meta(self._ctx, None, 0, ctypes.byref(need))
        out = np.zeros(need.value, dtype=META_DTYPE)
        if need.value:
            _check(self._L, self._ctx,
                   self._L.zc_export_chunk_meta(self._ctx, out.ctypes.data, out.size, ctypes.byref(need)),
                   "zc_export_chunk_meta")
        return out

    def _new_stream(self):
        # A fed stream's records are taken from the context as they are cut and
        # serialized right away, while their bytes are still in the feed window
        # (bytes_to_emit reads them): BackupCreator::outputInstruction also runs
        # inside handleMoreData (backup_creator.cc:267-273).  A long stream through
        # a bounded window would otherwise have evicted them by getBackupData.
        self._data = bytearray()  # BackupInstruction stream of the records taken
        self._taken = []          # record arrays taken from the context, stream order
        self._given = 0           # arrays of _taken that take_records() has returned
        self._data_taken = False

    def _drain(self):
        """Take the complete records from the context and serialize them now."""
        n = self._L.zc_record_count(self._ctx)
        if not n:
            return
        out = np.zeros(n, dtype=RECORD_DTYPE)
        got = ctypes.c_size_t()
        _check(self._L, self._ctx,
               self._L.zc_take_records(self._ctx, out.ctypes.data_as(ctypes.POINTER(_lib.ZcRecord)), n,
                                       ctypes.byref(got)), "zc_take_records")
        out = out[: got.value]
        self._data += self._serialize(out)
        self._taken.append(out)

    def _serialize(self, recs):
        recs = np.ascontiguousarray(recs)
        need = ctypes.c_size_t()
        self._L.zc_serialize_records(self._ctx, recs.ctypes.data, len(recs), None, 0, ctypes.byref(need))
        out = np.zeros(max(need.value, 1), dtype=np.uint8)
        rc = self._L.zc_serialize_records(self._ctx, recs.ctypes.data, len(recs), out.ctypes.data, out.size,
                                          ctypes.byref(need))
        _check(self._L, self._ctx, rc, "zc_serialize_records")
        return out[:need.value].tobytes()

    # -- feed contract -------------------------------------------------------
    def get_input_buffer(self):
        """Writable view of getInputBufferSize() bytes (pinned host staging)."""
        p = self._L.zc_get_input_buffer(self._ctx)
        if not p:
            raise _lib.ZcError("no input buffer after finish()")
        n = self._L.zc_get_input_buffer_size(self._ctx)
        return (ctypes.c_uint8 * n).from_address(p)

    def get_input_buffer_size(self):
        return self._L.zc_get_input_buffer_size(self._ctx)

    def handle_more_data(self, added):
        _check(self._L, self._ctx, self._L.zc_handle_more_data(self._ctx, added), "handleMoreData")
        self._drain()

    def feed(self, data):
        """The read loop of zutils.cc:100-124 over `data`: each piece copied into
        getInputBuffer() (at most getInputBufferSize() bytes), handleMoreData,
        and the records cut by then taken and serialized while their payload
        bytes are still in the feed window (a long stream slides the window on
        the next getInputBuffer call)."""
        data = np.ascontiguousarray(np.frombuffer(memoryview(data), dtype=np.uint8))
        pos = 0
        while pos < data.size:
            p = self._L.zc_get_input_buffer(self._ctx)
            room = self._L.zc_get_input_buffer_size(self._ctx)
            if not p or not room:
                msg = self._L.zc_last_error(self._ctx) or b""
                raise _lib.ZcError(f"getInputBuffer failed: {msg.decode(errors='replace')}")
            take = min(room, data.size - pos)
            ctypes.memmove(p, data.ctypes.data + pos, take)
            self.handle_more_data(take)
            pos += take

    def finish(self):
        _check(self._L, self._ctx, self._L.zc_finish(self._ctx), "finish")
        self._drain()

    # -- device-resident stream ----------------------------------------------
    def chunk_device(self, ptr, n):
        """Process `n` bytes already in HBM at device pointer `ptr` (e.g. a torch
        uint8 tensor's data_ptr()); feed + finish in one call."""
        self._new_stream()
        _check(self._L, self._ctx, self._L.zc_chunk_device(self._ctx, ctypes.c_void_p(ptr), n),
               "zc_chunk_device")

    def chunk_host(self, ptr, n):
        """Process `n` bytes in host memory at address `ptr` (pinned for full
        speed): HBM copies in 64 MiB segments overlapped with the scan, then
        the same pipeline as chunk_device (zutils.cc:100-124 read loop + finish)."""
        self._new_stream()
        _check(self._L, self._ctx, self._L.zc_chunk_host(self._ctx, ctypes.c_void_p(ptr), n), "zc_chunk_host")

    # -- the backup data kept in HBM -------------------------------------------
    def serialize_device(self, recs, d_stream, stream_len):
        """zc_serialize_records_device: the BackupInstruction stream of `recs` (a
        RECORD_DTYPE array whose offsets refer to the `stream_len` bytes at device
        pointer `d_stream`), written into a device buffer of its own.  Returns
        (device pointer, bytes); the caller hands the pointer to free_device."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        need = serialized_size(recs)
        d_out = ctypes.c_void_p()
        _check(self._L, self._ctx, self._L.zc_device_alloc(self._ctx, need, ctypes.byref(d_out)), "zc_device_alloc")
        wrote = ctypes.c_uint64()
        rc = self._L.zc_serialize_records_device(self._ctx, recs.ctypes.data, len(recs),
                                                 ctypes.c_void_p(d_stream) if stream_len else None, stream_len,
                                                 d_out, need, ctypes.byref(wrote))
        if rc != _lib.ZC_OK:
            msg = self._L.zc_last_error(self._ctx) or b""
            self._L.zc_device_free(self._ctx, d_out)
            raise _lib.ZcError(f"zc_serialize_records_device failed ({rc}): {msg.decode(errors='replace')}")
        return d_out.value, wrote.value

    def free_device(self, d_ptr):
        """zc_device_free of a buffer serialize_device returned."""
        _check(self._L, self._ctx, self._L.zc_device_free(self._ctx, ctypes.c_void_p(d_ptr)), "zc_device_free")

    def serialize_stats(self):
        """zc_serialize_last_stats as a dict: upload_ms, size_ms, write_ms (device
        time of the last serialize_device's steps), staged_msgs, copy_pieces."""
        ms = [ctypes.c_double() for _ in range(3)]
        cnt = [ctypes.c_uint64() for _ in range(2)]
        _check(self._L, self._ctx,
               self._L.zc_serialize_last_stats(self._ctx, *[ctypes.byref(v) for v in ms + cnt]),
               "zc_serialize_last_stats")
        names = ("upload_ms", "size_ms", "write_ms", "staged_msgs", "copy_pieces")
        return {k: v.value for k, v in zip(names, ms + cnt)}

    def _download(self, d_ptr, n):
        """`n` bytes of device memory as bytes: one read through the range reader's staging buffer."""
        if not n:
            return b""
        one, zero, slot = np.array([n], dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
        idx = ctypes.c_void_p()
        _check(self._L, self._ctx,
               self._L.zc_range_index_create(self._ctx, one.ctypes.data, 1, slot.ctypes.data, zero.ctypes.data,
                                             one.ctypes.data, 1, ctypes.byref(idx)), "zc_range_index_create")
        out = np.empty(n, dtype=np.uint8)
        try:
            rc = self._L.zc_range_set_slot(idx, 0, ctypes.c_void_p(d_ptr))
            if rc == _lib.ZC_OK:
                rc = self._L.zc_range_read_host(self._ctx, idx, zero.ctypes.data, one.ctypes.data, 1,
                                                out.ctypes.data, zero.ctypes.data)
            _check(self._L, self._ctx, rc, "zc_range_read_host")
        finally:
            self._L.zc_range_index_destroy(idx)
        return out.tobytes()

    def backup_device(self, ptr, n, on_new=None):
        """The backup of `n` bytes at device pointer `ptr` with its backup data kept
        in HBM: chunk_device, serialize_device, then backupFromFileHandle's
        shrink loop (zutils.cc:137-166) -- reset(), chunk_device on the
        serialized buffer where it lies, on this context, so that a pass matches
        the chunks the passes before it added; the new generation is kept only
        when it is strictly shorter, else the loop ends.  Only the final stream
        comes to the host.

        on_new(new_records, d_stream_ptr, pass_no) is called once per pass, the
        last, discarded one included (its chunks were added like the others'),
        with the pass's ZC_CHUNK_NEW records and the device buffer their offsets
        refer to, which stays valid during the call: the place to
        zc_bundle_gather their payloads.  Pass 0 is the user's stream.

        Returns (backup_data, iterations, pass_lengths): pass_lengths[k] is the
        length of the stream pass k wrote.  The context is reset() at the end:
        no buffer it refers to outlives the call."""
        def one_pass(d_stream, length, pass_no):
            self.chunk_device(d_stream, length)
            recs = self.records()
            if on_new is not None:
                on_new(recs[recs["kind"] == _lib.ZC_CHUNK_NEW], d_stream, pass_no)
            return self.serialize_device(recs, d_stream, length)

        cur, cur_n = one_pass(ptr, n, 0)
        lengths, iterations = [cur_n], 0
        try:
            while True:
                self.reset()
                nxt, nxt_n = one_pass(cur, cur_n, len(lengths))
                lengths.append(nxt_n)
                if nxt_n < cur_n:
                    self.free_device(cur)  # the next generation is serialized: nothing reads this one again
                    cur, cur_n = nxt, nxt_n
                    iterations += 1
                else:
                    self.free_device(nxt)
                    break
            data = self._download(cur, cur_n)
        finally:
            self._L.zc_reset(self._ctx)
            self._L.zc_device_free(self._ctx, ctypes.c_void_p(cur))
        self._new_stream()
        return data, iterations, lengths

    # -- results -------------------------------------------------------------
    def _held(self):
        n = self._L.zc_record_count(self._ctx)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        got = ctypes.c_size_t()
        _check(self._L, self._ctx,
               self._L.zc_get_records(self._ctx, out.ctypes.data_as(ctypes.POINTER(_lib.ZcRecord)), n,
                                      ctypes.byref(got)), "zc_get_records")
        return out[: got.value]

    def records(self):
        """Every record of the stream so far, in stream order (those already
        taken from the context and those it still holds)."""
        held = self._held()
        if not self._taken:
            return held
        return np.concatenate(self._taken + [held])

    def take_records(self):
        """Complete records cut since the last take_records() (the
        instructions outputInstruction writes during handleMoreData)."""
        self._drain()
        new = self._taken[self._given:]
        self._given = len(self._taken)
        return np.concatenate(new) if new else np.zeros(0, dtype=RECORD_DTYPE)

    @property
    def window(self):
        return int(self._L.zc_get_window(self._ctx))

    def set_window(self, window):
        """zc_set_window between streams (after reset(), before the next stream's
        first byte): the feed window in bytes, 0 for the whole stream in HBM."""
        _check(self._L, self._ctx, self._L.zc_set_window(self._ctx, int(window)), "zc_set_window")

    def record_tuples(self):
        """(kind_char, offset, size, rolling, sha1_hex) -- the oracle's format."""
        return [(KIND_CHAR[r["kind"]], int(r["offset"]), int(r["size"]), int(r["rolling"]),
                 bytes(r["sha1"]).hex()) for r in self.records()]

    def read_stream(self, offset, n):
        buf = np.empty(n, dtype=np.uint8)
        _check(self._L, self._ctx, self._L.zc_read_stream(self._ctx, offset, n, buf.ctypes.data),
               "zc_read_stream")
        return buf.tobytes()

    def stream_data(self, offset, n):
        """zc_stream_data: the bytes from the feed window's host mirror without a
        library-side copy (None when they are not in host memory)."""
        p = self._L.zc_stream_data(self._ctx, offset, n)
        return ctypes.string_at(p, n) if p else None

    def get_backup_data(self):
        """Serialized BackupInstruction stream; like the reference, only once."""
        if self._data_taken:
            raise _lib.ZcError("getBackupData() called twice")
        self._data_taken = True
        self._drain()
        return bytes(self._data)

    def stats(self):
        st = _lib.ZcStats()
        _check(self._L, self._ctx, self._L.zc_get_stats(self._ctx, ctypes.byref(st)), "zc_get_stats")
        return {name: getattr(st, name) for name, _ in _lib.ZcStats._fields_}

    def last_paths(self):
        """zc_last_stream_paths: the ZC_PATH_* bits of the last stream this
        context finished.  Raises ZcError before it has finished one."""
        bits = ctypes.c_uint32()
        _check(self._L, self._ctx, self._L.zc_last_stream_paths(self._ctx, ctypes.byref(bits)),
               "zc_last_stream_paths")
        return bits.value

    def scan_outputs(self):
        """zc_debug_scan_outputs (tests): what the scan left behind for the last
        stream, as a dict: n, blk (uint64 per 1 KiB span), wt_count / wt_side
        (per 256 KiB wave-tile), anchor_pos (uint64) / anchor_gear (uint32) in
        wave-tile order, keys (the scan-written grid keys, empty when they are
        no longer the scan's), max_tiles_per_wave.  Raises ZcError before any
        stream and after a stream through the feed window."""
        o = _lib.ZcScanOutputs()
        rc = self._L.zc_debug_scan_outputs(self._ctx, ctypes.byref(o))  # all capacities 0: the counts
        if rc == _lib.ZC_ERR_ARG and self._ctx:
            blk = np.zeros(o.n_blk, dtype=np.uint64)
            wt_count, wt_side = np.zeros(o.n_wt, dtype=np.uint32), np.zeros(o.n_wt, dtype=np.uint8)
            pos, gear = np.zeros(o.n_anchors, dtype=np.uint64), np.zeros(o.n_anchors, dtype=np.uint32)
            keys = np.zeros(o.n_keys, dtype=np.uint64)
            o.blk, o.blk_cap = blk.ctypes.data, blk.size
            o.wt_count, o.wt_side, o.wt_cap = wt_count.ctypes.data, wt_side.ctypes.data, wt_count.size
            o.anchor_pos, o.anchor_gear, o.anchor_cap = pos.ctypes.data, gear.ctypes.data, pos.size
            o.keys, o.key_cap = keys.ctypes.data, keys.size
            rc = self._L.zc_debug_scan_outputs(self._ctx, ctypes.byref(o))
        else:  # an empty stream needs no room
            blk = keys = pos = np.zeros(0, dtype=np.uint64)
            wt_count = gear = np.zeros(0, dtype=np.uint32)
            wt_side = np.zeros(0, dtype=np.uint8)
        _check(self._L, self._ctx, rc, "zc_debug_scan_outputs")
        return {"n": int(o.n), "blk": blk, "wt_count": wt_count, "wt_side": wt_side, "anchor_pos": pos,
                "anchor_gear": gear, "keys": keys, "max_tiles_per_wave": int(o.max_tiles_per_wave)}

    def scan_ms(self):
        """zc_stats.scan_ms of the last stream, without building the stats dict
        (bench.py reads it inside its timed loop)."""
        st = getattr(self, "_st_buf", None)
        if st is None:
            st = self._st_buf = _lib.ZcStats()
        _check(self._L, self._ctx, self._L.zc_get_stats(self._ctx, ctypes.byref(st)), "zc_get_stats")
        return st.scan_ms

    def reset(self):
        _check(self._L, self._ctx, self._L.zc_reset(self._ctx), "zc_reset")
        self._new_stream()

    def forget_stream_chunks(self):
        """Drop the index entries this context's streams added (Writer::add ->
        ChunkIndex::addChunk), keeping the seeded index: the next stream sees the
        index a fresh ZBackup instance loads (chunk_index.cc:26-79)."""
        _check(self._L, self._ctx, self._L.zc_forget_stream_chunks(self._ctx), "zc_forget_stream_chunks")

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


def fill_splitmix64(ptr, n, seed, device=0):
    """Seeded synthetic stream written straight into HBM (same bytes as the oracle's)."""
    L = _lib.load()
    rc = L.zc_fill_splitmix64(ctypes.c_void_p(ptr), n, seed, device)
    if rc != _lib.ZC_OK:
        raise _lib.ZcError(f"zc_fill_splitmix64 failed ({rc})")


class Sha256:
    """Whole-stream SHA-256 kept beside BackupCreator by the feed loop
    (sha256.hh:14-35; fed at zutils.cc:119, finished into BackupInfo.sha256 at
    zutils.cc:134).  Host-side, in libzchunk.so (zc_sha256_*)."""

    Size = 32

    def __init__(self):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        _check(self._L, None, self._L.zc_sha256_create(ctypes.byref(h)), "zc_sha256_create")
        self._h = h

    def add(self, data, size=None):
        """Sha256::add(data, size): bytes-like data, or a host address with its size."""
        if size is None:
            buf = memoryview(data).cast("B")
            arr = (ctypes.c_char * len(buf)).from_buffer_copy(buf) if buf.readonly else \
                (ctypes.c_char * len(buf)).from_buffer(buf)
            ptr, size = ctypes.addressof(arr), len(buf)
        else:
            ptr = data
        _check(self._L, None, self._L.zc_sha256_add(self._h, ptr, size), "zc_sha256_add")

    def finish(self):
        """Sha256::finish() -> the 32-byte digest; callable once, like SHA256_Final."""
        out = ctypes.create_string_buffer(32)
        _check(self._L, None, self._L.zc_sha256_finish(self._h, out), "zc_sha256_finish")
        return out.raw

    @property
    def uses_sha_extensions(self):
        return self._L.zc_sha256_impl(self._h) == 1

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.zc_sha256_destroy(h)
            self._h = None
