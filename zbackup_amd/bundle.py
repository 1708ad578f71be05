"""Bundle writer offload: the host mirror of the reference's bundle path.

  ChunkStorage::Writer::add -> bundling rule          chunk_storage.cc:31-46
  Bundle::Creator::addChunk -> payload assembly       bundle.cc:30-36
  Bundle::Creator::write    -> lzo1x_1 compression    bundle.cc:120-151,
                               framing                compression.cc:435-466, 586-606

For the read side: `BundleCompressor.scatter` is Bundle::Reader::get for every
chunk a restore emits (bundle.cc:235-251), `parse_backup_data` the instruction
parse of restore() (backup_restorer.cc:38-107), `frame_info` the frame a
bundle's lzo1x stream is stored under (compression.cc:369-402).

For encrypted repositories: `BundleCompressor.seal` / `.unseal` are the bundle
file EncryptedFile::OutputStream writes and InputStream reads back
(encrypted_file.cc:20-392, bundle.cc:96-218), `aes_encrypt` / `aes_decrypt`
the AES-128-CBC under them (encryption.cc:17-95).

For LZMA bundles (the default compression method): `BundleDecompressor` is
Bundle::Reader's lzma_stream_decoder (compression.cc:99-107, bundle.cc:179-216)
for many bundles in one device call (zc_xz_decode).

`plan_bundles` is host bookkeeping; `BundleCompressor.gather` and `.compress`
run on the GPU through libzchunk.so (zc_bundle_gather / zc_lzo_compress);
there is no CPU fallback.  Device buffers are passed as raw pointers (e.g. a
torch uint8 tensor's data_ptr()).
"""
import ctypes

import numpy as np

from . import _lib
from .chunker import _check

MAX_PAYLOAD_SIZE = 0x200000  # bundle.max_payload_size default, zbackup.proto:88


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def plan_bundles(sizes, max_payload=MAX_PAYLOAD_SIZE):
    """Writer::add's rule over the sizes of the chunks index.addChunk accepted,
    in order: returns (bundle index of each chunk, number of bundles)."""
    L = _lib.load()
    sizes = _u64(sizes)
    out = np.zeros(len(sizes), dtype=np.uint32)
    nb = ctypes.c_size_t()
    rc = L.zc_bundle_plan(sizes.ctypes.data, len(sizes), int(max_payload), out.ctypes.data, ctypes.byref(nb))
    _check(L, None, rc, "zc_bundle_plan")
    return out, nb.value


def lzo_capacity(payload_size):
    """Output bytes to reserve for one framed payload (suggestOutputSize + 16)."""
    return int(_lib.load().zc_lzo_capacity(int(payload_size)))


LAYOUT_DTYPE = np.dtype([("status", "<i4"), ("reserved", "<u4"), ("header_off", "<u8"), ("header_len", "<u8"),
                         ("info_off", "<u8"), ("info_len", "<u8"), ("body_off", "<u8"), ("body_len", "<u8")])
assert LAYOUT_DTYPE.itemsize == ctypes.sizeof(_lib.ZcBundleLayout)


def bundle_file_size(prefix_len, body_len, keyed):
    """Bytes of a bundle file whose prefix (R + both messages) and body have
    these lengths (zc_bundle_file_size; host arithmetic)."""
    return int(_lib.load().zc_bundle_file_size(int(prefix_len), int(body_len), 1 if keyed else 0))


def _key16(key, none_ok=False):
    if key is None and none_ok:
        return None
    key = bytes(key) if key is not None else None
    if key is not None and len(key) != 16:
        raise ValueError("an AES-128 key is 16 bytes (EncryptionKey::getKey)")
    return key


def _bundle_files(prefixes, body_off, body_len, file_off):
    """(zc_bundle_file array, the prefixes' blob) of a seal call."""
    prefixes = [bytes(p) for p in prefixes]
    if not len(prefixes) == len(body_off) == len(body_len) == len(file_off):
        raise ValueError("seal: prefixes, body_off, body_len and file_off differ in length")
    files = (_lib.ZcBundleFile * max(len(prefixes), 1))()
    pos = 0
    for k, p in enumerate(prefixes):
        files[k] = _lib.ZcBundleFile(pos, len(p), int(body_off[k]), int(body_len[k]), int(file_off[k]))
        pos += len(p)
    return _Counted(files, len(prefixes)), b"".join(prefixes) or b"\0"


XZ_ENC_RESULT_DTYPE = np.dtype([("status", "<i4"), ("info", "<u4"), ("size", "<u8")])
assert XZ_ENC_RESULT_DTYPE.itemsize == ctypes.sizeof(_lib.ZcXzEncResult)


class _Counted:
    """A ctypes array passed by pointer with its element count as len()."""

    def __init__(self, arr, n):
        self._as_parameter_ = ctypes.cast(arr, ctypes.c_void_p)
        self._arr, self._n = arr, n

    def __len__(self):
        return self._n


class BundleCompressor:
    """GPU payload assembly + lzo1x_1 compression on a context of its own
    (or on a BackupCreator's, `ctx=bc._ctx`)."""

    def __init__(self, device=0, ctx=None):
        self._L = _lib.load()
        self._own = ctx is None
        if ctx is None:
            ctx = ctypes.c_void_p()
            rc = self._L.zc_create(ctypes.byref(ctx), 65536, device, 0)
            if rc != _lib.ZC_OK:
                raise _lib.ZcError(f"zc_create failed ({rc})")
        self._ctx = ctx

    def gather(self, d_src, src_off, sizes, d_payload):
        """Bundle::Creator::addChunk for every chunk: d_payload <- the extents
        d_src[src_off[i] ..+ sizes[i]) back to back."""
        src_off, sizes = _u64(src_off), _u64(sizes)
        rc = self._L.zc_bundle_gather(self._ctx, d_src, src_off.ctypes.data, sizes.ctypes.data, len(sizes), d_payload)
        _check(self._L, self._ctx, rc, "zc_bundle_gather")

    def compress(self, d_payload, pay_off, pay_size, d_out, out_off):
        """Framed lzo1x_1 of payload i to d_out + out_off[i]; returns the framed sizes."""
        pay_off, pay_size, out_off = _u64(pay_off), _u64(pay_size), _u64(out_off)
        out_size = np.zeros(len(pay_size), dtype=np.uint64)
        rc = self._L.zc_lzo_compress(self._ctx, d_payload, pay_off.ctypes.data, pay_size.ctypes.data, len(pay_size),
                                     d_out, out_off.ctypes.data, out_size.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_lzo_compress")
        return out_size

    def compress_host(self, payloads):
        """Host bytes in, framed bytes out (zc_lzo_compress_host), one call for all."""
        payloads = [bytes(p) for p in payloads]
        sizes = np.array([len(p) for p in payloads], dtype=np.uint64)
        pay_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if len(sizes) else sizes
        caps = np.array([lzo_capacity(int(s)) for s in sizes], dtype=np.uint64)
        out_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64) if len(caps) else caps
        src = np.frombuffer(b"".join(payloads) or b"\0", dtype=np.uint8)
        out = np.zeros(int(caps.sum()) or 1, dtype=np.uint8)
        out_size = np.zeros(len(sizes), dtype=np.uint64)
        rc = self._L.zc_lzo_compress_host(self._ctx, src.ctypes.data, pay_off.ctypes.data, sizes.ctypes.data,
                                          len(sizes), out.ctypes.data, out_off.ctypes.data, out_size.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_lzo_compress_host")
        return [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(out_off, out_size)]

    # ---- LZMA bundles (compression.cc:78-97): xz streams instead of framed lzo1x_1 ----

    def xz_capacity(self, n):
        """Room that always suffices for the xz stream of an n-byte payload (zc_xz_capacity)."""
        return int(self._L.zc_xz_capacity(int(n)))

    @staticmethod
    def _xz_judge(res):
        for k, r in enumerate(res):
            st = int(r["status"])
            if st != _lib.ZC_XZ_OK:
                raise _lib.ZcError(f"bundle {k}: {_lib.XZ_STATUS_NAMES.get(st, st)} (status {st})")

    def compress_xz(self, d_payload, pay_off, pay_size, d_out, out_off, check=4, out_cap=None, strict=True):
        """The xz stream (zc_xz_encode; check 4 = CRC64, what zbackup writes) of
        payload i to d_out + out_off[i], room out_cap[i] (None: xz_capacity of
        its size).  Returns the streams' sizes; raises ZcError naming the first
        bundle whose room was too small (strict=False: the XZ_ENC_RESULT_DTYPE
        array instead, the statuses the caller's to read)."""
        pay_off, pay_size, out_off = _u64(pay_off), _u64(pay_size), _u64(out_off)
        out_cap = _u64([self.xz_capacity(s) for s in pay_size] if out_cap is None else out_cap)
        if not len(pay_off) == len(pay_size) == len(out_off) == len(out_cap):
            raise ValueError("compress_xz: pay_off, pay_size, out_off and out_cap differ in length")
        res = np.zeros(len(pay_size), dtype=XZ_ENC_RESULT_DTYPE)
        rc = self._L.zc_xz_encode(self._ctx, d_payload, pay_off.ctypes.data, pay_size.ctypes.data, len(pay_size),
                                  d_out, out_off.ctypes.data, out_cap.ctypes.data, int(check), res.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_xz_encode")
        if not strict:
            return res
        self._xz_judge(res)
        return res["size"].copy()

    def compress_xz_host(self, payloads, check=4):
        """Host bytes in, xz streams out (zc_xz_encode_host), one call for all."""
        payloads = [bytes(p) for p in payloads]
        sizes = np.array([len(p) for p in payloads], dtype=np.uint64)
        pay_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if len(sizes) else sizes
        caps = np.array([(self.xz_capacity(int(s)) + 15) & ~15 for s in sizes], dtype=np.uint64)
        out_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64) if len(caps) else caps
        src = np.frombuffer(b"".join(payloads) or b"\0", dtype=np.uint8)
        out = np.zeros(int(caps.sum()) or 1, dtype=np.uint8)
        res = np.zeros(len(sizes), dtype=XZ_ENC_RESULT_DTYPE)
        rc = self._L.zc_xz_encode_host(self._ctx, src.ctypes.data, pay_off.ctypes.data, sizes.ctypes.data, len(sizes),
                                       out.ctypes.data, out_off.ctypes.data, caps.ctypes.data, int(check),
                                       res.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_xz_encode_host")
        self._xz_judge(res)
        return [out[int(o):int(o) + int(r["size"])].tobytes() for o, r in zip(out_off, res)]

    def xz_last_stats(self):
        """dict(match_ms, code_ms, check_ms, total_ms) of the last compress_xz, and
        its schedule (zc_xz_encode_last_schedule): batches, max_rounds, generation."""
        v = [ctypes.c_double() for _ in range(4)]
        rc = self._L.zc_xz_encode_last_stats(self._ctx, *[ctypes.byref(x) for x in v])
        _check(self._L, self._ctx, rc, "zc_xz_encode_last_stats")
        st = dict(zip(("match_ms", "code_ms", "check_ms", "total_ms"), (x.value for x in v)))
        b, r, g = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.zc_xz_encode_last_schedule(self._ctx, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g))
        _check(self._L, self._ctx, rc, "zc_xz_encode_last_schedule")
        st.update(batches=b.value, max_rounds=r.value, generation=g.value)
        return st

    def scatter(self, d_src, src_off, sizes, d_dst, dst_off):
        """The inverse of gather: extent i, d_src[src_off[i] ..+ sizes[i]), to
        d_dst + dst_off[i]; one extent may go to many places."""
        src_off, sizes, dst_off = _u64(src_off), _u64(sizes), _u64(dst_off)
        rc = self._L.zc_bundle_scatter(self._ctx, d_src, src_off.ctypes.data, sizes.ctypes.data, len(sizes), d_dst,
                                       dst_off.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_bundle_scatter")

    def adler32(self, d_base, off, length):
        """zlib adler32 (from 1) of each device range d_base[off[i] ..+ length[i])."""
        off, length = _u64(off), _u64(length)
        out = np.zeros(len(off), dtype=np.uint32)
        rc = self._L.zc_adler32(self._ctx, d_base, off.ctypes.data, length.ctypes.data, len(off), out.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_adler32")
        return out

    # ---- encrypted repositories (encryption.cc:17-95, encrypted_file.cc:239-392) ----

    def _aes(self, fn, what, key, src, in_off, length, iv, dst, out_off):
        in_off, length, out_off = _u64(in_off), _u64(length), _u64(out_off)
        if not len(in_off) == len(length) == len(out_off):
            raise ValueError(f"{what}: in_off, length and out_off differ in length")
        key = _key16(key)
        if iv is not None:
            iv = bytes(iv)
            if len(iv) != 16 * len(length):
                raise ValueError(f"{what}: iv must hold 16 bytes per chain")
        rc = fn(self._ctx, key, src, in_off.ctypes.data, length.ctypes.data, len(length), iv, dst, out_off.ctypes.data)
        _check(self._L, self._ctx, rc, what)

    def aes_encrypt(self, key, d_in, in_off, length, d_out, out_off, iv=None):
        """AES-128-CBC of chain i, d_in[in_off[i] ..+ length[i]), to d_out +
        out_off[i]; iv = 16 bytes per chain, None: the zero IV.  A chain may be
        encrypted in place (the same extent in and out)."""
        self._aes(self._L.zc_aes128_cbc_encrypt, "zc_aes128_cbc_encrypt", key, d_in, in_off, length, iv, d_out,
                  out_off)

    def aes_decrypt(self, key, d_in, in_off, length, d_out, out_off, iv=None):
        """The inverse, out of place only (no input extent may touch an output extent)."""
        self._aes(self._L.zc_aes128_cbc_decrypt, "zc_aes128_cbc_decrypt", key, d_in, in_off, length, iv, d_out,
                  out_off)

    def seal(self, key, prefixes, d_body, body_off, body_len, d_files, file_off):
        """Bundle::Creator::write's file for every bundle: prefixes[i] (host
        bytes: the 16 random bytes R when keyed, then the serialized
        BundleFileHeader and BundleInfo messages), the Adler-32s, the body
        d_body[body_off[i] ..+ body_len[i]) and the padding, assembled at
        d_files + file_off[i] and encrypted there (key None: no R, no padding,
        no cipher).  Returns the files' sizes."""
        files, blob = _bundle_files(prefixes, body_off, body_len, file_off)
        size = np.zeros(len(files), dtype=np.uint64)
        rc = self._L.zc_bundle_seal(self._ctx, _key16(key, none_ok=True), blob, files, len(files), d_body, d_files,
                                    size.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_bundle_seal")
        return size

    def seal_host(self, key, prefixes, bodies):
        """Host bytes in, each bundle's file bytes out (zc_bundle_seal_host), one call for all."""
        bodies = [bytes(b) for b in bodies]
        blen = [len(b) for b in bodies]
        boff = np.concatenate([[0], np.cumsum(blen)[:-1]]) if blen else []
        sizes = [bundle_file_size(len(p), n, key is not None) for p, n in zip(prefixes, blen)]
        cap = [(s + 15) // 16 * 16 for s in sizes]
        foff = np.concatenate([[0], np.cumsum(cap)[:-1]]) if cap else []
        files, blob = _bundle_files(prefixes, boff, blen, foff)
        body = np.frombuffer(b"".join(bodies) or b"\0", dtype=np.uint8)
        out = np.zeros(int(sum(cap)) or 1, dtype=np.uint8)
        size = np.zeros(len(files), dtype=np.uint64)
        rc = self._L.zc_bundle_seal_host(self._ctx, _key16(key, none_ok=True), blob, files, len(files),
                                         body.ctypes.data, out.ctypes.data, size.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_bundle_seal_host")
        assert [int(s) for s in size] == sizes
        return [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(foff, size)]

    def unseal(self, key, d_files, file_off, file_size, d_plain, plain_off):
        """Bundle::Reader's side: file i, d_files[file_off[i] ..+ file_size[i]),
        decrypted to d_plain + plain_off[i] and checked.  Returns a
        LAYOUT_DTYPE array: per bundle its status (ZC_BUNDLE_*) and where the
        header message, the info message and the body lie in its plaintext."""
        file_off, file_size, plain_off = _u64(file_off), _u64(file_size), _u64(plain_off)
        layout = np.zeros(len(file_off), dtype=LAYOUT_DTYPE)
        rc = self._L.zc_bundle_unseal(self._ctx, _key16(key, none_ok=True), d_files, file_off.ctypes.data,
                                      file_size.ctypes.data, len(file_off), d_plain, plain_off.ctypes.data,
                                      layout.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_bundle_unseal")
        return layout

    def unseal_host(self, key, files, strict=True):
        """Bundle files (host bytes) to (header bytes, info bytes, body bytes)
        each: what a caller hands to its protobuf decoder, to liblzo2 and then
        to the Restorer.  A file the reference would refuse raises ZcError
        with its status (strict=False: its entry is the status instead)."""
        files = [bytes(f) for f in files]
        size = np.array([len(f) for f in files], dtype=np.uint64)
        cap = (size + np.uint64(15)) // np.uint64(16) * np.uint64(16)
        off = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64) if len(files) else size
        src = np.zeros(int(cap.sum()) or 1, dtype=np.uint8)
        for o, f in zip(off, files):
            src[int(o):int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
        plain = np.zeros(len(src), dtype=np.uint8)
        layout = np.zeros(len(files), dtype=LAYOUT_DTYPE)
        rc = self._L.zc_bundle_unseal_host(self._ctx, _key16(key, none_ok=True), src.ctypes.data, off.ctypes.data,
                                           size.ctypes.data, len(files), plain.ctypes.data, off.ctypes.data,
                                           layout.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_bundle_unseal_host")
        out = []
        for k, (o, lay) in enumerate(zip(off, layout)):
            st = int(lay["status"])
            if st != _lib.ZC_BUNDLE_OK:
                if strict:
                    raise _lib.ZcError(f"bundle file {k}: {_lib.BUNDLE_STATUS_NAMES.get(st, st)} (status {st})")
                out.append(st)
                continue
            p = plain[int(o):int(o) + int(size[k])]
            out.append(tuple(p[int(lay[a]):int(lay[a]) + int(lay[b])].tobytes()
                             for a, b in (("header_off", "header_len"), ("info_off", "info_len"),
                                          ("body_off", "body_len"))))
        return out

    def aes_last_form(self):
        """The form of the CBC kernel this context launched last (zc_aes_last_form):
        ZC_AES_FORM_* bits, the lane kernel's chains per wave in bits 8-15.
        Raises ZcError when it has launched none."""
        form = ctypes.c_uint32()
        rc = self._L.zc_aes_last_form(self._ctx, ctypes.byref(form))
        _check(self._L, self._ctx, rc, "zc_aes_last_form")
        return form.value

    def last_stats(self):
        """(parse kernel ms, 48 KiB blocks) of the last compress()."""
        ms, blocks = ctypes.c_double(), ctypes.c_uint64()
        self._L.zc_lzo_last_stats(self._ctx, ctypes.byref(ms), ctypes.byref(blocks))
        return ms.value, blocks.value

    def close(self):
        if self._own and self._ctx:
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


XZ_RESULT_DTYPE = np.dtype([("status", "<i4"), ("info", "<u4"), ("decoded", "<u8"), ("consumed", "<u8")])
assert XZ_RESULT_DTYPE.itemsize == ctypes.sizeof(_lib.ZcXzResult)


class BundleDecompressor:
    """LZMA bundles decoded on the GPU (zc_xz_decode): Bundle::Reader's
    lzma_stream_decoder (compression.cc:99-107, bundle.cc:179-216) for many
    bundles in one call, on a context of its own or on another object's
    (`ctx=bc._ctx`).  There is no CPU fallback."""

    def __init__(self, device=0, ctx=None):
        self._L = _lib.load()
        self._own = ctx is None
        if ctx is None:
            ctx = ctypes.c_void_p()
            rc = self._L.zc_create(ctypes.byref(ctx), 65536, device, 0)
            if rc != _lib.ZC_OK:
                raise _lib.ZcError(f"zc_create failed ({rc})")
        self._ctx = ctx

    @staticmethod
    def _judge(res, in_size, sizes):
        """The strictness of Bundle::Reader: the stream good, the whole body
        used (where the reference's Adler-32 would fail otherwise), the
        payload of BundleInfo's size."""
        for k, r in enumerate(res):
            st = int(r["status"])
            if st != _lib.ZC_XZ_OK:
                raise _lib.ZcError(f"bundle {k}: {_lib.XZ_STATUS_NAMES.get(st, st)} (status {st}) after "
                                   f"{int(r['decoded'])} bytes")
            if int(r["consumed"]) != int(in_size[k]):
                raise _lib.ZcError(f"bundle {k}: the stream ends after {int(r['consumed'])} of the body's "
                                   f"{int(in_size[k])} bytes")
            if sizes is not None and int(r["decoded"]) != int(sizes[k]):
                raise _lib.ZcError(f"bundle {k}: {int(r['decoded'])} bytes decoded, its payload has {int(sizes[k])}")

    def decode(self, d_in, in_off, in_size, d_out, out_off, out_cap, strict=True):
        """Stream i, d_in[in_off[i] ..+ in_size[i]), to d_out + out_off[i] with
        room out_cap[i] = the payload's size.  Returns an XZ_RESULT_DTYPE
        array; raises ZcError naming the first bundle that is not exactly its
        payload (strict=False: the statuses are the caller's to read)."""
        in_off, in_size, out_off, out_cap = _u64(in_off), _u64(in_size), _u64(out_off), _u64(out_cap)
        if not len(in_off) == len(in_size) == len(out_off) == len(out_cap):
            raise ValueError("decode: in_off, in_size, out_off and out_cap differ in length")
        res = np.zeros(len(in_off), dtype=XZ_RESULT_DTYPE)
        rc = self._L.zc_xz_decode(self._ctx, d_in, in_off.ctypes.data, in_size.ctypes.data, len(in_off), d_out,
                                  out_off.ctypes.data, out_cap.ctypes.data, res.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_xz_decode")
        if strict:
            self._judge(res, in_size, out_cap)
        return res

    def decode_host(self, bodies, sizes, strict=True):
        """Host bytes in, payload bytes out (zc_xz_decode_host), one call for
        all; sizes[i] = the payload's size from BundleInfo."""
        bodies = [bytes(b) for b in bodies]
        if len(bodies) != len(sizes):
            raise ValueError("decode_host: bodies and sizes differ in length")
        in_size = np.array([len(b) for b in bodies], dtype=np.uint64)
        in_off = np.concatenate([[0], np.cumsum(in_size)[:-1]]).astype(np.uint64) if len(bodies) else in_size
        cap = _u64([int(s) for s in sizes])
        out_off = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64) if len(cap) else cap
        src = np.frombuffer(b"".join(bodies) or b"\0", dtype=np.uint8)
        out = np.zeros(int(cap.sum()) or 1, dtype=np.uint8)
        res = np.zeros(len(bodies), dtype=XZ_RESULT_DTYPE)
        rc = self._L.zc_xz_decode_host(self._ctx, src.ctypes.data, in_off.ctypes.data, in_size.ctypes.data,
                                       len(bodies), out.ctypes.data, out_off.ctypes.data, cap.ctypes.data,
                                       res.ctypes.data)
        _check(self._L, self._ctx, rc, "zc_xz_decode_host")
        if strict:
            self._judge(res, in_size, cap)
            return [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(out_off, cap)]
        return [out[int(o):int(o) + int(r["decoded"])].tobytes() if r["status"] == 0 else int(r["status"])
                for o, r in zip(out_off, res)], res

    # ---- host bodies in, payloads kept in HBM ----

    @staticmethod
    def stage_size(bodies):
        """Device bytes the bodies take when staged (each 16-byte aligned)."""
        return sum((len(b) + 15) & ~15 for b in bodies)

    def alloc(self, n):
        """A device buffer of n bytes on the context's device (free() it)."""
        p = ctypes.c_void_p()
        _check(self._L, self._ctx, self._L.zc_device_alloc(self._ctx, int(n), ctypes.byref(p)), "zc_device_alloc")
        return p.value

    def free(self, d_ptr):
        _check(self._L, self._ctx, self._L.zc_device_free(self._ctx, d_ptr), "zc_device_free")

    def upload(self, d_dst, data):
        buf = np.ascontiguousarray(np.frombuffer(memoryview(data), dtype=np.uint8))
        if buf.size:
            _check(self._L, self._ctx, self._L.zc_upload(self._ctx, d_dst, buf.ctypes.data, buf.size), "zc_upload")

    def decode_bodies(self, bodies, d_stage, d_out, out_off, sizes):
        """The compressed bodies (host bytes) cross to d_stage (stage_size(bodies)
        bytes of device memory) in one upload and decode to d_out + out_off[i];
        the payloads never touch the host.  Strict, as decode()."""
        bodies = [bytes(b) for b in bodies]
        in_size = [len(b) for b in bodies]
        in_off, pos = [], 0
        for n in in_size:
            in_off.append(pos)
            pos += (n + 15) & ~15
        img = np.zeros(max(pos, 1), dtype=np.uint8)
        for o, b in zip(in_off, bodies):
            img[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        if pos:
            self.upload(d_stage, img[:pos])
        return self.decode(d_stage, in_off, in_size, d_out, out_off, sizes)

    def last_stats(self):
        """dict(decode_ms, check_ms, total_ms, n_wide) of the last decode."""
        d, c, t, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        rc = self._L.zc_xz_last_stats(self._ctx, ctypes.byref(d), ctypes.byref(c), ctypes.byref(t), ctypes.byref(w))
        _check(self._L, self._ctx, rc, "zc_xz_last_stats")
        return dict(decode_ms=d.value, check_ms=c.value, total_ms=t.value, n_wide=w.value)

    def close(self):
        if self._own and self._ctx:
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


INSTRUCTION_DTYPE = np.dtype([("kind", "<u4"), ("id", "u1", (24,)), ("reserved", "<u4"), ("data_off", "<u8"),
                              ("size", "<u8")])
assert INSTRUCTION_DTYPE.itemsize == ctypes.sizeof(_lib.ZcInstruction)


def _host_check(L, rc, what):
    if rc != _lib.ZC_OK:
        msg = L.zc_last_error(None) or b""
        raise _lib.ZcError(f"{what} failed ({rc}): {msg.decode(errors='replace')}")


def parse_backup_data(data):
    """A BackupInstruction stream (BackupCreator.get_backup_data()) as a
    structured array (INSTRUCTION_DTYPE), one entry per chunk_to_emit
    (ZC_INSTR_CHUNK, `id`) and bytes_to_emit (ZC_INSTR_BYTES, the bytes are
    data[data_off ..+ size)), in the order restore() acts on them."""
    L = _lib.load()
    data = bytes(data)
    n = ctypes.c_size_t()
    out = np.zeros(len(data) // 2 + 1, dtype=INSTRUCTION_DTYPE)  # an entry takes at least two bytes
    rc = L.zc_parse_instructions(data, len(data), out.ctypes.data, len(out), ctypes.byref(n))
    _host_check(L, rc, "zc_parse_instructions")
    return out[:n.value].copy()


def frame_info(framed):
    """(payload size, compressed size) of a framed bundle's first 16 bytes;
    raises on a frame the decoder would refuse."""
    L = _lib.load()
    framed = bytes(framed)
    n, cz = ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.zc_lzo_frame_info(framed, len(framed), ctypes.byref(n), ctypes.byref(cz))
    if rc == _lib.ZC_LZO_E_FRAME:
        raise _lib.ZcError(f"zc_lzo_frame_info: bad frame ({rc}) in {len(framed)} bytes")
    _host_check(L, rc, "zc_lzo_frame_info")
    return n.value, cz.value
