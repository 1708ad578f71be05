"""Reference for the index-file tests: a pure-Python restatement of the format
IndexFile::Writer / Reader use (index_file.cc:18-76, message.cc:16-42,
zbackup.proto:107-145, encrypted_file.cc:130-209), with a writer and a strict
reader that returns the library's status codes.  It shares no code with the
library (the AES comes from tests/aes_ref.py).

  plaintext = [R: 16 random bytes, keyed only]
              varint32 len + FileHeader{version = 1}                 02 08 01
              pairs of  varint32 len + IndexBundleHeader{id}         1A 0A 18 <24>
                        varint32 len + BundleInfo                    repeated 0A <len> ChunkRecord
              varint32 0
              little-endian Adler-32 of everything before it
              [PKCS#7 padding of 1..16 bytes, keyed only]
  ChunkRecord = 0A 18 <24-byte id> and 10 <varint32 size>, either order

The strict rules (narrower than libprotobuf): a tag is one byte; each field at
most once; no other field; a varint32 has at most 5 bytes and fits 32 bits.
TRUNCATED is about the file's end only (a frame's length varint, the message it
announces, R, the Adler-32); whatever breaks inside a message's announced bytes
is BAD_MESSAGE or one of the id / version codes.  A file's status is the first
failure met front to back, the padding first, the Adler-32 last."""
import random
import struct
import zlib

import numpy as np

from tests import aes_ref

(OK, BAD_SIZE, BAD_PADDING, TRUNCATED, BAD_VERSION, BAD_MESSAGE, BAD_BUNDLE_ID, BAD_CHUNK_ID,
 BAD_ADLER) = range(9)
STATUS_NAMES = ["OK", "BAD_SIZE", "BAD_PADDING", "TRUNCATED", "BAD_VERSION", "BAD_MESSAGE", "BAD_BUNDLE_ID",
                "BAD_CHUNK_ID", "BAD_ADLER"]


class Bad(Exception):
    def __init__(self, status):
        Exception.__init__(self, STATUS_NAMES[status])
        self.status = status


# ---- writer ----

def varint(v, pad_to=0):
    """The varint of v; pad_to > its natural length gives a padded (legal) form."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    while len(out) < pad_to:
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def message(payload):
    return varint(len(payload)) + bytes(payload)


def chunk_record(cid, size, size_first=False):
    a, b = b"\x0a" + message(cid), b"\x10" + varint(size)
    return b + a if size_first else a + b


def bundle_info(records, size_first=False):
    """records: [(chunk id blob, size), ...]; size_first: True, False, or a
    list of bools the records cycle through."""
    out = bytearray()
    for k, (cid, size) in enumerate(records):
        sf = size_first[k % len(size_first)] if isinstance(size_first, (list, tuple)) else size_first
        out += b"\x0a" + message(chunk_record(cid, size, sf))
    return bytes(out)


def body(bundles, size_first=False):
    """FileHeader, the bundles [(bundle id, records), ...], the terminator."""
    out = bytearray(message(b"\x08\x01"))
    for bid, records in bundles:
        out += message(b"\x0a" + message(bid))
        out += message(bundle_info(records, size_first))
    out += b"\x00"
    return bytes(out)


def seal(body_bytes, key=None, r=None, trailing=b"", adler=True):
    """A whole file around serialized bytes: R, the Adler-32, padding, CBC."""
    if key is not None:
        assert r is not None and len(r) == 16
    p = (bytes(r) if key is not None else b"") + bytes(body_bytes)
    if adler:
        p += struct.pack("<I", zlib.adler32(p))
    p += bytes(trailing)
    return encrypt(pad(p), key) if key is not None else p


def pad(p):
    n = 16 - len(p) % 16
    return bytes(p) + bytes([n]) * n


def encrypt(p, key):
    return aes_ref.cbc_encrypt(key, bytes(16), p)


def write(bundles, key=None, r=None, size_first=False):
    return seal(body(bundles, size_first), key, r)


def file_size(body_len, keyed):
    return (16 + body_len + 4) // 16 * 16 + 16 if keyed else body_len + 4


# ---- strict reader ----

def _varint(p, pos, limit):
    """(value, pos) or raises 'end' / 'bad' as a string."""
    v = 0
    for k in range(5):
        if pos >= limit:
            raise EOFError
        b = p[pos]
        pos += 1
        v |= (b & 0x7f) << (7 * k)
        if not b & 0x80:
            if v > 0xffffffff:
                raise ValueError
            return v, pos
    raise ValueError


def _frame_len(p, pos, end):
    try:
        v, pos = _varint(p, pos, end)
    except EOFError:
        raise Bad(TRUNCATED)
    except ValueError:
        raise Bad(BAD_MESSAGE)
    if v > end - pos:
        raise Bad(TRUNCATED)
    return v, pos


def _inner_varint(p, pos, mend):
    try:
        return _varint(p, pos, mend)
    except (EOFError, ValueError):
        raise Bad(BAD_MESSAGE)


def _record(p, pos, mend):
    cid = size = None
    while pos < mend:
        tag = p[pos]
        pos += 1
        if tag == 0x0a:
            if cid is not None:
                raise Bad(BAD_MESSAGE)
            n, pos = _inner_varint(p, pos, mend)
            if n > mend - pos:
                raise Bad(BAD_MESSAGE)
            if n != 24:
                raise Bad(BAD_CHUNK_ID)
            cid = bytes(p[pos:pos + 24])
            pos += 24
        elif tag == 0x10:
            if size is not None:
                raise Bad(BAD_MESSAGE)
            size, pos = _inner_varint(p, pos, mend)
        else:
            raise Bad(BAD_MESSAGE)
    if cid is None or size is None:
        raise Bad(BAD_MESSAGE)
    return cid, size


def read_bundle_info(p, pos=0, end=None):
    """The records of one BundleInfo; raises Bad."""
    end = len(p) if end is None else end
    records = []
    while pos < end:
        if p[pos] != 0x0a:
            raise Bad(BAD_MESSAGE)
        n, pos = _inner_varint(p, pos + 1, end)
        if n > end - pos:
            raise Bad(BAD_MESSAGE)
        records.append(_record(p, pos, pos + n))
        pos += n
    return records


def read_plain(p, keyed):
    """[(bundle id, records), ...] of one plaintext; raises Bad."""
    n = len(p)
    if n == 0 or (keyed and n % 16):
        raise Bad(BAD_SIZE)
    pos, end = 0, n
    if keyed:
        k = p[-1]
        if not 1 <= k <= 16 or bytes(p[-k:]) != bytes([k]) * k:
            raise Bad(BAD_PADDING)
        end = n - k
        if end < 16:
            raise Bad(TRUNCATED)
        pos = 16
    ln, pos = _frame_len(p, pos, end)
    mend, version = pos + ln, None
    while pos < mend:
        if p[pos] != 0x08 or version is not None:
            raise Bad(BAD_MESSAGE)
        version, pos = _inner_varint(p, pos + 1, mend)
    if version is None:
        raise Bad(BAD_MESSAGE)
    if version != 1:
        raise Bad(BAD_VERSION)
    bundles = []
    while True:
        ln, pos = _frame_len(p, pos, end)
        if ln == 0:
            break
        mend = pos + ln
        if p[pos] != 0x0a:
            raise Bad(BAD_MESSAGE)
        k, pos = _inner_varint(p, pos + 1, mend)
        if k > mend - pos:
            raise Bad(BAD_MESSAGE)
        if k != 24:
            raise Bad(BAD_BUNDLE_ID)
        bid = bytes(p[pos:pos + 24])
        pos += 24
        if pos != mend:
            raise Bad(BAD_MESSAGE)
        ln, pos = _frame_len(p, pos, end)
        bundles.append((bid, read_bundle_info(p, pos, pos + ln)))
        pos += ln
    if end - pos < 4:
        raise Bad(TRUNCATED)
    if struct.unpack_from("<I", p, pos)[0] != zlib.adler32(bytes(p[:pos])):
        raise Bad(BAD_ADLER)
    return bundles


def read(data, key=None):
    """(status, bundles) of one file; bundles is [] unless the status is OK."""
    keyed = key is not None
    try:
        if keyed and (len(data) == 0 or len(data) % 16):
            raise Bad(BAD_SIZE)
        p = aes_ref.cbc_decrypt(key, bytes(16), bytes(data)) if keyed else bytes(data)
        return OK, read_plain(p, keyed)
    except Bad as e:
        return e.status, []


def arrays(per_file):
    """zc_gc_input's arrays from [bundles of file 0, bundles of file 1, ...]."""
    ids, sizes, bids, bf, xf = bytearray(), [], bytearray(), [0], [0]
    for bundles in per_file:
        for bid, records in bundles:
            bids += bid
            for cid, size in records:
                ids += cid
                sizes.append(size)
            bf.append(len(sizes))
        xf.append(len(bf) - 1)
    return dict(ids=np.frombuffer(bytes(ids), dtype=np.uint8).reshape(-1, 24),
                sizes=np.array(sizes, dtype=np.uint32),
                bundle_first=np.array(bf, dtype=np.uint64),
                bundle_ids=np.frombuffer(bytes(bids), dtype=np.uint8).reshape(-1, 24),
                index_first=np.array(xf, dtype=np.uint64))


def read_many(files, key=None):
    """What zc_index_load gives for the files: the arrays and one status per file."""
    res = [read(f, key) for f in files]
    out = arrays([b for _, b in res])
    out["status"] = np.array([s for s, _ in res], dtype=np.int32)
    return out


# ---- test material ----

def rand_id(rng):
    return bytes(rng.getrandbits(8) for _ in range(24))


def rand_bundles(rng, counts, sizes=None):
    """One bundle per entry of counts, with that many records."""
    out = []
    for c in counts:
        recs = [(rand_id(rng), sizes[rng.randrange(len(sizes))] if sizes else rng.randrange(1, 65537))
                for _ in range(c)]
        out.append((rand_id(rng), recs))
    return out


def crafted_bodies():
    """(name, body bytes, the status of the file around them): every rule of
    the strict reader broken once.  A name that starts with "cut:" is sealed
    without an Adler-32, so that the bytes end where the case says."""
    rng = random.Random(77)
    bid, cid = rand_id(rng), rand_id(rng)
    hdr, end = message(b"\x08\x01"), b"\x00"
    bh = message(b"\x0a" + message(bid))
    rec = chunk_record(cid, 300)
    prec = b"\x0a" + varint(24, 2) + cid + b"\x10" + varint(300, 5)  # the same with padded varints

    def info(*records):
        return message(b"".join(b"\x0a" + message(r) for r in records))

    good = hdr + bh + info(rec) + end
    c = [
        ("good", good, OK),
        ("padded varints", hdr + bh + message(b"\x0a" + varint(len(prec), 3) + prec) + end, OK),
        ("version 2", message(b"\x08\x02") + end, BAD_VERSION),
        ("version missing", message(b"") + end, BAD_MESSAGE),
        ("version twice", message(b"\x08\x01\x08\x01") + end, BAD_MESSAGE),
        ("version wire type", message(b"\x0a\x01\x01") + end, BAD_MESSAGE),
        ("version field 2", message(b"\x10\x01") + end, BAD_MESSAGE),
        ("version varint 6 bytes", message(b"\x08\x81\x80\x80\x80\x80\x00") + end, BAD_MESSAGE),
        ("version varint 33 bits", message(b"\x08\x81\x80\x80\x80\x10") + end, BAD_MESSAGE),
        ("version varint cut by its message", message(b"\x08\x81") + end, BAD_MESSAGE),
        ("frame varint 6 bytes", hdr + b"\x80\x80\x80\x80\x80\x00" + end, BAD_MESSAGE),
        ("frame varint 33 bits", hdr + b"\x80\x80\x80\x80\x10" + end, BAD_MESSAGE),
        ("cut: frame varint", hdr + b"\x80", TRUNCATED),
        ("header past the end", hdr + b"\x40\x0a\x18" + bid, TRUNCATED),
        ("info past the end", hdr + bh + b"\x7f" + rec, TRUNCATED),
        ("cut: no terminator", hdr + bh + info(rec), TRUNCATED),
        ("bundle id 23 bytes", hdr + message(b"\x0a" + message(bid[:23])) + info(rec) + end, BAD_BUNDLE_ID),
        ("bundle id 25 bytes", hdr + message(b"\x0a" + message(bid + b"x")) + info(rec) + end, BAD_BUNDLE_ID),
        ("bundle id past its message", hdr + message(b"\x0a\x30" + bid) + info(rec) + end, BAD_MESSAGE),
        ("bundle header tag", hdr + message(b"\x12" + message(bid)) + info(rec) + end, BAD_MESSAGE),
        ("bundle id twice", hdr + message((b"\x0a" + message(bid)) * 2) + info(rec) + end, BAD_MESSAGE),
        ("bundle header stranger", hdr + message(b"\x0a" + message(bid) + b"\x20\x01") + info(rec) + end,
         BAD_MESSAGE),
        ("info tag", hdr + bh + message(b"\x12" + message(rec)) + end, BAD_MESSAGE),
        ("record past its info", hdr + bh + message(b"\x0a\x40" + rec) + end, BAD_MESSAGE),
        ("record length cut", hdr + bh + message(b"\x0a") + end, BAD_MESSAGE),
        ("chunk id 23 bytes", hdr + bh + info(chunk_record(cid[:23], 5)) + end, BAD_CHUNK_ID),
        ("chunk id 25 bytes", hdr + bh + info(chunk_record(cid + b"y", 5)) + end, BAD_CHUNK_ID),
        ("chunk id past its record", hdr + bh + info(b"\x0a\x30" + cid + b"\x10\x05") + end, BAD_MESSAGE),
        ("chunk id missing", hdr + bh + info(b"\x10\x05") + end, BAD_MESSAGE),
        ("size missing", hdr + bh + info(b"\x0a" + message(cid)) + end, BAD_MESSAGE),
        ("empty record", hdr + bh + info(b"") + end, BAD_MESSAGE),
        ("chunk id twice", hdr + bh + info(b"\x0a" + message(cid) + b"\x0a" + message(cid) + b"\x10\x05") + end,
         BAD_MESSAGE),
        ("size twice", hdr + bh + info(b"\x10\x05\x10\x05\x0a" + message(cid)) + end, BAD_MESSAGE),
        ("record stranger", hdr + bh + info(rec + b"\x18\x01") + end, BAD_MESSAGE),
        ("size wire type", hdr + bh + info(b"\x0a" + message(cid) + b"\x12\x01\x05") + end, BAD_MESSAGE),
        ("size varint 6 bytes", hdr + bh + info(b"\x0a" + message(cid) + b"\x10\x80\x80\x80\x80\x80\x00") + end,
         BAD_MESSAGE),
        ("size varint 33 bits", hdr + bh + info(b"\x0a" + message(cid) + b"\x10\xff\xff\xff\xff\x1f") + end,
         BAD_MESSAGE),
        ("size varint cut", hdr + bh + info(b"\x0a" + message(cid) + b"\x10\x80") + end, BAD_MESSAGE),
        ("bad record after good ones", hdr + bh + info(rec, rec, chunk_record(cid[:5], 1), rec) + end, BAD_CHUNK_ID),
        ("bad bundle after a good one", hdr + bh + info(rec) + message(b"\x0a" + message(bid[:3])) + info(rec) + end,
         BAD_BUNDLE_ID),
        ("bad record before a cut", hdr + bh + info(b"\x10\x05") + b"\x7f", BAD_MESSAGE),
    ]
    return c


def bad_files(key=None, r=None):
    """(name, file bytes, status): the crafted bodies sealed, and the faults of the file itself."""
    keyed = key is not None
    out = [(n, seal(b, key, r, adler=not n.startswith("cut:")), s) for n, b, s in crafted_bodies()]
    good = crafted_bodies()[0][1]
    f = bytearray(seal(good, key, r))
    out.append(("empty file", b"", BAD_SIZE))
    if keyed:
        out.append(("15 bytes", bytes(f[:15]), BAD_SIZE))
        out.append(("33 bytes", bytes(f[:33]), BAD_SIZE))
        p = bytes(r) + good
        p += struct.pack("<I", zlib.adler32(p))
        n = 16 - len(p) % 16
        out.append(("pad byte 0", encrypt(p + bytes(n - 1) + b"\x00", key), BAD_PADDING))
        out.append(("pad byte 17", encrypt(p + bytes([17]) * n, key), BAD_PADDING))
        if n > 1:
            out.append(("pad bytes differ", encrypt(p + bytes([n ^ 1]) + bytes([n]) * (n - 1), key), BAD_PADDING))
        out.append(("only padding", encrypt(bytes([16]) * 16, key), TRUNCATED))
        out.append(("R and padding", encrypt(pad(bytes(r)), key), TRUNCATED))
        bad = bytearray(p)
        bad[30] ^= 0x40  # inside the first bundle's id: only the Adler-32 notices
        out.append(("Adler-32", encrypt(pad(bytes(bad)), key), BAD_ADLER))
    else:
        out.append(("no room for the Adler-32", bytes(f[:-2]), TRUNCATED))
        f[8] ^= 0x40
        out.append(("Adler-32", bytes(f), BAD_ADLER))
    return out


def mutations(base_body, key=None, r=None, count=300, seed=5):
    """Single-byte flips and truncations of one valid file.  For every other
    one the Adler-32 is recomputed (and the file padded and encrypted again)
    after the change, so the parser's statuses are reached, not only BAD_ADLER."""
    rng = random.Random(seed)
    keyed = key is not None
    plain = (bytes(r) if keyed else b"") + bytes(base_body)
    whole = plain + struct.pack("<I", zlib.adler32(plain))
    out = []
    for k in range(count):
        kind = rng.randrange(4)
        if k % 2 == 0:  # change the serialized bytes, then seal again
            b = bytearray(base_body)
            if kind == 0:
                b = b[:rng.randrange(len(b))]
            else:
                i = rng.randrange(len(b))
                b[i] = (b[i] ^ (1 << rng.randrange(8))) if kind < 3 else rng.randrange(256)
            out.append(seal(bytes(b), key, r))
        else:  # change the finished file
            f = bytearray(encrypt(pad(whole), key) if keyed else whole)
            if kind == 0:
                cut = rng.randrange(len(f))
                f = f[:cut // 16 * 16] if keyed and rng.randrange(2) else f[:cut]
            else:
                i = rng.randrange(len(f))
                f[i] ^= 1 << rng.randrange(8)
            out.append(bytes(f))
    return out
