"""The reference of the xz tests: liblzma itself, through ctypes, and Python's
`lzma` (the same library) as the encoder.

  compress()            what Bundle::Creator's encoder call produces:
                        lzma_easy_encoder(6, LZMA_CHECK_CRC64), compression.cc:78-97
  buffer_decode()       lzma_stream_buffer_decode, as Bundle::Reader's decoder
                        is set up: memlimit UINT64_MAX, flags 0
  crc64()               lzma_crc64

`available()` is False where `lzma` does not import or liblzma.so.5 does not
load; tests that make streams skip with that reason, the committed fixtures
under tests/golden/xz/ serve the rest.
"""
import binascii
import ctypes
import json
import os
import struct

try:
    import lzma
    _L = ctypes.CDLL("liblzma.so.5")
    _L.lzma_stream_buffer_decode.restype = ctypes.c_int
    _L.lzma_stream_buffer_decode.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                             ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t]
    _L.lzma_crc64.restype = ctypes.c_uint64
    _L.lzma_crc64.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64]
except (ImportError, OSError) as e:  # pragma: no cover
    lzma, _L, _WHY = None, None, str(e)

LZMA_OK, LZMA_FORMAT_ERROR, LZMA_OPTIONS_ERROR, LZMA_DATA_ERROR, LZMA_BUF_ERROR = 0, 7, 8, 9, 10
# ZC_XZ_* (include/zchunk.h)
OK, E_FORMAT, E_UNSUPPORTED, E_HEADER, E_DATA, E_INPUT, E_OUTPUT, E_CHECK, E_BUDGET = range(9)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xz")


def available():
    return _L is not None


def why_not():
    return "liblzma is not here: " + _WHY if _L is None else ""


def compress(data, check=None, props=None, dict_size=None):
    """The reference's encoder call (preset 6, CRC64); `check` another check
    id, `props` = (lc, lp, pb) another property set."""
    check = lzma.CHECK_CRC64 if check is None else check
    if props is None and dict_size is None:
        return lzma.compress(bytes(data), check=check, preset=6)
    f = {"id": lzma.FILTER_LZMA2, "preset": 6}
    if props is not None:
        f.update(lc=props[0], lp=props[1], pb=props[2])
    if dict_size is not None:
        f["dict_size"] = dict_size
    return lzma.compress(bytes(data), format=lzma.FORMAT_XZ, check=check, filters=[f])


def buffer_decode(stream, cap):
    """(lzma_ret, in_pos, bytes): on an error in_pos is 0 and the bytes are empty."""
    stream = bytes(stream)
    mem = ctypes.c_uint64(2 ** 64 - 1)
    in_pos, out_pos = ctypes.c_size_t(0), ctypes.c_size_t(0)
    out = ctypes.create_string_buffer(max(cap, 1))
    ret = _L.lzma_stream_buffer_decode(ctypes.byref(mem), 0, None, stream, ctypes.byref(in_pos), len(stream), out,
                                       ctypes.byref(out_pos), cap)
    return ret, in_pos.value, out.raw[:out_pos.value] if ret == 0 else b""


def crc64(data):
    return _L.lzma_crc64(bytes(data), len(data), 0)


def crc32(data):
    return binascii.crc32(bytes(data)) & 0xffffffff


# ---- the container by hand: for the crafted cases ----

def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7f | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def parts(stream):
    """A one-block stream written by liblzma, cut at its container boundaries:
    dict(header, block_header, data, pad, check, index, footer)."""
    stream = bytes(stream)
    csz = {0: 0, 1: 4, 4: 8, 10: 32}[stream[7] & 15]
    hb = (stream[12] + 1) * 4
    back = (struct.unpack_from("<I", stream, len(stream) - 8)[0] + 1) * 4
    index = stream[-12 - back:-12]
    body_end = len(stream) - 12 - back
    # the index record: unpadded size, uncompressed size
    pos, vals = 2, []
    for _ in range(2):
        v, k = 0, 0
        while True:
            b = index[pos]
            pos += 1
            v |= (b & 0x7f) << (7 * k)
            k += 1
            if not b & 0x80:
                break
        vals.append(v)
    dlen = vals[0] - hb - csz
    d0 = 12 + hb
    return dict(header=stream[:12], block_header=stream[12:d0], data=stream[d0:d0 + dlen],
                pad=stream[d0 + dlen:body_end - csz], check=stream[body_end - csz:body_end], index=index,
                footer=stream[-12:], usize=vals[1])


def build(data, usize, payload_check, check_id=4, block_header=None, dict_prop=0x16):
    """A one-block stream around the LZMA2 bytes `data` (the end byte
    included) that decode to `usize` bytes with the check value `payload_check`
    (bytes)."""
    flags = bytes([0, check_id])
    header = b"\xfd7zXZ\0" + flags + struct.pack("<I", crc32(flags))
    if block_header is None:
        bh = bytes([2, 0, 0x21, 1, dict_prop, 0, 0, 0])
        block_header = bh + struct.pack("<I", crc32(bh))
    pad = b"\0" * (-len(data) % 4)
    rec = b"\0" + vli(1) + vli(len(block_header) + len(data) + len(payload_check)) + vli(usize)
    rec += b"\0" * (-len(rec) % 4)
    index = rec + struct.pack("<I", crc32(rec))
    tail = struct.pack("<I", len(index) // 4 - 1) + flags
    footer = struct.pack("<I", crc32(tail)) + tail + b"YZ"
    return header + block_header + data + pad + payload_check + index + footer


def chunks(data):
    """The LZMA2 chunks of a block's data: [(control byte, offset, bytes of the whole chunk)]."""
    out, pos = [], 0
    while True:
        c = data[pos]
        if c == 0:
            out.append((0, pos, 1))
            return out
        if c < 0x80:
            n = 3 + ((data[pos + 1] << 8 | data[pos + 2]) + 1)
        else:
            n = 5 + (1 if c >= 0xC0 else 0) + ((data[pos + 3] << 8 | data[pos + 4]) + 1)
        out.append((c, pos, n))
        pos += n


# ---- the committed fixtures ----

def golden():
    """[(name, stream bytes, payload bytes, manifest entry)] of tests/golden/xz/."""
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        man = json.load(f)
    out = []
    for e in man["streams"]:
        with open(os.path.join(GOLDEN, e["file"]), "rb") as f:
            stream = f.read()
        from tests import xz_inputs
        out.append((e["file"], stream, xz_inputs.payload(e["kind"], e["size"], e["seed"]).tobytes(), e))
    return out


GOLDEN_SET = (("text", 3000, 1, (3, 0, 2), 4), ("text", 60000, 2, (3, 0, 2), 4), ("random", 2049, 3, (3, 0, 2), 4),
              ("halfdup", 40000, 4, (3, 0, 2), 4), ("zeros", 65537, 5, (3, 0, 2), 4), ("period65", 5000, 6, (3, 0, 2), 1),
              ("period1", 274, 7, (0, 0, 0), 0), ("alphabet4", 20000, 8, (2, 2, 4), 4),
              ("text", 9000, 9, (4, 0, 2), 4), ("period300", 7000, 10, (0, 4, 0), 1), ("random", 0, 11, (3, 0, 2), 4),
              ("period64", 1, 12, (3, 0, 2), 4))


def write_golden():
    """Writes tests/golden/xz/ (run once: python -c 'from tests import xz_ref; xz_ref.write_golden()')."""
    from tests import xz_inputs
    os.makedirs(GOLDEN, exist_ok=True)
    man = []
    for kind, size, seed, props, check in GOLDEN_SET:
        name = "%s_%d_lc%d_lp%d_pb%d_check%d.xz" % ((kind, size) + props + (check,))
        stream = compress(xz_inputs.payload(kind, size, seed).tobytes(), check=check, props=props)
        assert len(stream) < 65536
        with open(os.path.join(GOLDEN, name), "wb") as f:
            f.write(stream)
        ctl = [c for c, _, _ in chunks(parts(stream)["data"])] if size else []
        man.append(dict(file=name, kind=kind, size=size, seed=seed, lc=props[0], lp=props[1], pb=props[2], check=check,
                        wide=props[0] + props[1] > 3 and any(c >= 0x80 for c in ctl)))
    with open(os.path.join(GOLDEN, "manifest.json"), "w") as f:
        json.dump({"streams": man}, f, indent=1)
        f.write("\n")
