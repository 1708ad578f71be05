"""Framed LZO1X bundles for the decoder tests, shared by the CPU check
(tests/test_unlzo.py -> tests/lzo/unlzo_core_check.cpp) and the GPU tests
(tests/test_gpu_unlzo.py): seeded payloads of tests/lzo_inputs.py compressed at
test time by liblzo2 (lzo1x_1 through the oracle's binding, lzo1x_999 -- whose
output holds the M1 forms lzo1x_1 never emits -- called here), framed as
zbackup frames them, and seeded mutations of such frames.  The library's own
lzo1x_decompress_safe gives every expected status."""
import ctypes
import struct

import numpy as np

from oracle import lzo_oracle
from tests.lzo_inputs import KINDS, payload

# the edges of the first-byte forms (17 + t, t < 4 / up to 238) and of the 255-runs
EDGE_SIZES = [0, 1, 2, 3, 4, 17, 18, 20, 21, 237, 238, 239, 240, 273, 274, 528, 49151, 49152, 49153, 49173, 98325,
              262144, 2097152]
COMPRESSORS = ("lzo1x_1", "lzo1x_999")
LZO1X_999_MEM_COMPRESS = 458752  # lzo1x.h: 14 * 16384 * sizeof(short)
E_FRAME, E_SIZE = -100, -101
ANY = 1000  # the check program's "whatever the library says"


def has_999():
    L = lzo_oracle.lzo_lib()
    return L is not None and hasattr(L, "lzo1x_999_compress")


def lzo1x_999(data):
    """lzo1x_999_compress(data) -> the raw LZO stream."""
    L = lzo_oracle.lzo_lib()
    n = len(data)
    out = ctypes.create_string_buffer(n + n // 16 + 64 + 3)
    olen = ctypes.c_size_t(len(out))
    wrk = ctypes.create_string_buffer(LZO1X_999_MEM_COMPRESS)
    src = ctypes.create_string_buffer(bytes(data), n) if n else ctypes.create_string_buffer(1)
    rc = L.lzo1x_999_compress(src, ctypes.c_size_t(n), out, ctypes.byref(olen), wrk)
    if rc != 0:
        raise RuntimeError(f"lzo1x_999_compress failed ({rc})")
    return out.raw[:olen.value]


def frame_stream(n, z):
    """zbackup's framing of stream z for a payload of n bytes (compression.cc:435-466)."""
    head = bytearray(b"ABCDEFGHIJKLMNOP")
    head[0:4] = struct.pack("<I", n)
    head[8:12] = struct.pack("<I", len(z))
    return bytes(head) + z


def frame(data, compressor="lzo1x_1"):
    data = bytes(data)
    return frame_stream(len(data), lzo_oracle.lzo1x_1(data) if compressor == "lzo1x_1" else lzo1x_999(data))


def library_decode(framed, out_cap=None):
    """The reference's reading of one framed bundle (compression.cc:369-402,
    472-490) with liblzo2: (status, the bytes decoded)."""
    if len(framed) < 16:
        return E_FRAME, b""
    n, = struct.unpack_from("<I", framed, 0)
    cz, = struct.unpack_from("<I", framed, 8)
    if 16 + cz > len(framed):
        return E_FRAME, b""
    cap = n if out_cap is None else min(n, int(out_cap))
    L = lzo_oracle.lzo_lib()
    out = ctypes.create_string_buffer(max(cap, 1))
    olen = ctypes.c_size_t(cap)
    src = ctypes.create_string_buffer(framed[16:16 + cz], max(cz, 1))
    rc = L.lzo1x_decompress_safe(src, ctypes.c_size_t(cz), out, ctypes.byref(olen), None)
    if rc != 0:
        return rc, out.raw[:olen.value]
    return (0 if olen.value == n else E_SIZE), out.raw[:olen.value]


def edge_cases():
    """(payload, framed) for every kind x edge size x compressor."""
    comps = COMPRESSORS if has_999() else COMPRESSORS[:1]
    out = []
    for i, (n, k) in enumerate((n, k) for n in EDGE_SIZES for k in KINDS):
        p = payload(k, n, 100 + i).tobytes()
        for c in comps:
            out.append((p, frame(p, c)))
    return out


def mutations(count, seed=1, size=20000):
    """`count` mutated frames of `size`-byte payloads: (framed, out_cap).  One
    bit flipped, one byte replaced, the stream cut at a random point, 1-3
    bytes appended inside csize, or the capacity one byte short."""
    rng = np.random.default_rng(seed)
    comps = COMPRESSORS if has_999() else COMPRESSORS[:1]
    bases = [frame(payload(k, size, 9000 + 10 * seed + j).tobytes(), c)
             for j, k in enumerate(KINDS) for c in comps]
    out = []
    for i in range(count):
        f = bytearray(bases[i % len(bases)])
        z = f[16:]
        how = int(rng.integers(0, 10))
        cap = size
        if how < 4:  # one bit
            z[int(rng.integers(0, len(z)))] ^= 1 << int(rng.integers(0, 8))
        elif how < 7:  # one byte
            z[int(rng.integers(0, len(z)))] = int(rng.integers(0, 256))
        elif how == 7:  # cut
            z = z[:int(rng.integers(0, len(z)))]
        elif how == 8:  # trailing bytes inside csize
            z = z + bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        else:  # the stream is whole, the output one byte short
            cap = size - 1
        out.append((frame_stream(size, bytes(z)), cap))
    return out


def frame_rule_cases():
    """(framed, out_cap, expected status) for the framing's own rules."""
    p = payload("text", 5000, 77).tobytes()
    f = frame(p)
    longer = bytearray(f)
    longer[0:4] = struct.pack("<I", len(p) + 1)  # the stream ends one byte before the frame's size
    shorter = bytearray(f)
    shorter[0:4] = struct.pack("<I", len(p) - 1)  # one byte more than the decoder's buffer: the library's -5
    over = bytearray(f)
    over[8:12] = struct.pack("<I", len(f) - 16 + 1)  # csize past the bytes given
    return [(b"", 0, E_FRAME), (f[:15], len(p), E_FRAME), (bytes(over), len(p), E_FRAME),
            (bytes(longer), len(p) + 1, E_SIZE), (bytes(shorter), len(p), -5),
            (f + b"unused input", len(p), 0),  # bytes after 16 + csize are not an error
            (f[:16 + 3], len(p), E_FRAME), (frame_stream(0, b""), 0, -4),  # an empty stream: input overrun
            (f, len(p), 0)]


def write_cases(path, cases):
    """The check program's input: (framed, out_cap, expect) per case."""
    with open(path, "wb") as fh:
        for framed, cap, expect in cases:
            fh.write(struct.pack("<iQI", expect, cap, len(framed)))
            fh.write(framed)
