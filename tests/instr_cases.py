"""The inputs of the device instruction parse's tests (test infrastructure
only): BackupInstruction streams built on chunker.serialize_instruction, each
case (name, stream bytes, tile) with tile the ZC_TEST_INSTR_TILE the case wants
(None: the default).  tests/test_instr_cases.py checks with the host parser
alone that the cases are what they claim; tests/test_gpu_instr.py runs them on
the device and tests/test_instr_core.py through the core's steps on the CPU."""
import ctypes

import numpy as np

from zbackup_amd.chunker import serialize_instruction as ser

T = 64            # the small tile of the geometry cases
T_DEFAULT = 8192  # zcin::kTileDefault
TILES = (64, 256, 4096, None)

# the host parser's eight failure texts (zc_parse_instructions)
TEXTS = ["truncated or overlong length varint",
         "instruction length past the end of the stream",
         "a field other than chunk_to_emit / bytes_to_emit",
         "truncated field length",
         "field past the end of its instruction",
         "chunk_to_emit is not a 24-byte chunk id",
         "chunk_to_emit twice in one instruction",
         "bytes_to_emit twice in one instruction"]

# test_parse_instructions_malformed's eleven streams (tests/test_unlzo.py)
MALFORMED = [
    ("truncated length varint", b"\x80"),
    ("overlong length varint", b"\x80\x80\x80\x80\x80\x01"),
    ("length past the end", b"\x05\x12\x01a"),
    ("another field number", b"\x03\x1a\x01a"),
    ("another wire type", b"\x02\x08\x01"),
    ("chunk blob of 23 bytes", bytes([25, 0x0a, 23]) + bytes(23)),
    ("chunk blob of 25 bytes", bytes([27, 0x0a, 25]) + bytes(25)),
    ("field past its instruction", b"\x03\x12\x05a" + b"bcde"),
    ("truncated field length", b"\x02\x12\x80"),
    ("a tag without a length", b"\x01\x12"),
    ("bad instruction after a good one", ser(raw=b"ok") + b"\x02\x12\x09"),
]


def varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([v & 0x7f | 0x80])
        v >>= 7
    return out + bytes([v])


def blob(k):
    return bytes((k * 7 + j) & 0xff for j in range(24))


def good(n, seed=0):
    """n good messages: chunks, short byte runs, both, empty ones."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        r = k % 5
        raw = rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        out.append(ser(chunk_blob=blob(k)) if r < 2 else ser(raw=raw) if r == 2
                   else ser(chunk_blob=blob(k), raw=raw) if r == 3 else ser())
    return b"".join(out)


def pad(length, seed=0):
    """Good messages of exactly `length` bytes in all."""
    rng = np.random.default_rng(seed)
    out, left, k = [], length, 0
    while left:
        k += 1
        if left >= 27 and rng.random() < 0.5:
            m = ser(chunk_blob=blob(k))
        elif left >= 3:
            m = ser(raw=bytes([k & 0xff]) * min(left - 3, int(rng.integers(0, 50))))
        else:
            m = ser()
        out.append(m)
        left -= len(m)
    data = b"".join(out)
    assert len(data) == length
    return data


def six_messages():
    body200 = bytes(np.random.default_rng(1).integers(0, 256, 200, dtype=np.uint8))
    return b"".join([ser(chunk_blob=blob(1)), ser(raw=b"tail bytes"), ser(chunk_blob=blob(2), raw=b"xyz"),
                     ser(raw=b""), ser(raw=body200), ser()])


def other_order():
    body = b"\x12\x02hi" + b"\x0a\x18" + blob(3)
    return bytes([len(body)]) + body


def basic():
    return [("six_messages", six_messages(), None), ("six_messages_T64", six_messages(), T),
            ("other_order", other_order(), None), ("both_orders", six_messages() + other_order() + six_messages(), T),
            ("empty", b"", None), ("one_message", ser(chunk_blob=blob(9)), None),
            ("one_message_T64", ser(chunk_blob=blob(9)), T)]


def malformed_placed():
    """Each malformed stream alone, straddling a tile edge, behind 1,000 good messages, at T = 64."""
    out = []
    front = good(1000, seed=3)
    for name, data in MALFORMED:
        out.append((f"{name}: alone", data, T))
        out.append((f"{name}: straddling", pad(3 * T - 1) + data, T))  # starts on a tile's last byte
        out.append((f"{name}: behind 1000", front + data, T))
    return out


def bytes_msg_of(total):
    """One bytes_to_emit message of exactly `total` bytes."""
    for k in range(max(total - 12, 0), total):
        m = ser(raw=bytes([0xee]) * k)
        if len(m) == total:
            return m
    raise AssertionError(total)


def geometry():
    out = [("ends_at_tile_end", pad(T - 27) + ser(chunk_blob=blob(1)) + good(5), T)]
    for vlen, raw_len in ((2, 200), (3, 20000), (5, 70)):
        # a message starting on a tile's last byte whose length varint crosses the edge
        body = b"\x12" + varint(raw_len) + bytes([0xab]) * raw_len
        lv = varint(len(body))
        if vlen == 5:  # a padded, still valid varint32: five bytes
            lv = bytes([len(body) & 0x7f | 0x80, (len(body) >> 7) | 0x80, 0x80, 0x80, 0x00])
            assert len(body) < 1 << 14
        assert len(lv) == vlen
        out.append((f"varint_{vlen}_across_edge", pad(2 * T - 1) + lv + body + good(7), T))
    for whole in (0, 1, 40):
        # a bytes_to_emit from the middle of a tile over `whole` whole tiles into the middle of another
        m = bytes_msg_of(T // 2 + whole * T + T // 2 - 10)
        out.append((f"bytes_over_{whole}_tiles", pad(T // 2) + m + good(9), T))
    for n in (T - 1, T, T + 1):
        out.append((f"stream_of_{n}", pad(n, seed=n), T))
    # tiles whose messages give 0, 1 and 2 entries each, side by side
    zero = b"\x00" * T
    one = b"".join(ser(raw=bytes(13)) for _ in range(4))          # 4 x 16 bytes
    two = b"".join(ser(chunk_blob=blob(k), raw=b"abc") for k in range(2))  # 2 x 32 bytes
    assert len(one) == T and len(two) == T
    out.append(("entries_0_1_2", zero + one + two + one + zero + two + two + zero, T))
    out.append(("scan_two_rounds", good(3000, seed=5), T))
    assert len(out[-1][1]) > 300 * T  # more than 256 tiles
    return out


def zeros():
    return [("zeros_T64", bytes(2 * T + 1), T), ("zeros_default", bytes(2 * T_DEFAULT + 1), None)]


def phantom_payloads():
    return ([("0x80 run", b"\x80" * 300), ("0xff run", b"\xff" * 300)] + MALFORMED
            + [("valid stream of 50", good(50, seed=11))])


def phantoms():
    """A bytes_to_emit whose payload looks like messages; good messages after it.  And the same cut so
    that the outer length is wrong."""
    out = []
    for name, payload in phantom_payloads():
        outer = ser(raw=payload)
        out.append((f"phantom {name}", good(3) + outer + good(20, seed=2), T))
        body = b"\x12" + varint(len(payload)) + payload
        cut = good(3) + varint(len(body) + 5) + body  # the outer length runs past the end
        out.append((f"phantom cut {name}", cut, T))
    return out


def all_named():
    return basic() + malformed_placed() + geometry() + zeros() + phantoms()


# ---- fuzz ----

def random_stream(rng, length):
    """(stream of about `length` bytes, marks): marks are (position, what) of
    every length varint's first byte ("len"), tag byte ("tag") and field length
    byte ("flen")."""
    out, marks, pos = [], [], 0
    while pos < length:
        r = rng.random()
        k = int(rng.integers(0, 1 << 30))
        if r < 0.35:
            m = ser(chunk_blob=blob(k))
        elif r < 0.45:
            m = ser(raw=b"")
        elif r < 0.62:
            m = ser(chunk_blob=blob(k), raw=bytes(24) if rng.random() < 0.6 else b"xy")
        elif r < 0.8:
            fill = int(rng.integers(0, 3))
            n = int(rng.integers(0, 300))
            m = ser(raw=(rng.integers(0, 256, n, dtype=np.uint8).tobytes() if fill == 0
                         else bytes([0x80]) * n if fill == 1 else bytes(n)))
        elif r < 0.85:
            m = ser(raw=rng.integers(0, 256, int(rng.integers(300, 6000)), dtype=np.uint8).tobytes())
        elif r < 0.9:
            m = other_order()
        else:
            m = ser()
        # the marks of this message, by a walk of its own bytes
        lv = 1
        while m[lv - 1] & 0x80:
            lv += 1
        marks.append((pos, "len"))
        q = lv
        while q < len(m):
            marks.append((pos + q, "tag"))
            marks.append((pos + q + 1, "flen"))
            fl, sh, q = 0, 0, q + 1
            while True:
                b = m[q]
                fl |= (b & 0x7f) << sh
                sh += 7
                q += 1
                if not b & 0x80:
                    break
            q += fl
        out.append(m)
        pos += len(m)
    return b"".join(out), marks


def mutate(rng, data, marks):
    d = bytearray(data)
    r = rng.random()
    if not d:
        return b"\x80" if r < 0.5 else b"\xff" * 7
    if r < 0.45 and marks:  # a length or tag byte
        pos, what = marks[int(rng.integers(0, len(marks)))]
        if what == "tag" and rng.random() < 0.5:
            d[pos] ^= 0x0a ^ 0x12  # the other field: a field twice, or a chunk id of another size
        elif what == "tag":
            d[pos] = [0x0a, 0x12, 0x1a, 0x08][int(rng.integers(0, 4))] if rng.random() < 0.8 else d[pos] ^ 0x10
        elif what == "flen":
            d[pos] = [0x80, 24, 23, d[pos] + 1 & 0xff, 0][int(rng.integers(0, 5))]
        else:
            d[pos] = [d[pos] ^ 1, d[pos] + 1 & 0xff, 0x80 | d[pos], 0][int(rng.integers(0, 4))]
    elif r < 0.65:  # any byte
        pos = int(rng.integers(0, len(d)))
        d[pos] ^= 1 << int(rng.integers(0, 8))
    elif r < 0.8:  # truncation
        del d[int(rng.integers(0, len(d))):]
    else:  # a spliced garbage run, at a message start half of the time
        pos = (marks[int(rng.integers(0, len(marks)))][0] if marks and rng.random() < 0.5
               else int(rng.integers(0, len(d) + 1)))
        run = bytes([[0x80, 0xff, 0x00, 0x12][int(rng.integers(0, 4))]]) * int(rng.integers(1, 40))
        d[pos:pos] = run
    return bytes(d)


def fuzz(n_streams=200, n_mutants=2000, seed=20240):
    """(streams, mutants): lists of (name, data, tile)."""
    rng = np.random.default_rng(seed)
    streams, marks = [], []
    for k in range(n_streams):
        # lengths from 0 to 70,000, most of them short so that the suite stays quick
        length = 0 if k == 0 else 70000 if k == 1 else int(70000 * rng.random() ** 4)
        data, mk = random_stream(rng, length)
        streams.append((f"fuzz {k}", data, TILES[int(rng.integers(0, 4))]))
        marks.append(mk)
    mutants = []
    for k in range(n_mutants):
        j = int(rng.integers(0, n_streams))
        mutants.append((f"mutant {k} of {j}", mutate(rng, streams[j][1], marks[j]), TILES[int(rng.integers(0, 4))]))
    return streams, mutants


# ---- the host parser, the reference of every test ----

def host_parse(lib, data):
    """("ok", the entries as bytes, 48 each) or ("error", the text after the function's name)."""
    from zbackup_amd.bundle import INSTRUCTION_DTYPE
    n = ctypes.c_size_t()
    out = np.zeros(len(data) // 2 + 1, dtype=INSTRUCTION_DTYPE)
    rc = lib.zc_parse_instructions(data, len(data), out.ctypes.data, len(out), ctypes.byref(n))
    if rc != 0:
        msg = lib.zc_last_error(None).decode()
        assert msg.startswith("zc_parse_instructions: ")
        return "error", msg[len("zc_parse_instructions: "):]
    return "ok", out[:n.value].tobytes()
