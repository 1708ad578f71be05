"""The xz encoder's tests: the cases, and the host core (zc_xzenc_core.h through
tests/xzenc/xzenc_core_check.cpp) as a program that encodes them.  The CPU test
builds it under ASan + UBSan; the GPU tests build it plain and compare the
device's streams with its byte for byte."""
import json
import os
import struct
import subprocess

import numpy as np

from tests import xz_inputs as XI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "xzenc")
KINDS = ("literal", "matched_literal", "match", "short_rep", "rep0", "rep1", "rep2", "rep3", "len_low", "len_mid",
         "len_high", "dist_slot_only", "dist_special", "dist_direct", "stored_chunk", "lzma_chunk")
CHUNK = 65536


def capacity(n):
    return 32 if n == 0 else n + 3 * ((n + CHUNK - 1) // CHUNK) + 64


def sanitizers_link(tmp):
    src = tmp / "trivial.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp / "trivial")],
                          capture_output=True).returncode == 0


def build_exe(tmp, sanitize):
    exe = str(tmp / ("xzenc_core_check_san" if sanitize else "xzenc_core_check"))
    cmd = ["g++", "-O1" if sanitize else "-O2", "-g", "-Wall", "-Werror", "-std=c++17",
           "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"), os.path.join(ROOT, "tests", "xzenc", "xzenc_core_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run(exe, tmp_path, cases, name="enc"):
    """cases: [(check id, payload bytes)].  The program aborts on any fault of
    the core.  Returns ([(status, stored chunks, stream)], {kind: count})."""
    cin, cout = tmp_path / (name + ".cases"), tmp_path / (name + ".streams")
    with open(cin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for check, data in cases:
            fh.write(struct.pack("<II", check, len(data)) + data)
    out = subprocess.run([exe, str(cin), str(cout)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert lines[-1] == f"ok {len(cases)}"
    kinds = dict(zip(KINDS, (int(x) for x in lines[-2].split()[1:])))
    res = []
    with open(cout, "rb") as fh:
        for (check, data), ln in zip(cases, lines):
            status, stored, size = struct.unpack("<iIQ", fh.read(16))
            stream = fh.read(size)
            assert len(stream) == size
            assert [int(x) for x in ln.split()] == [status, stored, size, capacity(len(data))]
            res.append((status, stored, stream))
        assert fh.read() == b""
    os.remove(cin)
    os.remove(cout)
    return res, kinds


# ---- the schedule: zc_xzenc.hip's cutting rule and generations, restated ----

GEN_END = 0xffffffff  # a launch whose last generation would reach this clears the tables first


def batch_ends(sizes, room):
    """Where xzenc_encode cuts a call: a batch is the longest run of payloads whose
    sizes fit pool = max(largest payload, room).  The ends, one per batch."""
    if not len(sizes):
        return []
    pool, ends, in_batch = max(max(sizes), 1, room), [], 0
    for i, n in enumerate(sizes):
        if in_batch and in_batch + n > pool:
            ends.append(i)
            in_batch = 0
        in_batch += n
    return ends + [len(sizes)]


def rounds_of(count, cus):
    """Payloads the busiest wave of a launch over `count` payloads takes."""
    slots = 4 * max(1, min((count + 3) // 4, 2 * cus))
    return (count + slots - 1) // slots


def generations(ends, cus, gen):
    """The generation after a call cut at `ends` that began at `gen`, and the
    batches before which the tables were cleared (none regrown on the way)."""
    cleared, lo = [], 0
    for b, hi in enumerate(ends):
        r = rounds_of(hi - lo, cus)
        if gen + r >= GEN_END:
            cleared.append(b)
            gen = 0
        gen += r
        lo = hi
    return gen, cleared


# ---- the cases ----

def _p(kind, n, seed):
    return XI.payload(kind, n, seed).tobytes()


def grid_cases():
    """Every kind of tests/xz_inputs.py at every size of XI.SIZES (CRC64), and
    check ids 0 and 1 on a subset: [(name, check, payload)]."""
    out = []
    for kind in XI.KINDS:
        for n in XI.SIZES:
            out.append((f"{kind}_{n}", 4, _p(kind, n, 7)))
    for check in (0, 1):
        for kind, n in (("text", 3000), ("random", 500), ("zeros", 1), ("halfdup", 70000), ("random", 0)):
            out.append((f"{kind}_{n}_check{check}", check, _p(kind, n, 3)))
    return out


def chunk_rule_cases():
    """[(name, check, payload)]; what each reaches is asserted by the test
    that uses it (with xz_ref.chunks)."""
    rnd = _p("random", 3 * CHUNK, 21)
    return [("text_3_chunks", 4, _p("text", 3 * CHUNK - 5, 11)),
            ("random_two_stored", 4, rnd[:65537]),
            ("random_then_text", 4, rnd[:CHUNK] + _p("text", 30000, 12)),
            ("text_then_random", 4, _p("text", CHUNK, 13) + rnd[:20000]),
            ("random_text_random_text", 4, rnd[:CHUNK] + _p("text", CHUNK, 14) + rnd[CHUNK:2 * CHUNK] + _p("text", 999, 15))]


def match_form_cases():
    out = []
    for per in (1, 2, 3, 63, 64, 65, 300):
        out.append((f"period{per}_5000", 4, _p(f"period{per}", 5000, 31)))
    rng = np.random.default_rng(32)
    for run_len in (273, 274, 546):
        # a run of equal bytes between random bytes that do not continue it
        body = np.full(run_len, 0x41, dtype=np.uint8)
        left = rng.integers(0, 64, 100, dtype=np.uint8)
        right = rng.integers(0, 64, 100, dtype=np.uint8)
        out.append((f"run{run_len}", 4, np.concatenate([left, body, right]).tobytes()))
    blk = rng.integers(0, 256, 100000, dtype=np.uint8).tobytes()
    mid = _p("text", (1 << 20) - 100000, 33)
    out.append(("far_copy_1mib", 4, blk + mid + blk))
    # four distances in turn, each repeated with a different byte behind it: rep1, rep2, rep3
    words = [rng.integers(0, 256, 40, dtype=np.uint8).tobytes() for _ in range(4)]
    seq = b"".join(words)
    order = rng.integers(0, 4, 400)
    seq += b"".join(words[k] + bytes([int(rng.integers(0, 256))]) for k in order)
    out.append(("four_sources", 4, seq))
    return out


def all_cases():
    return grid_cases() + chunk_rule_cases() + match_form_cases()


# ---- the committed fixtures: lengths and CRC64s of the host core's streams ----

GOLDEN_SET = (("text", 3000, 1, 4), ("text", 70000, 2, 4), ("random", 2049, 3, 4), ("halfdup", 40000, 4, 4),
              ("zeros", 65537, 5, 4), ("period65", 5000, 6, 1), ("period1", 274, 7, 0), ("alphabet4", 20000, 8, 4),
              ("random", 65537, 9, 4), ("period300", 7000, 10, 1), ("random", 0, 11, 4), ("period64", 1, 12, 4),
              ("halfdup", 200000, 13, 4))


def crc64(data):
    """CRC-64/XZ, bytewise (no liblzma needed)."""
    global _T64
    try:
        t = _T64
    except NameError:
        t = []
        for i in range(256):
            r = i
            for _ in range(8):
                r = (r >> 1) ^ (0xC96C5795D7870F42 if r & 1 else 0)
            t.append(r)
        _T64 = t
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def golden():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)["streams"]


def golden_cases():
    return [(e["check"], _p(e["kind"], e["size"], e["seed"])) for e in golden()]


def write_golden(exe, tmp_path):
    """Writes tests/golden/xzenc/manifest.json from the host core."""
    cases = [(check, _p(kind, size, seed)) for kind, size, seed, check in GOLDEN_SET]
    res, _ = run(exe, tmp_path, cases, "golden")
    man = [dict(kind=kind, size=size, seed=seed, check=check, stream_len=len(s), stream_crc64="%016x" % crc64(s),
                stored_chunks=stored)
           for (kind, size, seed, check), (_, stored, s) in zip(GOLDEN_SET, res)]
    os.makedirs(GOLDEN, exist_ok=True)
    with open(os.path.join(GOLDEN, "manifest.json"), "w") as f:
        json.dump({"streams": man}, f, indent=1)
        f.write("\n")
