"""zc_xz_core.h -- the decoder zc_xz.hip's kernels run -- compiled for the host
under ASan + UBSan with a main of its own (tests/xz/xz_core_check.cpp) and held
to liblzma (tests/xz_ref.py): valid streams of every payload kind, edge size
and property set; single-bit flips and truncations; crafted streams with the
exact status.  No GPU."""
import os
import random
import struct
import subprocess

import pytest

from tests import xz_inputs as XI
from tests import xz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lzma = pytest.mark.skipif(not R.available(), reason=R.why_not())


def _sanitizers_link(tmp):
    src = tmp / "trivial.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp / "trivial")],
                          capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """The check program under ASan + UBSan.  Where not even a trivial program
    links with them the tests that run it skip, with that reason: without the
    sanitizers the memory-safety half of what they check would be missing."""
    tmp = tmp_path_factory.mktemp("xz_core")
    exe = str(tmp / "xz_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "xz", "xz_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not _sanitizers_link(tmp):
        pytest.skip("g++ does not link a program under -fsanitize=address,undefined here")
    out = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe, True


def case(stream, cap, lzma_ret, in_pos, expect, want=-1):
    return (bytes(stream), cap, lzma_ret, in_pos, bytes(expect), want)


def ref_case(stream, cap, want=-1):
    """A case whose expectation is liblzma's answer."""
    ret, in_pos, data = R.buffer_decode(stream, cap)
    return case(stream, cap, ret, in_pos, data, want)


def run_cases(exe, tmp_path, cases, name="cases.bin"):
    """Runs the cases; the program aborts on any disagreement.  Returns
    [(status, decoded, consumed, wide)]."""
    path = tmp_path / name
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for stream, cap, ret, in_pos, expect, want in cases:
            fh.write(struct.pack("<iiQQI", ret, want, cap, in_pos, len(stream)) + stream)
            fh.write(struct.pack("<I", len(expect)) + expect)
    out = subprocess.run([exe[0], str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert lines[-1] == f"ok {len(cases)}"
    os.remove(path)
    return [tuple(int(x) for x in ln.split()) for ln in lines[:-1]]


def test_crc_constants_and_combine(check_exe):
    out = subprocess.run([check_exe[0]], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-4000:]


def test_committed_streams_decode(check_exe, tmp_path):
    """The fixtures need no liblzma: the payload comes from its seed."""
    gold = R.golden()
    assert len(gold) >= 8
    cases = []
    for _, stream, data, _ in gold:
        cases.append(case(stream, len(data), 0, len(stream), data, R.OK))
        if data:
            cases.append(case(stream, len(data) - 1, -1, 0, b"", R.E_OUTPUT))
    res = run_cases(check_exe, tmp_path, cases)
    wide = {e["file"]: bool(e.get("wide")) for _, _, _, e in gold}
    k = 0
    for name, stream, data, _ in gold:
        assert bool(res[k][3]) == wide[name], name
        k += 2 if data else 1


@needs_lzma
@pytest.mark.parametrize("props", XI.PROPS, ids=lambda p: "lc%d_lp%d_pb%d" % p)
def test_valid_streams_every_kind_size_and_property_set(check_exe, tmp_path, props):
    cases = []
    for kind in XI.KINDS:
        for n in XI.SIZES:
            data = XI.payload(kind, n, 7).tobytes()
            stream = R.compress(data, props=props)
            for cap, want in ((n + 100, R.OK), (n, R.OK), (n - 1, R.E_OUTPUT)):
                if cap < 0:
                    continue
                c = ref_case(stream, cap, want)
                assert c[2] == (R.LZMA_OK if want == R.OK else R.LZMA_BUF_ERROR), (kind, n, cap, c[2])
                if want == R.OK:
                    assert c[4] == data and c[3] == len(stream)
                cases.append(c)
    res = run_cases(check_exe, tmp_path, cases)
    need_wide = props[0] + props[1] > 3
    # a stream without an LZMA chunk (no block, or stored chunks alone) never asks for the wide form
    assert any(r[3] for r in res) == need_wide
    if not need_wide:
        assert not any(r[3] for r in res)


@needs_lzma
def test_chunk_limits(check_exe, tmp_path):
    """A second LZMA chunk without reset (the compressed form passes 64 KiB),
    the 2 MiB chunk limit, and stored chunks followed by an LZMA chunk."""
    cases, seen = [], set()
    n = 300000
    while True:  # a text-like size whose compressed form passes 64 KiB
        data = XI.payload("text", n, 11).tobytes()
        stream = R.compress(data)
        ctl = [c for c, _, _ in R.chunks(R.parts(stream)["data"])]
        if any(0x80 <= c < 0xA0 for c in ctl[1:]):
            break
        n *= 2
        assert n < 8 << 20
    seen.update(ctl)
    cases.append(ref_case(stream, len(data), R.OK))
    data = bytes((2 << 20) + 1)
    stream = R.compress(data)
    ctl = [c for c, _, _ in R.chunks(R.parts(stream)["data"])]
    assert ctl[0] == 0xFF and 0x80 <= ctl[1] < 0xA0, ctl
    cases.append(ref_case(stream, len(data), R.OK))
    data = XI.payload("halfdup", 2 << 20, 5).tobytes()
    stream = R.compress(data)
    ctl = [c for c, _, _ in R.chunks(R.parts(stream)["data"])]
    assert ctl[0] == 1 and 2 in ctl and any(c >= 0xC0 for c in ctl), ctl
    cases.append(ref_case(stream, len(data), R.OK))
    for c in cases:
        assert c[2] == 0
    run_cases(check_exe, tmp_path, cases)


@needs_lzma
@pytest.mark.parametrize("check", (0, 1, 4))
def test_check_ids(check_exe, tmp_path, check):
    cases = []
    for kind, n in (("text", 3000), ("random", 500), ("zeros", 1), ("halfdup", 70000)):
        stream = R.compress(XI.payload(kind, n, 3).tobytes(), check=check)
        assert stream[7] == check
        cases.append(ref_case(stream, n, R.OK))
    stream = R.compress(b"", check=check)
    assert len(stream) == 32
    cases.append(ref_case(stream, 0, R.OK))
    run_cases(check_exe, tmp_path, cases)


MUTANT_BASES = (("text", 1500, (3, 0, 2), 4), ("text", 4000, (3, 0, 2), 0), ("text", 2500, (0, 0, 0), 1),
                ("alphabet4", 3000, (2, 2, 4), 4), ("alphabet4", 2000, (4, 0, 2), 0), ("period65", 900, (3, 0, 2), 4),
                ("period3", 700, (0, 4, 0), 0), ("halfdup", 600, (3, 0, 2), 4), ("random", 300, (3, 0, 2), 0),
                ("zeros", 5000, (3, 1, 2), 1), ("period300", 2000, (3, 0, 2), 0), ("text", 600, (3, 0, 2), 4))


def mutant_cases(flips, cuts, seed=20):
    """Single-bit flips at seeded positions and truncations of each base stream, with liblzma's answer."""
    rng = random.Random(seed)
    cases = []
    for kind, n, props, check in MUTANT_BASES:
        stream = R.compress(XI.payload(kind, n, 9).tobytes(), check=check, props=props)
        for _ in range(flips):
            m = bytearray(stream)
            bit = rng.randrange(8 * len(m))
            m[bit >> 3] ^= 1 << (bit & 7)
            cases.append(ref_case(m, n))
        for _ in range(cuts):
            cases.append(ref_case(stream[:rng.randrange(len(stream))], n))
    return cases


@needs_lzma
def test_mutants_agree_with_liblzma(check_exe, tmp_path):
    """300 single-bit flips and 50 truncations of each of 12 streams: the core
    accepts exactly what liblzma accepts, with the same bytes; otherwise its
    status is non-zero and the walk ended within its trip count (the program
    aborts on ZC_XZ_E_BUDGET)."""
    cases, rets = mutant_cases(300, 50), {}
    for c in cases:
        rets[c[2]] = rets.get(c[2], 0) + 1
    print("liblzma on the mutants:", sorted(rets.items()))
    for cls in (R.LZMA_FORMAT_ERROR, R.LZMA_DATA_ERROR, R.LZMA_BUF_ERROR):
        assert rets.get(cls, 0) >= 1, rets
    res = run_cases(check_exe, tmp_path, cases)
    assert len(res) == 12 * 350
    for c, r in zip(cases, res):
        assert (r[0] == 0) == (c[2] == 0)
        assert r[0] != R.E_BUDGET


def _flip(b, at, mask=1):
    m = bytearray(b)
    m[at] ^= mask
    return bytes(m)


def crafted_cases():
    """Hand-made streams with liblzma's answer and the exact status wanted
    (also run on the device by tests/test_gpu_xz.py)."""
    data = XI.payload("text", 1000, 1).tobytes()
    stream = R.compress(data)
    p = R.parts(stream)
    assert p["header"] + p["block_header"] + p["data"] + p["pad"] + p["check"] + p["index"] + p["footer"] == stream
    assert p["block_header"][:8] == bytes([2, 0, 0x21, 1, 0x16, 0, 0, 0]) and stream[6:8] == b"\0\4"
    assert R.build(p["data"], len(data), p["check"]) == stream  # the builder writes what liblzma writes
    n = len(data)
    cases = []

    def add(s, want, cap=n, ret=None):
        c = ref_case(s, cap, want)
        if ret is not None:
            assert c[2] == ret, (want, c[2], ret)
        cases.append(c)

    add(_flip(stream, 0), R.E_FORMAT, ret=R.LZMA_FORMAT_ERROR)
    add(_flip(stream, 5), R.E_FORMAT, ret=R.LZMA_FORMAT_ERROR)
    i_check = len(stream) - 12 - len(p["index"]) - 8
    for at in (8, 12 + 8, len(stream) - 12 - 1, len(stream) - 12):  # header, block header, index, footer CRC32
        add(_flip(stream, at), R.E_HEADER, ret=R.LZMA_DATA_ERROR)
    add(_flip(stream, len(stream) - 1), R.E_HEADER, ret=R.LZMA_DATA_ERROR)  # 'Z'
    add(_flip(stream, i_check), R.E_CHECK, ret=R.LZMA_DATA_ERROR)
    add(_flip(stream, i_check + 7, 0x80), R.E_CHECK, ret=R.LZMA_DATA_ERROR)
    cut = 0
    for part in ("header", "block_header", "data", "pad", "check", "index"):
        add(stream[:cut], R.E_INPUT)
        cut += len(p[part])
        add(stream[:cut - 1], R.E_INPUT)
    add(stream[:cut], R.E_INPUT)
    add(stream[:-1], R.E_INPUT)
    # LZMA2's rules
    c0 = R.crc64(b"A").to_bytes(8, "little")
    add(R.build(b"\x01\x00\x00A\x00", 1, c0), R.OK, ret=0)
    add(R.build(b"\x02\x00\x00A\x00", 1, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    add(R.build(b"\x01\x00\x00A\x03\x00\x00A\x00", 2, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    add(R.build(b"\x01\x00\x00A\x7f\x00\x00A\x00", 2, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    add(R.build(b"\xe0\x00\x00\x00\x05\xe1\x00\x00\x00\x00\x00\x00\x00", 1, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    # lc + lp = 5: 4 + 9 * 1 = 13
    add(R.build(b"\xe0\x00\x00\x00\x05\x0d\x00\x00\x00\x00\x00\x00\x00", 1, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    # an LZMA chunk without properties after a dictionary reset; without a state reset
    lz = p["data"]
    assert lz[0] >= 0xE0
    add(R.build(b"\x01\x00\x00A" + bytes([0xA0]) + lz[1:5] + lz[6:], n + 1, c0), R.E_DATA, ret=R.LZMA_DATA_ERROR)
    add(R.build(bytes([0xC0]) + lz[1:], n, p["check"]), R.E_DATA, ret=R.LZMA_DATA_ERROR)  # no dictionary reset first
    # a stored chunk, then the LZMA chunks with a dictionary reset of their own
    both = b"A" * 77 + data
    add(R.build(b"\x01\x00\x4c" + b"A" * 77 + lz, len(both), R.crc64(both).to_bytes(8, "little")), R.OK, cap=len(both),
        ret=0)
    # the same behind a stored chunk without the reset: the LZMA chunk keeps its reset
    add(R.build(b"\x01\x00\x00A\x02\x00\x4b" + b"A" * 76 + lz, len(both), R.crc64(both).to_bytes(8, "little")), R.OK,
        cap=len(both), ret=0)
    # a chunk one byte longer / shorter than its symbols
    for d in (1, -1):
        us = (lz[1] << 8 | lz[2]) + d
        add(R.build(lz[:1] + bytes([us >> 8, us & 255]) + lz[3:], n + d, p["check"]), R.E_DATA, cap=n + 1,
            ret=R.LZMA_DATA_ERROR)
    # a distance beyond the block's dictionary: matches 5,000 back under a 4 KiB dictionary
    far = XI.payload("halfdup", 10000, 2).tobytes()
    pf = R.parts(R.compress(far))
    add(R.build(pf["data"], len(far), pf["check"]), R.OK, cap=len(far), ret=0)
    add(R.build(pf["data"], len(far), pf["check"], dict_prop=0), R.E_DATA, cap=len(far), ret=R.LZMA_DATA_ERROR)
    add(R.compress(far, dict_size=4096), R.OK, cap=len(far), ret=0)
    # block padding, index and footer against the block
    odd = R.parts(R.compress(b"abc"))
    assert len(odd["pad"]) > 0
    s = R.compress(b"abc")
    at = 12 + len(odd["block_header"]) + len(odd["data"])
    add(_flip(s, at), R.E_DATA, cap=3, ret=R.LZMA_DATA_ERROR)
    rec = b"\0" + R.vli(1) + R.vli(len(p["block_header"]) + len(p["data"]) + 8) + R.vli(n + 1)
    rec += b"\0" * (-len(rec) % 4)
    bad_index = rec + struct.pack("<I", R.crc32(rec))
    assert len(bad_index) == len(p["index"])
    add(stream[:-12 - len(bad_index)] + bad_index + p["footer"], R.E_HEADER, ret=R.LZMA_DATA_ERROR)
    tail = struct.pack("<I", len(p["index"]) // 4) + stream[6:8]
    add(stream[:-12] + struct.pack("<I", R.crc32(tail)) + tail + b"YZ", R.E_HEADER, ret=R.LZMA_DATA_ERROR)
    # block header with both size fields, right and wrong
    for dc, du, want in ((0, 0, R.OK), (1, 0, R.E_HEADER), (0, 1, R.E_HEADER)):
        bh = bytes([0, 0xC0]) + R.vli(len(p["data"]) + dc) + R.vli(n + du) + bytes([0x21, 1, 0x16])
        bh += b"\0" * (-(len(bh) + 4) % 4)
        bh = bytes([(len(bh) + 4) // 4 - 1]) + bh[1:]
        bh += struct.pack("<I", R.crc32(bh))
        add(R.build(p["data"], n, p["check"], block_header=bh), want, ret=0 if want == R.OK else R.LZMA_DATA_ERROR)
    # what liblzma reads and this decoder does not
    import lzma
    add(lzma.compress(data, check=lzma.CHECK_SHA256), R.E_UNSUPPORTED, ret=0)
    add(lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64,
                      filters=[{"id": lzma.FILTER_DELTA, "dist": 1}, {"id": lzma.FILTER_LZMA2, "preset": 6}]),
        R.E_UNSUPPORTED, ret=0)
    add(stream + stream, R.E_UNSUPPORTED, ret=0)
    add(stream + bytes(8) + stream, R.E_UNSUPPORTED, ret=0)
    blk = p["block_header"] + p["data"] + p["pad"] + p["check"]
    rec = b"\0" + R.vli(2) + 2 * (R.vli(len(p["block_header"]) + len(p["data"]) + 8) + R.vli(n))
    rec += b"\0" * (-len(rec) % 4)
    idx2 = rec + struct.pack("<I", R.crc32(rec))
    tail = struct.pack("<I", len(idx2) // 4 - 1) + stream[6:8]
    add(p["header"] + blk + blk + idx2 + struct.pack("<I", R.crc32(tail)) + tail + b"YZ", R.E_UNSUPPORTED, cap=2 * n,
        ret=0)
    # bytes after the footer are the caller's to judge
    add(stream + b"tail", R.OK, ret=0)
    add(stream + bytes(4), R.OK, ret=0)
    return cases


@needs_lzma
def test_crafted_streams_have_the_exact_status(check_exe, tmp_path):
    cases = crafted_cases()
    assert {c[5] for c in cases} == {R.OK, R.E_FORMAT, R.E_UNSUPPORTED, R.E_HEADER, R.E_DATA, R.E_INPUT, R.E_CHECK}
    run_cases(check_exe, tmp_path, cases)
