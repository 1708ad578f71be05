"""zc_xzenc_core.h -- the encoder zc_xzenc.hip's kernels run -- compiled for the
host under ASan + UBSan with a main of its own (tests/xzenc/xzenc_core_check.cpp).
The program round-trips every stream through zc_xz_core.h and aborts on any
difference, on a stream that depends on its room, and on a missing E_OUTPUT;
here every stream is held to liblzma (tests/xz_ref.py).  No GPU."""
import struct

import pytest

from tests import xz_inputs as XI
from tests import xz_ref as R
from tests import xzenc_ref as E

needs_lzma = pytest.mark.skipif(not R.available(), reason=R.why_not())


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("xzenc_core")
    if not E.sanitizers_link(tmp):
        pytest.skip("g++ does not link a program under -fsanitize=address,undefined here")
    return E.build_exe(tmp, sanitize=True)


@pytest.fixture(scope="module")
def encoded(check_exe, tmp_path_factory):
    """Every case through the core once: {name: (check, payload, stored chunks, stream)}, the symbol counts."""
    cases = E.all_cases()
    res, kinds = E.run(check_exe, tmp_path_factory.mktemp("xzenc_run"), [(c, d) for _, c, d in cases])
    out = {}
    for (name, check, data), (status, stored, stream) in zip(cases, res):
        assert status == R.OK, name
        out[name] = (check, data, stored, stream)
    return out, kinds


def dict_prop_for(n):
    prop = 0
    while (2 | (prop & 1)) << (prop // 2 + 11) < n:
        prop += 1
    return prop


@needs_lzma
def test_liblzma_reads_every_stream_and_the_container_says_what_the_block_is(encoded):
    streams, _ = encoded
    assert len(streams) == len(XI.KINDS) * len(XI.SIZES) + 10 + 5 + 12
    for name, (check, data, stored, stream) in streams.items():
        n = len(data)
        ret, in_pos, back = R.buffer_decode(stream, n)
        assert ret == R.LZMA_OK and back == data and in_pos == len(stream), name
        assert len(stream) <= E.capacity(n), name
        assert stream[:6] == b"\xfd7zXZ\0" and stream[6:8] == bytes([0, check]), name
        if n == 0:
            assert len(stream) == 32 and stream == R.compress(b"", check=check), name
            continue
        p = R.parts(stream)
        assert p["header"] + p["block_header"] + p["data"] + p["pad"] + p["check"] + p["index"] + p["footer"] == stream
        bh = bytes([2, 0, 0x21, 1, dict_prop_for(n), 0, 0, 0])
        assert p["block_header"] == bh + struct.pack("<I", R.crc32(bh)), name
        assert p["usize"] == n and p["pad"] == bytes(-len(p["data"]) % 4), name
        want = {0: b"", 1: struct.pack("<I", R.crc32(data)), 4: struct.pack("<Q", R.crc64(data))}[check]
        assert p["check"] == want, name
        assert R.build(p["data"], n, want, check_id=check, block_header=p["block_header"]) == stream, name
        ch = R.chunks(p["data"])
        assert ch[-1][0] == 0 and ch[-1][1] + 1 == len(p["data"]), name
        assert sum(1 for c, _, _ in ch if c in (1, 2)) == stored, name
        assert len(ch) - 1 == (n + E.CHUNK - 1) // E.CHUNK, name  # chunk k covers payload [64 Ki k, 64 Ki (k + 1))
        for c, _, size in ch[:-1]:
            if c >= 0x80:
                assert size - (6 if c >= 0xC0 else 5) <= 65536, name


def controls(stream):
    return [c & 0xE0 if c >= 0x80 else c for c, _, _ in R.chunks(R.parts(stream)["data"])]


def test_chunk_rules(encoded):
    """Each input reaches the rule it is named for.  The fifth rule of the
    format, a chunk cut by the compressed-size limit, has no case: a chunk
    covers 64 KiB of payload at most and its LZMA form is given up the moment
    it cannot be smaller than the stored form (header + compressed >= 3 +
    payload), so a kept chunk's compressed size is below its payload's 64 KiB
    and never reaches the 16-bit field's limit; the random cases below are the
    ones that run into that rule, and they end stored."""
    s, _ = encoded
    assert controls(s["text_3_chunks"][3]) == [0xE0, 0x80, 0x80, 0]       # no reset after the first
    assert controls(s["random_two_stored"][3]) == [1, 2, 0]                    # stored: dictionary reset, then none
    assert controls(s["random_then_text"][3]) == [1, 0xC0, 0]             # state reset with the properties
    assert controls(s["text_then_random"][3]) == [0xE0, 2, 0]
    assert controls(s["random_text_random_text"][3]) == [1, 0xC0, 2, 0xA0, 0]  # state reset, properties known
    assert controls(s["far_copy_1mib"][3])[:3] == [1, 0xC0, 0x80]


def test_every_symbol_kind_is_coded(encoded):
    """literal, matched literal, match, short rep, rep0 (long), rep1..3, the
    three length coders, and the three distance forms: a slot alone (distance
    1..4), a slot with reverse-tree bits (5..128), and a slot with direct bits
    and the align bits (129 and up)."""
    _, kinds = encoded
    assert set(kinds) == set(E.KINDS)
    for k, v in kinds.items():
        assert v >= 1, (k, kinds)


def test_match_forms(encoded):
    s, _ = encoded
    for per in (1, 2, 3, 63, 64, 65, 300):
        assert len(s[f"period{per}_5000"][3]) < 200 + per, per  # the period once, then matches
    for run_len in (273, 274, 546):
        assert len(s[f"run{run_len}"][3]) < 280, run_len        # 200 literals of 6 bits and a few matches
    check, data, stored, stream = s["far_copy_1mib"]
    assert len(stream) < len(data) - 99000  # the second copy of the 100,000 random bytes costs next to nothing


def test_determinism(check_exe, tmp_path, encoded):
    s, _ = encoded
    names = ("text_65537", "halfdup_2049", "random_65537", "four_sources", "period300_274")
    again, _ = E.run(check_exe, tmp_path, [(s[n][0], s[n][1]) for n in names])
    for n, (_, _, stream) in zip(names, again):
        assert stream == s[n][3], n


def test_committed_lengths_and_crcs(check_exe, tmp_path):
    """The fixtures need no liblzma: the payload comes from its seed, the
    stream is known by its length and CRC64."""
    gold = E.golden()
    assert len(gold) >= 12
    res, _ = E.run(check_exe, tmp_path, E.golden_cases())
    for e, (status, stored, stream) in zip(gold, res):
        assert status == R.OK
        assert (len(stream), "%016x" % E.crc64(stream), stored) == (e["stream_len"], e["stream_crc64"],
                                                                   e["stored_chunks"]), e


def _lzo_frame(data):
    from oracle import lzo_oracle
    return lzo_oracle.frame(data)


def test_smaller_than_lzo_on_two_mib(check_exe, tmp_path):
    """The reason to write LZMA rather than lzo is size: on 2 MiB text-like,
    half-duplicated, zero and periodic payloads the stream is smaller than the
    framed lzo1x_1 output.  Random payloads are held to the capacity bound."""
    try:
        _lzo_frame(b"probe")
    except Exception as e:  # liblzo2 is reached the way tests/test_lzo.py reaches it
        pytest.skip(f"liblzo2 is not here: {e}")
    kinds = ("text", "halfdup", "zeros", "period300", "random")
    cases = [(4, XI.payload(k, 2 << 20, 5).tobytes()) for k in kinds]
    res, _ = E.run(check_exe, tmp_path, cases)
    for k, (_, data), (status, stored, stream) in zip(kinds, cases, res):
        lzo = len(_lzo_frame(data))
        print(k, "xz", len(stream), "lzo1x_1 framed", lzo)
        assert status == R.OK and len(stream) <= E.capacity(len(data))
        if k != "random":
            assert len(stream) < lzo, k


def test_the_model_of_the_cutting_rule():
    """tests/xzenc_ref.py's restatement of how zc_xz_encode cuts a call into
    batches (the GPU tests predict zc_xz_encode_last_schedule with it), against
    cuts written out by hand."""
    ends = E.batch_ends
    assert ends([], 1) == [] and ends([], 1 << 40) == []                  # the empty call launches nothing
    assert ends([0, 0, 0], 1) == [3]                                        # no bytes: one batch, never cut
    assert ends([100], 1) == [1] and ends([100, 100], 1) == [1, 2]          # larger than the room: the pool grows to it
    assert ends([10, 20, 30], 60) == [3]                                    # an exact fit
    assert ends([10, 20, 30], 59) == [2, 3] and ends([10, 20, 30], 61) == [3]
    assert ends([30, 30, 30, 30], 60) == [2, 4]
    assert ends([5, 0, 0, 5], 5) == [3, 4]                                  # empty payloads never start a batch ...
    assert ends([0, 0, 5, 0, 5, 0], 1) == [4, 6]                            # ... and never end one
    assert ends([7, 1, 1, 1], 1) == [1, 4] and ends([1, 1, 1, 7], 1) == [3, 4]  # the pool is the largest payload
    assert ends([65537, 0, 65536, 1, 0, 1], 65537) == [2, 5, 6]                # 65536 + 1 fits exactly
    assert E.rounds_of(1, 256) == 1 and E.rounds_of(2048, 256) == 1 and E.rounds_of(2049, 256) == 2
    assert E.rounds_of(5, 1) == 1 and E.rounds_of(9, 1) == 2 and E.rounds_of(3 * 8 + 1, 1) == 4
    # generations: a batch a generation, the clear when the last one would reach 0xffffffff
    assert E.generations([1, 2, 3], 256, 0) == (3, [])
    assert E.generations([1, 2, 3], 256, 0xfffffffb) == (0xfffffffe, [])
    assert E.generations([1, 2, 3], 256, 0xfffffffc) == (1, [2])
    assert E.generations([1, 2, 3], 256, 0xfffffffe) == (3, [0])
    assert E.generations([2049], 256, 0xfffffffc) == (0xfffffffe, []) and E.generations([2049], 256, 0xfffffffd) == (2, [0])
