"""GPU tests of the LZMA bundle decoder, through the C ABI (zc_xz_decode /
zc_xz_decode_host, BundleDecompressor): the streams of tests/test_xz.py --
every payload kind, edge size and property set, the chunk limits, the three
check ids, mutants and crafted streams -- decoded on the device and held to
liblzma (tests/xz_ref.py).  Every call packs its streams at odd offsets and
its outputs between 0xEE canaries, which are checked: nothing outside a
bundle's room is written."""
import numpy as np
import pytest

from tests import xz_inputs as XI
from tests import xz_ref as R

pytestmark = pytest.mark.gpu
needs_lzma = pytest.mark.skipif(not R.available(), reason=R.why_not())

CANARY = 0xEE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


@pytest.fixture(scope="module")
def dec(torch_cuda):
    from zbackup_amd.bundle import BundleDecompressor
    with BundleDecompressor() as d:
        yield d


def run(torch, dec, streams, caps, seed=0):
    """One zc_xz_decode call over the streams, packed at odd offsets, outputs
    between canaries.  Returns (results, [the cap bytes of each output])."""
    rng = np.random.default_rng(seed)
    in_off, pos = [], 1
    for s in streams:
        in_off.append(pos)
        pos += len(s) + int(rng.integers(0, 7))
    src = np.zeros(pos + 16, dtype=np.uint8)
    for o, s in zip(in_off, streams):
        src[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    out_off, pos = [], 3
    for c in caps:
        out_off.append(pos)
        pos += c + int(rng.integers(1, 9))
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((pos + 16,), CANARY, dtype=torch.uint8, device="cuda")
    res = dec.decode(d_in.data_ptr(), in_off, [len(s) for s in streams], d_out.data_ptr(), out_off, caps, strict=False)
    got = d_out.cpu().numpy()
    keep = np.ones(len(got), dtype=bool)
    for o, c in zip(out_off, caps):
        keep[o:o + c] = False
    assert np.all(got[keep] == CANARY), "a byte outside every bundle's room was written"
    return res, [got[o:o + c] for o, c in zip(out_off, caps)]


def hold_to(cases, res, outs):
    """cases as tests/test_xz.py makes them: (stream, cap, lzma_ret, in_pos, bytes, wanted status or -1)."""
    for k, (c, r, o) in enumerate(zip(cases, res, outs)):
        stream, cap, ret, in_pos, expect, want = c
        st = int(r["status"])
        assert st != R.E_BUDGET, k
        assert int(r["decoded"]) <= cap, k
        if want >= 0:
            assert st == want, (k, st, want)
        elif ret >= 0:
            assert (st == 0) == (ret == 0), (k, st, ret)
        if st == 0:
            assert int(r["consumed"]) == in_pos and int(r["decoded"]) == len(expect), k
            assert o[:len(expect)].tobytes() == expect, k
            assert np.all(o[len(expect):] == CANARY), k
            assert int(r["info"]) & 15 == stream[7] & 15, k


def test_committed_streams(torch_cuda, dec):
    """The fixtures need no liblzma.  Both forms run: two fixtures need the
    wide one; with room one byte short each ends ZC_XZ_E_OUTPUT."""
    gold = R.golden()
    cases = [(s, len(d), 0, len(s), d, R.OK) for _, s, d, _ in gold]
    cases += [(s, len(d) - 1, -1, 0, b"", R.E_OUTPUT) for _, s, d, _ in gold if d]
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases])
    hold_to(cases, res, outs)
    wide = [bool(e["wide"]) for _, _, _, e in gold]
    assert [bool(int(r["info"]) & 0x100) for r in res[:len(gold)]] == wide
    stats = dec.last_stats()
    assert stats["n_wide"] == 2 * sum(wide) and stats["decode_ms"] > 0 and stats["total_ms"] >= stats["decode_ms"]
    print(stats)


@needs_lzma
@pytest.mark.parametrize("props", XI.PROPS, ids=lambda p: "lc%d_lp%d_pb%d" % p)
def test_every_kind_size_and_property_set(torch_cuda, dec, props):
    cases = []
    for kind in XI.KINDS:
        for n in XI.SIZES:
            data = XI.payload(kind, n, 7).tobytes()
            stream = R.compress(data, props=props)
            cases.append((stream, n, 0, len(stream), data, R.OK))
            if n in (1, 65, 274, XI.WINDOW + 1, 65537):
                cases.append((stream, n - 1, R.LZMA_BUF_ERROR, 0, b"", R.E_OUTPUT))
                cases.append((stream, n + 5, 0, len(stream), data, R.OK))
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases], seed=props[0])
    hold_to(cases, res, outs)
    assert (dec.last_stats()["n_wide"] > 0) == (props[0] + props[1] > 3)


@needs_lzma
def test_chunk_limits(torch_cuda, dec):
    """A second LZMA chunk without reset, the 2 MiB chunk limit (chunks FF.. then
    80..), and 34 stored chunks followed by an LZMA chunk with reset."""
    text = XI.payload("text", 1200000, 11).tobytes()
    st = R.compress(text)
    ctl = [c for c, _, _ in R.chunks(R.parts(st)["data"])]
    assert any(0x80 <= c < 0xA0 for c in ctl[1:]), ctl
    zeros = bytes((2 << 20) + 1)
    half = XI.payload("halfdup", 2 << 20, 5).tobytes()
    cases = [(s, len(d), 0, len(s), d, R.OK) for s, d in ((st, text), (R.compress(zeros), zeros),
                                                          (R.compress(half), half))]
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases])
    hold_to(cases, res, outs)
    print(dec.last_stats())


@needs_lzma
def test_check_ids_and_a_wrong_check(torch_cuda, dec):
    cases = []
    for check in (0, 1, 4):
        for kind, n in (("text", 3000), ("random", 500), ("zeros", 1), ("halfdup", 70000), ("text", 0)):
            data = XI.payload(kind, n, 3).tobytes()
            stream = R.compress(data, check=check)
            assert stream[7] == check
            cases.append((stream, n, 0, len(stream), data, R.OK))
            p = R.parts(stream) if n else None
            if n and check:
                at = len(stream) - 12 - len(p["index"]) - 1  # the stored check's last byte
                bad = bytearray(stream)
                bad[at] ^= 0x40
                cases.append((bytes(bad), n, R.LZMA_DATA_ERROR, 0, b"", R.E_CHECK))
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases])
    hold_to(cases, res, outs)


@needs_lzma
def test_mutants_agree_with_liblzma(torch_cuda, dec):
    """40 single-bit flips and 10 truncations of each of 12 streams in one
    call: accepted exactly when liblzma accepts, with its bytes; never
    ZC_XZ_E_BUDGET; nothing written outside the rooms."""
    from tests.test_xz import mutant_cases
    cases = mutant_cases(40, 10, seed=21)
    rets = {c[2] for c in cases}
    assert {R.LZMA_DATA_ERROR, R.LZMA_BUF_ERROR} <= rets, rets
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases])
    hold_to(cases, res, outs)


@needs_lzma
def test_crafted_streams_have_the_exact_status(torch_cuda, dec):
    from tests.test_xz import crafted_cases
    cases = crafted_cases()
    res, outs = run(torch_cuda, dec, [c[0] for c in cases], [c[1] for c in cases])
    hold_to(cases, res, outs)


def test_host_form_and_strictness(torch_cuda, dec):
    from zbackup_amd import ZcError
    gold = R.golden()
    bodies, datas = [s for _, s, _, _ in gold], [d for _, _, d, _ in gold]
    assert dec.decode_host(bodies, [len(d) for d in datas]) == datas
    assert dec.decode_host([], []) == []
    with pytest.raises(ZcError, match="bundle 1: the stream ends after"):
        dec.decode_host([bodies[0], bodies[1] + b"\0\0\0\0"], [len(datas[0]), len(datas[1])])
    with pytest.raises(ZcError, match="bundle 0: ZC_XZ_E_OUTPUT"):
        dec.decode_host(bodies[:1], [len(datas[0]) - 1])
    with pytest.raises(ZcError, match="bundle 0: 3000 bytes decoded, its payload has 3001"):
        dec.decode_host(bodies[:1], [len(datas[0]) + 1])
    with pytest.raises(ZcError, match="bundle 2: ZC_XZ_E_FORMAT"):
        dec.decode_host(bodies[:2] + [b"not an xz stream"], [len(d) for d in datas[:2]] + [5])


def test_argument_errors(torch_cuda, dec):
    from zbackup_amd import ZcError
    torch = torch_cuda
    s = R.golden()[0][1]
    d_in = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(ZcError, match="overlap"):
        dec.decode(d_in.data_ptr(), [0, 0], [len(s)] * 2, d_out.data_ptr(), [0, 2999], [3000, 3000])
    with pytest.raises(ZcError, match="null pointer"):
        dec.decode(d_in.data_ptr(), [0], [len(s)], None, [0], [3000])
    # the device-memory helpers: null pointers, nothing to do, a round trip
    L, ctx = dec._L, dec._ctx
    assert L.zc_device_alloc(ctx, 16, None) != 0 and b"zc_device_alloc: null pointer" in L.zc_last_error(ctx)
    assert L.zc_upload(ctx, None, b"x", 1) != 0 and b"zc_upload: null pointer" in L.zc_last_error(ctx)
    assert L.zc_upload(ctx, d_out.data_ptr(), None, 1) != 0
    assert L.zc_upload(ctx, None, None, 0) == 0 and L.zc_device_free(ctx, None) == 0
    buf = dec.alloc(0)
    assert buf
    dec.free(buf)
    dec.upload(d_out.data_ptr() + 5, b"abc")
    assert bytes(d_out[4:9].cpu().numpy()) == bytes([CANARY]) + b"abc" + bytes([CANARY])
    d_out[5:8] = CANARY
    assert len(dec.decode(d_in.data_ptr(), [], [], d_out.data_ptr(), [], [])) == 0  # nothing to do
    assert bool(torch.all(d_out == CANARY))
    # rooms that touch do not overlap; a room of no bytes lies anywhere
    res = dec.decode(d_in.data_ptr(), [0, 0, 0], [len(s)] * 3, d_out.data_ptr(), [0, 3000, 100], [3000, 3000, 0],
                     strict=False)
    assert [int(r["status"]) for r in res] == [R.OK, R.OK, R.E_OUTPUT]
