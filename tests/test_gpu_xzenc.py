"""GPU tests of the LZMA bundle encoder, through the C ABI (zc_xz_encode /
zc_xz_encode_host, BundleCompressor.compress_xz): every payload of
tests/xzenc_ref.py encoded on the device and held byte for byte to the host
core's stream for the same payload, to Python's lzma and to zc_xz_decode.
Every call packs its payloads at odd offsets and its outputs between 64-byte
0xEE canaries, which are checked: nothing outside a bundle's room is written."""
import hashlib
import lzma
import zlib

import numpy as np
import pytest

from tests import aes_ref
from tests import xz_inputs as XI
from tests import xz_ref as R
from tests import xzenc_ref as E

pytestmark = pytest.mark.gpu

CANARY = 0xEE
GUARD = 64
KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d7781")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


@pytest.fixture(scope="module")
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """The host core as a plain program (the CPU test runs it under the sanitizers)."""
    return E.build_exe(tmp_path_factory.mktemp("xzenc_host"), sanitize=False)


@pytest.fixture(scope="module")
def reference(host_exe, tmp_path_factory):
    """The host core's streams of every case, computed once: (cases, [(status, stored, stream)])."""
    cases = E.all_cases()
    by_check = {}
    for k, (_, check, _) in enumerate(cases):
        by_check.setdefault(check, []).append(k)
    res, _ = E.run(host_exe, tmp_path_factory.mktemp("xzenc_ref"), [(c, d) for _, c, d in cases])
    return cases, res, by_check


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    monkeypatch.delenv("ZC_TEST_XZENC_POOL", raising=False)
    monkeypatch.delenv("ZC_TEST_XZENC_GEN0", raising=False)


def encode(torch, comp, payloads, check=4, caps=None, seed=0):
    """One zc_xz_encode call: payloads packed at odd offsets, outputs between
    canaries.  Returns (results, [the cap bytes of each output])."""
    rng = np.random.default_rng(seed)
    pay_off, pos = [], 1
    for p in payloads:
        pay_off.append(pos)
        pos += len(p) + int(rng.integers(0, 7))
    src = np.zeros(pos + 16, dtype=np.uint8)
    for o, p in zip(pay_off, payloads):
        src[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    caps = [comp.xz_capacity(len(p)) for p in payloads] if caps is None else caps
    out_off, pos = [], GUARD + 3
    for c in caps:
        out_off.append(pos)
        pos += c + GUARD + int(rng.integers(0, 9))
    d_pay = torch.from_numpy(src).cuda()
    d_out = torch.full((pos + 16,), CANARY, dtype=torch.uint8, device="cuda")
    res = comp.compress_xz(d_pay.data_ptr(), pay_off, [len(p) for p in payloads], d_out.data_ptr(), out_off,
                           check=check, out_cap=caps, strict=False)
    got = d_out.cpu().numpy()
    keep = np.ones(len(got), dtype=bool)
    for o, c in zip(out_off, caps):
        keep[o:o + c] = False
    assert np.all(got[keep] == CANARY), "a byte outside every bundle's room was written"
    return res, [got[o:o + c] for o, c in zip(out_off, caps)], (d_out, out_off)


def streams_of(res, outs):
    out = []
    for r, o in zip(res, outs):
        assert int(r["status"]) == R.OK
        n = int(r["size"])
        assert n <= len(o) and np.all(o[n:] == CANARY)  # nothing behind the stream either
        out.append(o[:n].tobytes())
    return out


def test_every_case_gives_the_host_core_s_bytes(torch_cuda, comp, reference):
    """The whole kind x size grid and the chunk-rule and match-form cases, one
    call per check id (the CRC64 call holds some 200 bundles)."""
    from zbackup_amd.bundle import BundleDecompressor
    torch = torch_cuda
    cases, ref, by_check = reference
    assert sorted(by_check) == [0, 1, 4] and len(by_check[4]) > 190
    for check, idx in sorted(by_check.items()):
        payloads = [cases[k][2] for k in idx]
        res, outs, (d_out, out_off) = encode(torch, comp, payloads, check=check, seed=check)
        got = streams_of(res, outs)
        for k, s, r in zip(idx, got, res):
            name = cases[k][0]
            assert s == ref[k][2], name  # byte for byte: a race in the match kernel or the stores shows here
            assert int(r["info"]) & 15 == check and int(r["info"]) >> 8 == ref[k][1], name
            assert lzma.decompress(s) == cases[k][2], name
            if cases[k][2]:
                ch = R.chunks(R.parts(s)["data"])
                assert sum(1 for c, _, _ in ch if c in (1, 2)) == int(r["info"]) >> 8, name
        # back through the device decoder, from where the streams lie
        sizes = [len(p) for p in payloads]
        back_off = np.concatenate([[0], np.cumsum([n + 5 for n in sizes])[:-1]]).astype(np.uint64)
        d_back = torch.full((sum(sizes) + 5 * len(sizes) + 16,), CANARY, dtype=torch.uint8, device="cuda")
        with BundleDecompressor(ctx=comp._ctx) as dec:
            dres = dec.decode(d_out.data_ptr(), out_off, [len(s) for s in got], d_back.data_ptr(), back_off, sizes,
                              strict=False)
        back = d_back.cpu().numpy()
        for k, p, o, s, dr in zip(idx, payloads, back_off, got, dres):
            assert int(dr["status"]) == R.OK and int(dr["consumed"]) == len(s) and int(dr["decoded"]) == len(p)
            assert back[int(o):int(o) + len(p)].tobytes() == p, cases[k][0]
    st = comp.xz_last_stats()
    print(st)
    assert st["match_ms"] > 0 and st["code_ms"] > 0 and st["total_ms"] >= st["code_ms"]


def test_committed_lengths_and_crcs(torch_cuda, comp):
    gold = E.golden()
    for check in (0, 1, 4):
        sel = [e for e in gold if e["check"] == check]
        payloads = [XI.payload(e["kind"], e["size"], e["seed"]).tobytes() for e in sel]
        res, outs, _ = encode(torch_cuda, comp, payloads, check=check, seed=9)
        for e, s, r in zip(sel, streams_of(res, outs), res):
            assert (len(s), "%016x" % E.crc64(s), int(r["info"]) >> 8) == (e["stream_len"], e["stream_crc64"],
                                                                           e["stored_chunks"]), e


def test_repeated_calls_on_a_warm_context(torch_cuda, comp, reference):
    """The tables are tagged with a generation, not cleared: the same call
    again gives the same bytes, and again after a call with other payloads."""
    cases, ref, by_check = reference
    idx = [k for k in by_check[4] if len(cases[k][2]) in (2049, 65537)]
    assert len(idx) >= 24
    payloads = [cases[k][2] for k in idx]
    for turn in range(3):
        res, outs, _ = encode(torch_cuda, comp, payloads, seed=turn)
        assert streams_of(res, outs) == [ref[k][2] for k in idx], turn
        if turn == 1:
            other = [XI.payload("text", 5000 + 17 * j, 50 + j).tobytes() for j in range(40)]
            res, outs, _ = encode(torch_cuda, comp, other, seed=7)
            for s, p in zip(streams_of(res, outs), other):
                assert lzma.decompress(s) == p


def test_more_bundles_than_one_grid_pass(torch_cuda, comp, host_exe, tmp_path):
    """The grid is at most two blocks of four waves per CU, a wave per bundle:
    with more bundles than that a wave takes a second one under the next
    generation of its table."""
    torch = torch_cuda
    waves = 2 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    n = waves + waves // 2 + 3
    kinds = ("text", "halfdup", "alphabet4", "random", "period65")
    payloads = [XI.payload(kinds[j % 5], 2048 - j % 7, 1000 + j).tobytes() for j in range(n)]
    ref, _ = E.run(host_exe, tmp_path, [(4, p) for p in payloads])
    res, outs, _ = encode(torch, comp, payloads, seed=3)
    got = streams_of(res, outs)
    pick = set(np.random.default_rng(5).choice(n, 64, replace=False).tolist()) | {0, waves - 1, waves, n - 1}
    for j, (s, (_, stored, want)) in enumerate(zip(got, ref)):
        if j in pick:
            assert s == want, j
            assert lzma.decompress(s) == payloads[j], j
        assert (len(s), zlib.crc32(s)) == (len(want), zlib.crc32(want)), j


# ---- the schedule: batches and the tables' generations (ZC_TEST_XZENC_POOL / ZC_TEST_XZENC_GEN0) ----

GEN_LAST = 0xfffffffe  # the last generation a launch may use


def fresh(monkeypatch, gen0=None):
    """A compressor of its own: the encoder's state, made by its first call, reads ZC_TEST_XZENC_GEN0."""
    from zbackup_amd.bundle import BundleCompressor
    if gen0 is not None:
        monkeypatch.setenv("ZC_TEST_XZENC_GEN0", str(gen0))
    return BundleCompressor()


def cus_of(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def mixed_payloads(cases, by_check):
    """Some 40 payloads, the sizes mixed: grid cases of 0, 1, 2049, 65536 and
    65537 bytes and payloads of 300 and 40000; the largest first and last,
    empty ones before and behind it."""
    kinds = ("text", "halfdup", "random", "period65", "alphabet4", "zeros")
    grid = {(cases[k][0].rsplit("_", 1)[0], len(cases[k][2])): cases[k][2] for k in by_check[4]}
    order = [65537, 0, 0, 65537, 1, 300, 2049, 40000, 0, 40000, 0, 65536, 1, 0, 2049, 300, 65536, 0, 65537, 0, 40000,
             300, 300, 2049, 1, 65536, 0, 0, 65536, 40000, 2049, 2049, 1, 300, 65537, 0, 40000, 0, 1, 0, 65537]
    out = []
    for j, n in enumerate(order):
        kind = kinds[j % len(kinds)]
        out.append(grid[(kind, n)] if (kind, n) in grid else XI.payload(kind, n, 200 + j).tobytes())
    assert sum(1 for j, n in enumerate(order) if (kinds[j % len(kinds)], n) in grid) >= 25
    return out


@pytest.fixture(scope="module")
def mixed(reference, host_exe, tmp_path_factory):
    """(payloads, {check: [(status, stored, stream)]}): the host core's streams, which know no batches."""
    cases, _, by_check = reference
    payloads = mixed_payloads(cases, by_check)
    tmp = tmp_path_factory.mktemp("xzenc_mixed")
    return payloads, {check: E.run(host_exe, tmp, [(check, p) for p in payloads])[0] for check in (0, 1, 4)}


def assert_streams(res, outs, payloads, ref, check=4):
    got = streams_of(res, outs)
    for j, (s, r, p, (_, stored, want)) in enumerate(zip(got, res, payloads, ref)):
        assert s == want, (j, len(p))
        assert int(r["info"]) & 15 == check and int(r["info"]) >> 8 == stored, (j, len(p))
        assert lzma.decompress(s) == p, (j, len(p))


@pytest.mark.parametrize("room", [65537, 1])
def test_a_call_cut_into_batches(torch_cuda, monkeypatch, reference, mixed, room):
    """ZC_TEST_XZENC_POOL stands for the free memory's share, so a call of a
    few hundred KiB is cut as one of many GiB would be: later batches begin at
    first > 0, write their candidates from offset 0 of the buffer the batch
    before used, and run under the next generation.  Room 65537: batches of
    several payloads.  Room 1: the pool is the largest payload, and among
    payloads of 0, 40000 and more bytes every non-empty one is a batch."""
    cases, ref_all, by_check = reference
    payloads, ref = mixed
    keep = list(range(len(payloads))) if room == 65537 else [j for j, p in enumerate(payloads)
                                                             if len(p) == 0 or len(p) >= 40000]
    payloads = [payloads[j] for j in keep]
    sizes = [len(p) for p in payloads]
    assert sizes[0] == sizes[-1] == max(sizes) == 65537 and len(payloads) >= (40 if room == 65537 else 20)
    ends = E.batch_ends(sizes, room)
    assert len(ends) >= 5
    cuts = ends[:-1]
    assert any(sizes[e - 1] == 0 for e in cuts) and any(sizes[e + 1] == 0 for e in cuts)  # empty ones at a cut
    if room == 1:
        assert len(ends) == sum(1 for n in sizes if n)
    # the grid's payloads among them are the module's reference too
    known = {cases[k][2]: ref_all[k][2] for k in by_check[4]}
    assert all(ref[4][j][2] == known[p] for j, p in zip(keep, payloads) if p in known)
    monkeypatch.setenv("ZC_TEST_XZENC_POOL", str(room))
    with fresh(monkeypatch) as c:
        gen = 0
        for check in (0, 1, 4):
            res, outs, _ = encode(torch_cuda, c, payloads, check=check, seed=check + room)
            assert_streams(res, outs, payloads, [ref[check][j] for j in keep], check)
            st = c.xz_last_stats()
            gen += len(ends)
            print(room, check, st)
            assert (st["batches"], st["max_rounds"], st["generation"]) == (len(ends), 1, gen)
        # what does not parse is ignored: one batch, wider than any before, so on regrown tables
        for bad in ("none", "0", "-5"):
            monkeypatch.setenv("ZC_TEST_XZENC_POOL", bad)
            res, outs, _ = encode(torch_cuda, c, payloads, seed=9)
            assert_streams(res, outs, payloads, [ref[4][j] for j in keep])
            st = c.xz_last_stats()
            assert (st["batches"], st["max_rounds"]) == (1, 1), bad
        assert st["generation"] == 3


def test_the_last_generation_is_used_and_the_next_call_clears(torch_cuda, monkeypatch, mixed):
    """A call whose last batch runs under generation 0xfffffffe exactly: no
    clear.  The call after it starts over on cleared tables."""
    payloads, ref = mixed
    payloads, ref = payloads[:16], ref[4][:16]
    ends = E.batch_ends([len(p) for p in payloads], 65537)
    assert len(ends) >= 3
    monkeypatch.setenv("ZC_TEST_XZENC_POOL", "65537")
    with fresh(monkeypatch, GEN_LAST - len(ends)) as c:
        res, outs, _ = encode(torch_cuda, c, payloads, seed=1)
        assert_streams(res, outs, payloads, ref)
        st = c.xz_last_stats()
        assert (st["batches"], st["max_rounds"], st["generation"]) == (len(ends), 1, GEN_LAST)
        assert E.generations(ends, cus_of(torch_cuda), GEN_LAST - len(ends)) == (GEN_LAST, [])
        res, outs, _ = encode(torch_cuda, c, payloads, seed=2)
        assert_streams(res, outs, payloads, ref)
        st = c.xz_last_stats()
        assert (st["batches"], st["generation"]) == (len(ends), len(ends))  # cleared before its first batch
        assert E.generations(ends, cus_of(torch_cuda), GEN_LAST) == (len(ends), [0])


def test_the_tables_are_cleared_in_the_middle_of_a_call(torch_cuda, monkeypatch, mixed):
    payloads, ref = mixed
    payloads, ref = payloads[:16], ref[4][:16]
    ends = E.batch_ends([len(p) for p in payloads], 65537)
    assert len(ends) >= 4
    monkeypatch.setenv("ZC_TEST_XZENC_POOL", "65537")
    gen0 = GEN_LAST - 2  # two batches fit, the third clears
    assert E.generations(ends, cus_of(torch_cuda), gen0) == (len(ends) - 2, [2])
    with fresh(monkeypatch, gen0) as c:
        for turn in range(2):
            res, outs, _ = encode(torch_cuda, c, payloads, seed=3 + turn)
            assert_streams(res, outs, payloads, ref)  # the batches before the clear and after it
            st = c.xz_last_stats()
            assert (st["batches"], st["generation"]) == (len(ends), (turn + 1) * len(ends) - 2)
        other = [XI.payload("text", 5000 + 17 * j, 50 + j).tobytes() for j in range(12)]
        res, outs, _ = encode(torch_cuda, c, other, seed=7)
        for s, p in zip(streams_of(res, outs), other):
            assert lzma.decompress(s) == p


def test_two_rounds_under_the_last_two_generations(torch_cuda, monkeypatch, host_exe, tmp_path):
    """test_more_bundles_than_one_grid_pass's shape on a context whose launch
    starts at generation 0xfffffffd: the waves' second payloads run under
    0xfffffffe, the last one there is."""
    torch = torch_cuda
    waves = 2 * 4 * cus_of(torch)
    n = waves + waves // 2 + 3
    kinds = ("text", "halfdup", "alphabet4", "random", "period65")
    payloads = [XI.payload(kinds[j % 5], 2048 - j % 7, 1000 + j).tobytes() for j in range(n)]
    ref, _ = E.run(host_exe, tmp_path, [(4, p) for p in payloads])
    with fresh(monkeypatch, GEN_LAST - 2) as c:  # the launch's first generation is the scratch's + 1
        res, outs, _ = encode(torch, c, payloads, seed=3)
        st = c.xz_last_stats()
        assert (st["batches"], st["max_rounds"], st["generation"]) == (1, 2, GEN_LAST)
        got = streams_of(res, outs)
        pick = set(np.random.default_rng(5).choice(n, 64, replace=False).tolist()) | {0, waves - 1, waves, n - 1}
        for j, (s, (_, stored, want)) in enumerate(zip(got, ref)):
            if j in pick:
                assert s == want, j
                assert lzma.decompress(s) == payloads[j], j
            assert (len(s), zlib.crc32(s)) == (len(want), zlib.crc32(want)), j
        # one more round would pass the end: the same call again clears first
        res, outs, _ = encode(torch, c, payloads[:waves // 4], seed=4)
        assert streams_of(res, outs) == [r[2] for r in ref[:waves // 4]]
        assert c.xz_last_stats()["generation"] == 1


def test_regrown_tables_start_from_gen0(torch_cuda, monkeypatch, mixed):
    """A small call, then one wide enough to take more tables: the new tables
    are cleared and start from ZC_TEST_XZENC_GEN0 as the first ones did."""
    payloads, ref = mixed
    gen0 = 0x7fffffff
    with fresh(monkeypatch, gen0) as c:
        res, outs, _ = encode(torch_cuda, c, payloads[:4], seed=1)
        assert_streams(res, outs, payloads[:4], ref[4][:4])
        assert c.xz_last_stats()["generation"] == gen0 + 1
        res, outs, _ = encode(torch_cuda, c, payloads, seed=2)  # 41 waves' tables instead of 4
        assert_streams(res, outs, payloads, ref[4])
        st = c.xz_last_stats()
        assert (st["batches"], st["generation"]) == (1, gen0 + 1)
        res, outs, _ = encode(torch_cuda, c, payloads[:4], seed=3)  # narrower again: the tables stay
        assert_streams(res, outs, payloads[:4], ref[4][:4])
        assert c.xz_last_stats()["generation"] == gen0 + 2
    for bad in ("-1", str(0xffffffff), "x", ""):  # outside [0, 0xfffffffe]: not honoured
        with fresh(monkeypatch, bad) as c:
            res, outs, _ = encode(torch_cuda, c, payloads[:4], seed=1)
            assert_streams(res, outs, payloads[:4], ref[4][:4])
            assert c.xz_last_stats()["generation"] == 1, bad


def test_room_one_byte_short(torch_cuda, comp, reference):
    cases, ref, by_check = reference
    names = ("text_2049", "halfdup_65537", "random_2048", "period3_274", "text_65536")
    idx = [k for k in by_check[4] if cases[k][0] in names]
    assert len(idx) == len(names)
    payloads = [cases[k][2] for k in idx]
    for short in (1, 2):
        caps = [len(ref[k][2]) for k in idx]  # exactly the stream's length: enough
        caps[short] -= 1
        res, outs, _ = encode(torch_cuda, comp, payloads, caps=caps, seed=short)
        for j, (k, r, o) in enumerate(zip(idx, res, outs)):
            if j == short:
                assert int(r["status"]) == R.E_OUTPUT and int(r["size"]) == 0
            else:
                assert int(r["status"]) == R.OK and o.tobytes() == ref[k][2], cases[k][0]
    res, outs, _ = encode(torch_cuda, comp, payloads, caps=[0, 11, 23, 24, 31], seed=4)
    assert [int(r["status"]) for r in res] == [R.E_OUTPUT] * 5


def test_host_form_equals_the_device_form(torch_cuda, comp, reference):
    cases, ref, by_check = reference
    for check in (0, 1, 4):
        idx = [k for k in by_check[check] if len(cases[k][2]) <= 70000][::3]
        got = comp.compress_xz_host([cases[k][2] for k in idx], check=check)
        assert got == [ref[k][2] for k in idx], check
    assert comp.compress_xz_host([]) == []


def test_write_path_end_to_end(torch_cuda, comp):
    """stream -> chunks -> bundles -> xz -> sealed files, with and without a
    key (all on the GPU); then the files unsealed and the bodies decoded and
    replayed on the device by Restorer.replay_bodies."""
    from zbackup_amd import ZC_CHUNK_NEW, BackupCreator, Restorer
    from zbackup_amd.bundle import bundle_file_size, plan_bundles
    from tests.lzo_inputs import payload
    torch = torch_cuda
    W = 4096
    a = payload("text", 2 << 20, 21)
    data = np.concatenate([a, payload("random", 1 << 20, 22), a[5:(1 << 20) + 5], np.zeros(512 << 10, np.uint8),
                           payload("repeats", (1 << 20) + (512 << 10), 23)])
    assert len(data) == 6 << 20
    d = torch.from_numpy(data).cuda()
    with BackupCreator(chunk_max_size=W, sha1=True) as bc:
        bc.chunk_device(d.data_ptr(), len(data))
        recs = bc.records()
        backup_data = bc.get_backup_data()
    seen, offs, sizes, ids = set(), [], [], []
    for r in recs[recs["kind"] == ZC_CHUNK_NEW]:
        cid = bytes(r["sha1"]) + int(r["rolling"]).to_bytes(8, "little")
        if cid not in seen:
            seen.add(cid)
            offs.append(int(r["offset"]))
            sizes.append(int(r["size"]))
            ids.append(cid)
    bundle_of, nb = plan_bundles(sizes, max_payload=512 << 10)
    assert nb >= 8
    d_payload = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    comp.gather(d.data_ptr(), offs, sizes, d_payload.data_ptr())
    pay_size = np.bincount(bundle_of, weights=sizes, minlength=nb).astype(np.uint64)
    pay_off = np.concatenate([[0], np.cumsum(pay_size)[:-1]]).astype(np.uint64)
    z_off = np.concatenate([[0], np.cumsum([comp.xz_capacity(int(s)) for s in pay_size])]).astype(np.uint64)
    d_z = torch.empty(int(z_off[-1]), dtype=torch.uint8, device="cuda")
    z_size = comp.compress_xz(d_payload.data_ptr(), pay_off, pay_size, d_z.data_ptr(), z_off[:-1])
    assert int(z_size.sum()) < int(pay_size.sum())
    rng = np.random.default_rng(24)
    infos = [[(ids[i], sizes[i]) for i in np.nonzero(bundle_of == k)[0]] for k in range(nb)]
    for key in (KEY, None):
        lead = rng.integers(0, 256, 16, dtype=np.uint8).tobytes() if key else b""
        prefixes = [lead + aes_ref.message(b"\x08\x01") +
                    aes_ref.message(b"".join(cid + n.to_bytes(4, "little") for cid, n in info)) for info in infos]
        fsize = [bundle_file_size(len(p), int(z), key is not None) for p, z in zip(prefixes, z_size)]
        room = [(n + 15) & ~15 for n in fsize]  # a file begins 16-byte aligned
        f_off = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        d_files = torch.empty(int(sum(room)), dtype=torch.uint8, device="cuda")
        assert [int(s) for s in comp.seal(key, prefixes, d_z.data_ptr(), z_off[:-1], z_size, d_files.data_ptr(),
                                          f_off)] == fsize
        files = d_files.cpu().numpy()
        order = [int(k) for k in rng.permutation(nb)]
        unsealed = comp.unseal_host(key, [files[int(f_off[k]):int(f_off[k]) + fsize[k]].tobytes() for k in order])
        read_infos = []
        for (hdr, info, body), k in zip(unsealed, order):
            assert hdr == b"\x08\x01" and len(body) == int(z_size[k])
            read_infos.append([(info[i:i + 24], int.from_bytes(info[i + 24:i + 28], "little"))
                               for i in range(0, len(info), 28)])
            assert read_infos[-1] == infos[k]
        with Restorer(ctx=comp._ctx) as rs:
            plan = rs.plan(backup_data, read_infos)
            assert plan.length == len(data)
            used = [unsealed[b][2] for b in plan.used]
            d_work = torch.full((plan.bodies_work_size(used),), CANARY, dtype=torch.uint8, device="cuda")
            d_out = torch.full((len(data) + 32,), CANARY, dtype=torch.uint8, device="cuda")
            n = rs.replay_bodies(plan, used, d_work.data_ptr(), d_out.data_ptr() + 16, len(data))
        assert n == len(data)
        out = d_out.cpu().numpy()
        assert (out[:16] == CANARY).all() and (out[16 + n:] == CANARY).all()
        assert np.array_equal(out[16:16 + n], data)
        assert hashlib.sha256(out[16:16 + n].tobytes()).digest() == hashlib.sha256(data.tobytes()).digest()
