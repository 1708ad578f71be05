"""GPU tests of the resident chunk index, through the C ABI (ChunkIndex,
Restorer.plan_index, IndexedRestorer.from_index): the device's answers equal
tests/resolve_ref.py's word for word -- every record's owner and offset, every
bundle's payload size and duplicate flag, every fetched plan array, the counts
-- on the cases of tests/resolve_cases.py; an index built from a live
zc_index_set equals the one built from its fetched arrays; and a repository
written on the GPU restores from its file bytes alone."""
import hashlib

import numpy as np
import pytest

from tests import aes_ref
from tests import resolve_cases as C
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xEE
KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d7781")
PLAN_ARRAYS = ("used", "used_size", "slot", "off", "size", "dst")
PLAN_COUNTS = ("n_entries", "n_used", "length", "n_missing", "first_missing", "n_dup_used", "first_dup")


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


def make_index(comp, bundles):
    from zbackup_amd import ChunkIndex
    ids, sizes, first = C.arrays(bundles)
    return ChunkIndex.from_arrays(ids, sizes, first, ctx=comp._ctx)


def assert_index(cx, ix, strangers=()):
    """Counts, per-bundle sizes and flags, and findChunk for every record and
    for ids the index does not hold."""
    assert cx.counts() == R.counts(ix)
    size, dup = cx.bundles()
    assert size.dtype == np.uint64 and size.tolist() == ix["bundle_size"]
    assert dup.tolist() == ix["dup"]
    keys = [bytes(c) for b in ix["bundles"] for c, _ in b] + list(strangers)
    if not keys:
        b, off, sz = cx.lookup(np.zeros((0, 24), dtype=np.uint8))
        assert len(b) == len(off) == len(sz) == 0
        return
    want = [R.lookup(ix, c) for c in keys]
    b, off, sz = cx.lookup(np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 24))
    for name, got, col in (("bundle", b, 0), ("off", off, 1), ("size", sz, 2)):
        w = np.array([x[col] for x in want], dtype=np.uint64)
        if not np.array_equal(got.astype(np.uint64), w):
            at = int(np.nonzero(got.astype(np.uint64) != w)[0][0])
            raise AssertionError(f"lookup {name}[{at}] = {got[at]}, expected {w[at]}")


def assert_plan(got, ref):
    for name in PLAN_COUNTS:
        assert getattr(got, name) == ref[name], f"{name}: {getattr(got, name)}, expected {ref[name]}"
    for name in PLAN_ARRAYS:
        g, w = getattr(got, name), np.asarray(ref[name], dtype=np.uint64)
        assert g.shape == w.shape, f"{name}: {g.shape} entries, {w.shape} expected"
        if not np.array_equal(g.astype(np.uint64), w):
            at = int(np.nonzero(g.astype(np.uint64) != w)[0][0])
            raise AssertionError(f"{name}[{at}] = {g[at]}, expected {w[at]}")


def run_case(comp, case, monkeypatch):
    if case["bits"] is not None:
        monkeypatch.setenv("ZC_TEST_RESOLVE_BITS", str(case["bits"]))
    ix = R.build(case["bundles"])
    with make_index(comp, case["bundles"]) as cx:
        build_stats = cx.last_stats()
        assert_index(cx, ix, strangers=case.get("strangers", ()))
        got = cx.resolve(C.instructions(case["entries"]), case["data_len"])
        assert_plan(got, R.resolve(ix, case["entries"]))
        return got, build_stats, cx.last_stats()


@pytest.mark.parametrize("n", C.SCAN_EDGES)
def test_scan_edges(comp, monkeypatch, n):
    """n records and n entries: below, at and above a wave, a workgroup and --
    at 65,537 -- the tiles' second level."""
    got, build, _ = run_case(comp, C.scan_edge(n), monkeypatch)
    assert got.n_entries == n and build["table_slots"] >= max(2 * n, 2)


@pytest.mark.parametrize("make", C.SMALL, ids=[f.__name__ for f in C.SMALL])
def test_named_cases(comp, monkeypatch, make):
    case = make()
    got, build, last = run_case(comp, case, monkeypatch)
    if case["bits"] is not None:
        assert build["table_slots"] == last["table_slots"] == 1 << case["bits"]
    if "min_probe" in case:
        # the group alone fills min_probe slots in a row: its last member's walk is that long
        assert build["max_probe"] >= case["min_probe"] and last["max_probe"] >= case["min_probe"]
        assert last["max_probe"] <= 1 << case["bits"]
    for name in ("n_missing", "first_missing", "n_dup_used", "first_dup"):
        if name in case:
            assert getattr(got, name) == case[name]


def test_more_tiles_than_one_round_of_the_tile_scan(comp, monkeypatch):
    """256 tiles of 1,024 values are one round of the second level: 263,000
    records and entries take two, with a carry between them."""
    rng = np.random.default_rng(53)
    n = 263000
    raw = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    sizes = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    first = np.concatenate([np.arange(0, n, 517), [n]]).astype(np.uint64)
    from zbackup_amd import ChunkIndex
    with ChunkIndex.from_arrays(raw, sizes, first, ctx=comp._ctx) as cx:
        size, dup = cx.bundles()
        run = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))])
        assert np.array_equal(size, run[first[1:].astype(np.int64)] - run[first[:-1].astype(np.int64)])
        assert not dup.any() and cx.counts()["ids"] == n
        b, off, sz = cx.lookup(raw)
        rec = np.arange(n)
        want_b = np.searchsorted(first, rec, side="right") - 1
        assert np.array_equal(b, want_b) and np.array_equal(sz, sizes)
        assert np.array_equal(off, run[:-1] - run[first[want_b].astype(np.int64)])
        ins = np.zeros(n, dtype=C.INSTR)
        pick = rng.integers(0, n, n)
        ins["id"] = raw[pick]
        got = cx.resolve(ins, 0)
        assert got.n_missing == 0 and got.n_used == len(np.unique(want_b[pick]))
        assert np.array_equal(got.used, np.unique(want_b[pick]))
        assert np.array_equal(got.size, sizes[pick].astype(np.uint64))
        assert np.array_equal(got.dst, np.concatenate([[0], np.cumsum(got.size)[:-1]]))
        assert got.length == int(got.size.sum())
        assert np.array_equal(got.used[got.slot], want_b[pick])


def test_repeated_resolves_and_two_indices_on_one_context(comp, monkeypatch):
    a, b = C.scan_edge(257), C.shapes()
    ia, ib = R.build(a["bundles"]), R.build(b["bundles"])
    with make_index(comp, a["bundles"]) as ca, make_index(comp, b["bundles"]) as cb:
        for turn in range(3):
            assert_plan(ca.resolve(C.instructions(a["entries"]), a["data_len"]), R.resolve(ia, a["entries"]))
            assert_plan(cb.resolve(C.instructions(b["entries"]), b["data_len"]), R.resolve(ib, b["entries"]))
            # a's stream against b's index: every chunk misses, the bytes runs stay
            cross = cb.resolve(C.instructions(a["entries"]), a["data_len"])
            assert_plan(cross, R.resolve(ib, a["entries"]))
            assert cross.n_missing == sum(1 for e in a["entries"] if e[0] == "chunk")
        assert_index(ca, ia)
        assert_index(cb, ib)


def test_python_errors_name_the_id_and_the_bundle(comp):
    from zbackup_amd import BundleInfos, ChunkIndex, Restorer, ZcError, serialize_instruction
    case = C.dup_used()
    x, z, y = (case["entries"][k][1] for k in (0, 1, 2))
    gone = bytes(range(24))
    # from_bundles: what a caller who holds only bundle files has, as lists or as a BundleInfos
    ids, sizes, first = C.arrays(case["bundles"])
    infos = BundleInfos(ids, sizes, first, np.zeros(len(first) - 1, dtype=np.uint8))
    with ChunkIndex.from_bundles(infos, ctx=comp._ctx) as cx:
        assert_index(cx, R.build(case["bundles"]))
    with ChunkIndex.from_bundles(case["bundles"], ctx=comp._ctx) as cx:
        assert_index(cx, R.build(case["bundles"]))
        plan = Restorer.plan_index(serialize_instruction(chunk_blob=x) + serialize_instruction(raw=b"abc") +
                                   serialize_instruction(chunk_blob=z), cx)
        assert plan.used == [0, 1] and plan.length == 9 + 3 + 4 and plan.pay_off == [0, 16] and plan.instr_off == 32
        with pytest.raises(ZcError, match=gone.hex()):
            Restorer.plan_index(serialize_instruction(chunk_blob=x) + serialize_instruction(chunk_blob=gone), cx)
        with pytest.raises(ZcError, match="bundle 2: a chunk id twice"):
            Restorer.plan_index(serialize_instruction(chunk_blob=x) + serialize_instruction(chunk_blob=y), cx)


def test_index_from_a_live_set_equals_the_one_from_its_arrays(comp):
    """Index files written by write_index, with and without a key; one file
    with a bad Adler-32 contributes nothing."""
    from zbackup_amd import ChunkIndex, IndexLoader, write_index
    rng = np.random.default_rng(59)
    case = C.scan_edge(257)
    more = C.dup_used()["bundles"] + C.shapes()["bundles"][:4]
    groups = [case["bundles"][:9], more, [], case["bundles"][9:]]
    named = [[(rng.integers(0, 256, 24, dtype=np.uint8).tobytes(), recs) for recs in g] for g in groups]
    for key in (None, KEY):
        files = [write_index(g, key=key, r=bytes(rng.integers(0, 256, 16, dtype=np.uint8)) if key else None, comp=comp)
                 for g in named]
        spoiled = bytearray(write_index(named[1], key=None)) if key is None else None
        if spoiled is not None:
            spoiled[-1] ^= 1  # the stored Adler-32
            files.insert(2, bytes(spoiled))
        with IndexLoader(ctx=comp._ctx, key=key) as loader, loader.load_resident(files) as live:
            host = live.fetch()
            if spoiled is not None:
                assert host.status_names[2] == "Adler-32 mismatch" and host.index_first[2] == host.index_first[3]
            assert not np.delete(host.status, 2).any() if spoiled is not None else not host.status.any()
            bundles = [recs for g in groups for recs in g]
            assert live.n_records == sum(len(b) for b in bundles) and live.n_bundles == len(bundles)
            ix = R.build(bundles)
            with ChunkIndex.from_index_set(live) as cs, \
                    ChunkIndex.from_arrays(host.ids, host.sizes, host.bundle_first, ctx=comp._ctx) as ch:
                assert_index(cs, ix)
                assert_index(ch, ix)
                ins = C.instructions(case["entries"])
                ref = R.resolve(ix, case["entries"])
                assert_plan(cs.resolve(ins, case["data_len"]), ref)
                assert_plan(ch.resolve(ins, case["data_len"]), ref)
        # an empty set
        with IndexLoader(ctx=comp._ctx, key=key) as loader, loader.load_resident([]) as live:
            with ChunkIndex.from_index_set(live) as cs:
                assert cs.counts() == {"records": 0, "bundles": 0, "ids": 0, "flagged": 0}


def test_restore_from_file_bytes_alone(torch_cuda, comp):
    """chunk, bundle, compress_xz, seal, write_index; then from the files'
    bytes: load_resident -> ChunkIndex -> plan_index -> unseal the used bundles
    -> replay_bodies, and IndexedRestorer.from_index for ranges."""
    from zbackup_amd import (ZC_CHUNK_NEW, BackupCreator, ChunkIndex, IndexedRestorer, IndexLoader, Restorer,
                             parse_backup_data, write_index)
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
    rng = np.random.default_rng(61)
    infos = [[(ids[i], sizes[i]) for i in np.nonzero(bundle_of == k)[0]] for k in range(nb)]
    bundle_ids = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in range(nb)]
    want_sha = hashlib.sha256(data.tobytes()).digest()
    entries = parse_backup_data(backup_data)
    for key in (KEY, None):
        lead = rng.integers(0, 256, 16, dtype=np.uint8).tobytes() if key else b""
        prefixes = [lead + aes_ref.message(b"\x08\x01") + aes_ref.message(b"".join(c + bytes(4) for c, _ in info))
                    for info in infos]
        fsize = [bundle_file_size(len(p), int(z), key is not None) for p, z in zip(prefixes, z_size)]
        room = [(n + 15) & ~15 for n in fsize]
        f_off = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        d_files = torch.empty(int(sum(room)), dtype=torch.uint8, device="cuda")
        comp.seal(key, prefixes, d_z.data_ptr(), z_off[:-1], z_size, d_files.data_ptr(), f_off)
        all_files = d_files.cpu().numpy()
        # the repository as it lies on disk: bundle files by bundle id, two index files
        bundle_files = {bundle_ids[k]: all_files[int(f_off[k]):int(f_off[k]) + fsize[k]].tobytes() for k in range(nb)}
        cut = nb // 2 + 1
        index_files = [write_index([(bundle_ids[k], infos[k]) for k in ks], key=key,
                                   r=bytes(rng.integers(0, 256, 16, dtype=np.uint8)) if key else None, comp=comp)
                       for ks in (range(cut, nb), range(cut))]  # the later bundles' file is read first
        del all_files, d_files

        # ---- from here on only index_files, bundle_files, backup_data and the key ----
        with IndexLoader(ctx=comp._ctx, key=key) as loader, loader.load_resident(index_files) as live:
            names = live.fetch().bundle_ids  # which file a bundle number is
            with ChunkIndex.from_index_set(live) as cx, Restorer(ctx=comp._ctx) as rs:
                assert cx.counts() == {"records": len(ids), "bundles": nb, "ids": len(ids), "flagged": 0}
                plan = rs.plan_index(backup_data, cx)
                assert plan.length == len(data) and plan.used == sorted(plan.used) and len(plan.used) == nb
                assert all(o % 16 == 0 for o in plan.pay_off)
                unsealed = comp.unseal_host(key, [bundle_files[names[b].tobytes()] for b in plan.used])
                bodies = [body for _, _, body in unsealed]
                d_work = torch.full((plan.bodies_work_size(bodies),), CANARY, dtype=torch.uint8, device="cuda")
                d_out = torch.full((len(data) + 32,), CANARY, dtype=torch.uint8, device="cuda")
                n = rs.replay_bodies(plan, bodies, d_work.data_ptr(), d_out.data_ptr() + 16, len(data))
                assert n == len(data)
                out = d_out.cpu().numpy()
                assert (out[:16] == CANARY).all() and (out[16 + n:] == CANARY).all()
                assert hashlib.sha256(out[16:16 + n].tobytes()).digest() == want_sha
                # ranges that cross bundle and bytes_to_emit borders
                with IndexedRestorer.from_index(backup_data, cx) as ir:
                    assert ir.size == len(data)
                    ends = np.cumsum(plan.sizes).astype(np.int64)
                    slot_change = [int(ends[k]) for k in range(len(ends) - 1) if plan.slot[k] != plan.slot[k + 1]]
                    raw = [int(plan.dst_off[k]) for k in range(len(entries)) if entries[k]["kind"] == 1]
                    reads = [(max(p - 700, 0), 1400) for p in slot_change[:3] + slot_change[-2:] + raw[:2]]
                    reads += [(0, 1), (len(data) - 5, 5), (len(data), 0), (123457, 70001)]
                    reads = [(o, min(s, len(data) - o)) for o, s in reads]
                    for b in ir.needs(reads):
                        ir.decode_payload(b, unseal_one(comp, key, bundle_files[names[b].tobytes()]))
                    for o, s in reads:
                        assert ir.read_host(o, s) == data[o:o + s].tobytes(), (o, s)


def unseal_one(comp, key, file_bytes):
    return comp.unseal_host(key, [file_bytes])[0][2]
