"""GPU tests of the index-file loader (zc_index.hip): every array of every case
is compared word for word with tests/index_ref.py -- ids, sizes, bundle_first,
bundle_ids, index_first and the status of every file.  The shapes are the
smallest that reach each edge: empty and tiny files, the varint edges of the
lengths and sizes, both field orders, every offset of a header and a record
against the LDS tile's edge (ZC_TEST_INDEX_TILE), the lane and the wave path of
the record kernels side by side (ZC_TEST_INDEX_WAVE_MIN), bad files among good
ones, a few hundred mutations, unsealed bundle files, and the way from
write_index to a garbage collection plan."""
import random

import numpy as np
import pytest

from tests import aes_ref
from tests import index_ref as R

pytestmark = pytest.mark.gpu

KEY = bytes(range(0x40, 0x50))
RND = bytes(range(0xA0, 0xB0))
EDGE_SIZES = [0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28, 2 ** 32 - 1]
ARRAYS = ("status", "index_first", "bundle_ids", "bundle_first", "sizes", "ids")
KEYS = pytest.mark.parametrize("key", [None, KEY], ids=["plain", "keyed"])


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


def loader(comp, key):
    from zbackup_amd import IndexLoader
    return IndexLoader(ctx=comp._ctx, key=key)


def assert_same(got, ref, what=""):
    for name in ARRAYS:
        g, w = getattr(got, name), ref[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            pytest.fail(f"{what}: {name} differs first at {at.tolist()}: {g[tuple(at)]} != {w[tuple(at)]}")


def check(comp, files, key, what=""):
    got = loader(comp, key).load(files)
    ref = R.read_many(files, key)
    assert_same(got, ref, what)
    return got, ref


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    monkeypatch.delenv("ZC_TEST_INDEX_TILE", raising=False)
    monkeypatch.delenv("ZC_TEST_INDEX_WAVE_MIN", raising=False)


@KEYS
def test_empty_and_tiny_files(comp, key):
    rng = random.Random(10)
    files = [R.write([], key, RND)]
    for n in (0, 1, 15, 16, 32):
        files += [bytes(n), bytes(rng.getrandbits(8) for _ in range(n))]
    files += [R.write([], key, RND), R.write(R.rand_bundles(rng, [0]), key, RND),
              R.write(R.rand_bundles(rng, [1]), key, RND)]
    got, ref = check(comp, files, key)
    assert got.status[0] == 0 and got.index_first[1] == 0 and got.status[-1] == 0 and len(got.sizes) == 1
    assert loader(comp, key).load([]).status.shape == (0,)


@KEYS
@pytest.mark.parametrize("size_first", [False, True, [True, False, False]], ids=["id-size", "size-id", "mixed"])
def test_varint_edges_and_field_orders(comp, key, size_first):
    """BundleInfo lengths on both sides of the 1-, 2- and 3-byte varint (4, 5
    and 600 records), every size on a varint edge, both field orders."""
    rng = random.Random(11)
    bundles = R.rand_bundles(rng, [4, 5], [5]) + R.rand_bundles(rng, [600, 0, 1], EDGE_SIZES)
    bundles.append((R.rand_id(rng), [(R.rand_id(rng), s) for s in EDGE_SIZES]))
    lens = [len(R.bundle_info(r, size_first)) for _, r in bundles]
    assert lens[0] < 128 <= lens[1] < 16384 <= lens[2]
    got, _ = check(comp, [R.write(bundles, key, RND, size_first=size_first)], key)
    assert got.status[0] == 0 and got.sizes[-len(EDGE_SIZES):].tolist() == EDGE_SIZES


def _sweep_files(rng, key):
    """64 files whose first BundleInfo is 0..63 bytes longer from one to the
    next (by record count and the sizes' varints), so that what follows it --
    a bundle header, then records -- starts at every offset against a tile's edge."""
    files, lens = [], []
    for d in range(64):
        k, extra = (8, d) if d <= 32 else (9, d - 30)
        recs = []
        for _ in range(k):
            e = min(4, extra)
            extra -= e
            recs.append((R.rand_id(rng), [5, 128, 16384, 2 ** 21, 2 ** 28][e]))
        assert extra == 0
        lens.append(len(R.bundle_info(recs)))
        bundles = [(R.rand_id(rng), recs)] + R.rand_bundles(rng, [3, 0, 2])
        if d % 16 == 5:
            bundles.insert(2, R.rand_bundles(rng, [40])[0])  # longer than several 256-byte tiles
        files.append(R.write(bundles, key, RND, size_first=[False, True]))
    assert lens == list(range(240, 304))
    return files


@KEYS
@pytest.mark.parametrize("wave_min", [1, None], ids=["wave", "lane"])
def test_tile_edges(comp, monkeypatch, key, wave_min):
    monkeypatch.setenv("ZC_TEST_INDEX_TILE", "256")
    if wave_min:
        monkeypatch.setenv("ZC_TEST_INDEX_WAVE_MIN", str(wave_min))
    got, _ = check(comp, _sweep_files(random.Random(12), key), key)
    assert (got.status == 0).all()
    monkeypatch.setenv("ZC_TEST_INDEX_TILE", "128")  # the smallest tile: barely more than one record
    check(comp, _sweep_files(random.Random(13), key)[:8], key)


@KEYS
def test_lane_and_wave_paths_side_by_side(comp, monkeypatch, key):
    """One bundle of 5,000 records between 300 bundles of 0-3 records: with
    the threshold at 100 bytes the bundles of 0-3 records stay with a lane and
    everything longer takes a wave; then the same file with the default."""
    rng = random.Random(14)
    counts = [rng.randrange(4) for _ in range(150)] + [5000] + [rng.randrange(4) for _ in range(150)]
    f = R.write(R.rand_bundles(rng, counts, EDGE_SIZES + [65536] * 9), key, RND, size_first=[False, False, True])
    monkeypatch.setenv("ZC_TEST_INDEX_WAVE_MIN", "100")
    got, _ = check(comp, [f], key)
    assert got.status[0] == 0 and len(got.sizes) == sum(counts)
    monkeypatch.delenv("ZC_TEST_INDEX_WAVE_MIN")
    check(comp, [f], key)
    monkeypatch.setenv("ZC_TEST_INDEX_TILE", "256")
    check(comp, [f, f], key)


@KEYS
def test_every_crafted_fault(comp, monkeypatch, key):
    """Every rule of the strict reader broken once, all in one call."""
    bad = R.bad_files(key, RND)
    got, ref = check(comp, [d for _, d, _ in bad], key)
    for k, (name, _, status) in enumerate(bad):
        assert got.status[k] == status, name
    monkeypatch.setenv("ZC_TEST_INDEX_WAVE_MIN", "1")
    monkeypatch.setenv("ZC_TEST_INDEX_TILE", "128")
    check(comp, [d for _, d, _ in bad], key)


@KEYS
def test_mixed_statuses(comp, key):
    """40 files, every third one bad with a status of each kind: the good
    files' records are unharmed and dense, the bad files contribute nothing."""
    rng = random.Random(15)
    by_status = {}
    for _, d, s in R.bad_files(key, RND):
        if s != R.OK:
            by_status.setdefault(s, d)
    kinds = sorted(by_status)
    assert kinds == [s for s in range(1, 9) if key is not None or s != R.BAD_PADDING]
    files, bad_at = [], []
    for i in range(40):
        if i % 3 == 1:
            bad_at.append(i)
            files.append(by_status[kinds[len(bad_at) % len(kinds)]])
        else:
            files.append(R.write(R.rand_bundles(rng, [rng.randrange(5) for _ in range(rng.randrange(4))]), key, RND))
    got, ref = check(comp, files, key)
    assert set(got.status[bad_at].tolist()) == set(kinds)
    for i in bad_at:
        assert got.index_first[i + 1] == got.index_first[i]
    good = [i for i in range(40) if i not in bad_at]
    assert (got.status[good] == 0).all()
    # only good files: the same records
    assert_same(loader(comp, key).load([files[i] for i in good]), R.read_many([files[i] for i in good], key))


@KEYS
@pytest.mark.parametrize("hooks", [False, True], ids=["default", "small-tile-wave"])
def test_mutations(comp, monkeypatch, key, hooks):
    """About 300 single-byte flips and truncations of one small valid file;
    for half of them the Adler-32 is right again after the change."""
    if hooks:
        monkeypatch.setenv("ZC_TEST_INDEX_TILE", "128")
        monkeypatch.setenv("ZC_TEST_INDEX_WAVE_MIN", "40")
    rng = random.Random(16)
    base = R.body(R.rand_bundles(rng, [2, 0, 3, 1], EDGE_SIZES), size_first=[False, True])
    files = R.mutations(base, key, RND, count=300)
    got, ref = check(comp, files, key)
    seen = set(got.status.tolist())
    assert {R.OK, R.TRUNCATED, R.BAD_MESSAGE, R.BAD_ADLER} <= seen, seen


def test_unkeyed_trailing_bytes_are_ignored(comp):
    rng = random.Random(17)
    b = R.rand_bundles(rng, [3, 1])
    files = [R.seal(R.body(b), None, trailing=bytes(rng.getrandbits(8) for _ in range(n))) for n in (1, 15, 16, 300)]
    got, _ = check(comp, files, None)
    assert (got.status == 0).all() and len(got.sizes) == 16


@KEYS
def test_files_in_device_memory(torch_cuda, comp, monkeypatch, key):
    """zc_index_load proper: the files already in HBM; without a key at odd
    offsets, so that neither the tiles nor the lanes' words start aligned."""
    rng = random.Random(18)
    files = [R.write(R.rand_bundles(rng, [rng.randrange(70) for _ in range(rng.randrange(1, 5))], EDGE_SIZES), key,
                     RND, size_first=[True, False]) for _ in range(9)]
    files.insert(4, b"")
    files.append(R.bad_files(key, RND)[3][1])
    step = 16 if key is not None else 1
    off, pos = [], 3 if key is None else 0
    for f in files:
        off.append(pos)
        pos += (len(f) + step - 1) // step * step + (0 if key is not None else 5)
    img = np.zeros(pos + 16, dtype=np.uint8)
    for o, f in zip(off, files):
        img[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d = torch_cuda.from_numpy(img).to("cuda:0")
    ld = loader(comp, key)
    for tile in (None, "256"):
        if tile:
            monkeypatch.setenv("ZC_TEST_INDEX_TILE", tile)
            monkeypatch.setenv("ZC_TEST_INDEX_WAVE_MIN", "300")
        got = ld.load_device(d.data_ptr(), off, [len(f) for f in files])
        assert_same(got, R.read_many(files, key), f"tile {tile}")
    st = ld.last_stats()
    assert st["total_ms"] > 0 and st["frame_ms"] > 0 and st["records_ms"] > 0
    if key is not None:
        assert st["decrypt_ms"] > 0


@KEYS
def test_a_warm_context_keeps_nothing(comp, key):
    """A smaller and then a larger set on the context the first call warmed:
    scratch of the earlier call must not show through."""
    rng = random.Random(19)
    big = [R.write(R.rand_bundles(rng, [rng.randrange(40) for _ in range(6)]), key, RND) for _ in range(12)]
    small = [R.write(R.rand_bundles(rng, [2]), key, RND), R.bad_files(key, RND)[5][1]]
    bigger = big + [R.write(R.rand_bundles(rng, [700, 3]), key, RND)] + small
    ld = loader(comp, key)
    for files in (big, small, bigger, small, []):
        assert_same(ld.load(files), R.read_many(files, key))


@KEYS
def test_bundle_info_parse_over_unsealed_bundles(torch_cuda, comp, key):
    """Bundles sealed by BundleCompressor.seal and unsealed by zc_bundle_unseal:
    the record kernels over the layouts' BundleInfo give back what went in."""
    from zbackup_amd.bundle import bundle_file_size
    rng = random.Random(20)
    keyed = key is not None
    counts = [0, 1, 32, 3, 700, 32]
    bundles = [recs for _, recs in R.rand_bundles(rng, counts, [1, 127, 128, 16383, 16384, 65536])]
    bodies = [bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 200))) for _ in counts]
    prefixes = [(RND if keyed else b"") + R.message(b"\x08\x01") + R.message(R.bundle_info(recs, [False, True]))
                for recs in bundles]
    body_len = [len(b) for b in bodies]
    body_off = np.concatenate([[0], np.cumsum(body_len)[:-1]])
    fsize = [bundle_file_size(len(p), n, keyed) for p, n in zip(prefixes, body_len)]
    cap = [(s + 15) // 16 * 16 for s in fsize]
    file_off = np.concatenate([[0], np.cumsum(cap)[:-1]])
    d_body = torch_cuda.from_numpy(np.frombuffer(b"".join(bodies), dtype=np.uint8).copy()).to("cuda:0")
    d_files = torch_cuda.zeros(sum(cap), dtype=torch_cuda.uint8, device="cuda:0")
    d_plain = torch_cuda.zeros(sum(cap), dtype=torch_cuda.uint8, device="cuda:0")
    comp.seal(key, prefixes, d_body.data_ptr(), body_off, body_len, d_files.data_ptr(), file_off)
    layout = comp.unseal(key, d_files.data_ptr(), file_off, fsize, d_plain.data_ptr(), file_off)
    assert (layout["status"] == 0).all()
    ld = loader(comp, key)
    info_off = file_off.astype(np.uint64) + layout["info_off"]
    want = R.arrays([[(b"\0" * 24, recs) for recs in bundles]])
    for dev in (True, False):
        if dev:
            got = ld.bundle_infos_device(d_plain.data_ptr(), info_off, layout["info_len"])
        else:
            lay = layout.copy()
            lay["info_off"] = info_off
            got = ld.bundle_infos(lay, d_plain.cpu().numpy())
        assert (got.status == 0).all() and len(got) == len(bundles)
        for name in ("ids", "sizes", "bundle_first"):
            assert np.array_equal(getattr(got, name), want[name]), (dev, name)
        assert list(got) == bundles and got[4] == bundles[4]
    # a broken BundleInfo among good ones: its status, no records of its own
    plain = bytearray(d_plain.cpu().numpy().tobytes())
    plain[int(info_off[2])] ^= 0xFF  # the first record's tag
    with pytest.raises(R.Bad) as bad:
        R.read_bundle_info(bytes(plain), int(info_off[2]), int(info_off[2] + layout["info_len"][2]))
    status = bad.value.status
    lay = layout.copy()
    lay["info_off"] = info_off
    got = ld.bundle_infos(lay, bytes(plain))
    assert got.status.tolist() == [0, 0, status, 0, 0, 0] and got[2] == [] and got[3] == bundles[3]
    assert got[4] == bundles[4] and len(got.sizes) == sum(counts) - 32
    # what Restorer.plan and Adopter.adopt take
    from zbackup_amd import Restorer
    from zbackup_amd.adopt import bundle_layout
    from zbackup_amd.restore import chunk_map
    good = ld.bundle_infos_device(d_plain.data_ptr(), info_off, layout["info_len"])
    assert chunk_map(good) == chunk_map(bundles) and Restorer.plan(b"", good).length == 0
    pays = [bytes(sum(n for _, n in recs)) for recs in bundles[:4]]
    for a, b in zip(bundle_layout(good[:4], pays), bundle_layout(bundles[:4], pays)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@KEYS
def test_write_index_matches_the_reference_writer(comp, key):
    from zbackup_amd import write_index
    rng = random.Random(21)
    for counts in ([], [0], [1, 5, 130], [600]):
        b = R.rand_bundles(rng, counts, EDGE_SIZES)
        f = write_index(b, key=key, r=RND, comp=comp)
        assert f == R.write(b, key, RND)
        if key is not None:
            assert aes_ref.cbc_decrypt(key, bytes(16), f)[:16] == RND


@KEYS
def test_from_the_files_to_a_gc_plan(comp, key):
    """write_index -> IndexLoader.load -> Collector.plan_index gives the plan
    Collector.plan gives for the lists."""
    from zbackup_amd import Collector, write_index
    rng = random.Random(22)
    indexes = [R.rand_bundles(rng, [rng.randrange(6) for _ in range(rng.randrange(1, 6))]) for _ in range(5)]
    indexes.append([])
    used = [c for bundles in indexes for _, recs in bundles for c, _ in recs if rng.randrange(3)]
    files = [write_index(b, key=key, r=RND, comp=comp) for b in indexes]
    iset = loader(comp, key).load(files)
    assert (iset.status == 0).all() and iset.status_names == ["ok"] * 6 and iset.bundles() == indexes
    plans = []
    for how in ("index", "lists"):
        col = Collector(ctx=comp._ctx)
        col.mark_ids(used)
        kw = dict(deep=True, max_payload=200000)
        plans.append(col.plan_index(iset, **kw) if how == "index" else col.plan(indexes, **kw))
    for name in plans[0].__slots__:
        a, b = getattr(plans[0], name), getattr(plans[1], name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert len(plans[0].copy) > 0
