"""GPU tests of garbage collection, through the C ABI: every output array of
zc_gc_plan equals tests/gc_ref.py's (a restatement of BundleCollector with
Python sets) exactly -- on empty and one-record inputs, at wave and table
capacity edges with the default table and with ZC_TEST_GC_BITS forcing the
smallest legal one, on near-equal ids, on one id 5,000 times over, on a random
repository under all eight flag combinations, on 2^20 records -- and a
collected repository restores the kept backup byte for byte."""
import hashlib

import numpy as np
import pytest

from oracle import lzo_oracle
from tests import gc_ref
from tests.lzo_inputs import payload

pytestmark = pytest.mark.gpu

CANARY = 0xEE
ARRAYS = ("record_flags", "bundle_total", "bundle_used", "bundle_action", "copy", "copy_bundle", "copy_off",
          "new_bundle_index", "new_bundle_size")
INDEX_FIELDS = ("total", "used", "kept", "modified_bundles", "removed", "modified", "necessary", "unlink")


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


def collector(comp, used):
    from zbackup_amd import Collector
    col = Collector(ctx=comp._ctx)
    col.mark_ids(used if isinstance(used, np.ndarray) else list(used))
    return col


def assert_equal(plan, ref):
    for name in ARRAYS:
        got, want = getattr(plan, name), np.asarray(ref[name], dtype=np.uint64)
        assert got.shape == want.shape, f"{name}: {got.shape} entries, {want.shape} expected"
        if not np.array_equal(got.astype(np.uint64), want):
            at = int(np.nonzero(got.astype(np.uint64) != want)[0][0])
            raise AssertionError(f"{name}[{at}] = {got[at]}, expected {want[at]}")
    assert len(plan.indexes) == len(ref["indexes"])
    for i, x in enumerate(ref["indexes"]):
        for f in INDEX_FIELDS:
            assert int(plan.indexes[i][f]) == int(x[f]), f"index file {i}: {f}"
    assert plan.files_to_unlink() == gc_ref.files_to_unlink(ref)


def plan_bytes(plan):
    return b"".join(getattr(plan, name).tobytes() for name in ARRAYS) + plan.indexes.tobytes()


def check(comp, indexes, used, flags=0, max_payload=gc_ref.MAX_PAYLOAD_SIZE):
    """One zc_gc_plan call against gc_ref; returns (plan, ref, stats)."""
    ref = gc_ref.plan(indexes, used, flags, max_payload)
    col = collector(comp, used)
    plan = col.plan(indexes, deep=bool(flags & gc_ref.DEEP), repack=bool(flags & gc_ref.REPACK),
                    concat=bool(flags & gc_ref.CONCAT), max_payload=max_payload)
    assert_equal(plan, ref)
    return plan, ref, col.last_stats()


def random_ids(rng, n):
    return [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in range(n)]


def random_indexes(rng, n_records, pool, size_of, n_indexes=2, max_records=9):
    """n_records records drawn from pool, in bundles of 0..max_records, over n_indexes index files."""
    bundles, left = [], n_records
    while left:
        k = min(int(rng.integers(0, max_records + 1)), left)
        recs = [pool[int(j)] for j in rng.integers(0, len(pool), k)]
        bundles.append((rng.integers(0, 256, 24, dtype=np.uint8).tobytes(), [(c, size_of[c]) for c in recs]))
        left -= k
    cuts = [len(bundles) * i // n_indexes for i in range(n_indexes + 1)]
    return [bundles[cuts[i]:cuts[i + 1]] for i in range(n_indexes)]


def test_empty_and_single(comp):
    a, B1 = bytes(range(24)), bytes(range(100, 124))
    for flags in (0, gc_ref.DEEP, gc_ref.DEEP | gc_ref.REPACK | gc_ref.CONCAT):
        plan, _, _ = check(comp, [], [], flags)  # N = U = B = I = 0
        assert plan.copy.size == 0 and plan.indexes.size == 0
        check(comp, [[]], [], flags)  # an index file without bundles
        check(comp, [[(B1, [])]], [], flags)  # one bundle with no records
        check(comp, [[(B1, [])]], [a], flags)
        plan, _, _ = check(comp, [[(B1, [(a, 77)])]], [], flags)  # N = 1, U = 0
        assert plan.bundle_action.tolist() == [gc_ref.REMOVE]
        plan, _, _ = check(comp, [[(B1, [(a, 77)])]], [a], flags)  # N = 1, U = 1
        assert plan.record_flags[0] & gc_ref.USED
        check(comp, [[(B1, [(a, 77)])]], [bytes(24)], flags)  # U = 1, a stranger


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_wave_and_capacity_edges(comp, monkeypatch, n, forced):
    """n records, nearly all ids distinct: with the table forced to the
    smallest power of two above n, 1023 ids leave one slot of 1024 free."""
    rng = np.random.default_rng(n)
    pool = random_ids(rng, n)
    size_of = {c: int(rng.integers(1, 70000)) for c in pool}
    # every id of the pool once, three of them twice: n records in all
    recs = pool[:n - 3] + pool[:3]
    order = rng.permutation(n)
    bundles, at = [], 0
    while at < n:
        k = int(rng.integers(0, 10))
        bundles.append((random_ids(rng, 1)[0], [(recs[j], size_of[recs[j]]) for j in order[at:at + k]]))
        at += k
    indexes = [bundles[:len(bundles) // 2], bundles[len(bundles) // 2:]]
    used = [pool[int(j)] for j in rng.integers(0, n, n // 2)] + random_ids(rng, 20)
    bits = n.bit_length()  # 2^bits > n: the smallest table with a free slot
    if forced:
        monkeypatch.setenv("ZC_TEST_GC_BITS", str(bits))
    else:
        monkeypatch.delenv("ZC_TEST_GC_BITS", raising=False)
    for flags in (0, gc_ref.DEEP, gc_ref.REPACK):
        _, _, st = check(comp, indexes, used, flags, max_payload=200000)
        want_slots = 1 << bits if forced else 1 << (2 * n - 1).bit_length()
        assert st["table_slots"] == max(want_slots, 2)
        if forced:
            assert st["max_probe"] > 1  # the small table really made ids collide
        assert st["max_probe"] <= st["table_slots"]
    # out of range: ignored
    for bad in ("0", "-4", "33", str(bits - 1), "zz"):
        monkeypatch.setenv("ZC_TEST_GC_BITS", bad)
        _, _, st = check(comp, indexes, used)
        assert st["table_slots"] == 1 << (2 * n - 1).bit_length()


def test_near_equal_ids(comp, monkeypatch):
    """Ids that differ in byte 0 only, byte 23 only, the SHA-1 half only or the
    rolling-hash half only: a partial compare would merge them."""
    rng = np.random.default_rng(5)
    base = bytearray(random_ids(rng, 1)[0])
    ids = [bytes(base)]
    for v in range(1, 256):
        a, b = bytearray(base), bytearray(base)
        a[0] ^= v
        b[23] ^= v
        ids += [bytes(a), bytes(b)]
    for _ in range(100):
        ids.append(random_ids(rng, 1)[0][:16] + bytes(base[16:]))  # the SHA-1 half only
        ids.append(bytes(base[:16]) + random_ids(rng, 1)[0][:8])   # the rolling-hash half only
    assert len(set(ids)) == len(ids)
    size_of = {c: 1000 + k for k, c in enumerate(ids)}
    indexes = random_indexes(rng, 2 * len(ids), ids, size_of, n_indexes=3, max_records=7)
    used = ids[::3]
    for k in range(24):  # strangers one byte away from an id that is there
        s = bytearray(ids[1 + 7 * k])
        s[k] ^= 0x80
        if bytes(s) not in size_of:
            used.append(bytes(s))
    for bits in (None, (2 * len(ids)).bit_length()):
        if bits:
            monkeypatch.setenv("ZC_TEST_GC_BITS", str(bits))
        for flags in (0, gc_ref.DEEP, gc_ref.DEEP | gc_ref.REPACK):
            check(comp, indexes, used, flags, max_payload=50000)


def test_one_id_five_thousand_times(comp):
    """5,000 records of one id in 500 bundles over 3 index files, deep: the
    counted record is the first in processing order -- the LAST record of the
    first bundle --, the copy list holds it once, and two calls agree to the byte."""
    a = bytes(range(7, 31))
    bundles = [(bytes([k % 256, k // 256] * 12), [(a, 4096)] * 10) for k in range(500)]
    indexes = [bundles[:100], bundles[100:350], bundles[350:]]
    for flags in (gc_ref.DEEP | gc_ref.REPACK, gc_ref.DEEP, gc_ref.REPACK, 0):
        plan, ref, _ = check(comp, indexes, [a, a], flags)
        again, _, _ = check(comp, indexes, [a, a], flags)
        assert plan_bytes(plan) == plan_bytes(again)
        if flags & gc_ref.DEEP:
            assert np.nonzero(plan.record_flags & gc_ref.COUNTED)[0].tolist() == [9]
            assert plan.bundle_total.tolist() == [1] + [0] * 499
        if flags & gc_ref.REPACK:
            assert plan.copy.tolist() == [9] and plan.new_bundle_size.tolist() == [4096]
            assert (plan.bundle_action == gc_ref.REPACK_BUNDLE).all()
    # unused, deep: only the first bundle has anything to remove; the others' records are dropped
    plan, _, _ = check(comp, indexes, [], gc_ref.DEEP)
    assert plan.bundle_action[0] == gc_ref.REMOVE and plan.copy.size == 0


def random_repository():
    """5 index files, ~240 bundles of 0..40 records, ~4,000 records from a pool
    of 1,500 ids; bundle ids repeat across index files; index 2 holds used ids
    only, index 4 is a copy of index 1.  The used set: 40 % of the pool, 200
    strangers, duplicates."""
    rng = np.random.default_rng(20)
    pool = random_ids(rng, 1500)
    size_of = {c: int(rng.integers(100, 66000)) for c in pool}
    used_pool = [pool[int(j)] for j in rng.permutation(1500)[:600]]
    used = used_pool + random_ids(rng, 200) + used_pool[:150]
    rng.shuffle(used)

    def bundles_of(n_bundles, ids, bundle_ids):
        out = []
        for k in range(n_bundles):
            k_recs = int(rng.integers(0, 3)) if rng.random() < 0.2 else int(rng.integers(0, 41))  # some tiny ones
            recs = [ids[int(j)] for j in rng.permutation(len(ids))[:k_recs]]
            out.append((bundle_ids[k], [(c, size_of[c]) for c in recs]))
        return out

    names = random_ids(rng, 140)
    i0 = bundles_of(72, pool, names[:72])
    i1 = bundles_of(52, pool, names[72:124])
    i2 = [(names[124 + k], [(c, size_of[c]) for c in used_pool[10 * k:10 * k + int(rng.integers(1, 10))]])
          for k in range(8)]
    i3 = bundles_of(60, pool, names[:60])      # index 0's bundle ids again
    i4 = [(b, list(r)) for b, r in i1]         # a complete copy of index 1
    return [i0, i1, i2, i3, i4], used


def test_random_repository_all_flag_combinations(comp):
    indexes, used = random_repository()
    n_records = sum(len(r) for ix in indexes for _, r in ix)
    assert 3500 < n_records < 5000 and sum(len(ix) for ix in indexes) > 190
    seen = {"action": set(), "modified": set(), "necessary": set(), "unlink": set()}
    closed_on_size = 0
    for flags in range(8):
        plan, ref, _ = check(comp, indexes, used, flags, max_payload=300000)
        for a, t in zip(ref["bundle_action"], ref["bundle_total"]):
            seen["action"].add((a, t != 0) if a == gc_ref.REMOVE else a)
        for x in ref["indexes"]:
            for f in ("modified", "necessary", "unlink"):
                seen[f].add(bool(x[f]))
        per_index = np.bincount(ref["new_bundle_index"], minlength=5) if ref["new_bundle_index"] else np.zeros(5)
        closed_on_size += int((per_index > 1).sum())
    # gc_ref says every case occurs in this input: a change of seed cannot empty one silently
    assert seen["action"] == {gc_ref.KEEP, (gc_ref.REMOVE, True), (gc_ref.REMOVE, False), gc_ref.REPACK_BUNDLE,
                              gc_ref.DROP_RECORD}
    assert seen["modified"] == seen["necessary"] == seen["unlink"] == {True, False}
    assert closed_on_size >= 8  # several new bundles closed on size, not at an index file's end


@pytest.mark.parametrize("deep", [False, True])
def test_a_million_records(comp, big_case, deep):
    """2^20 records, 2^19 used ids: many workgroups contend on the table."""
    from zbackup_amd import Collector
    ids, sizes, bundle_first, bundle_ids, index_first, used, indexes, used_list = big_case
    flags = gc_ref.DEEP if deep else 0
    ref = gc_ref.plan(indexes, used_list, flags, 1 << 21)
    col = Collector(ctx=comp._ctx)
    col.mark_ids(used)
    plan = col.plan_arrays(ids, sizes, bundle_first, bundle_ids, index_first, deep=deep, max_payload=1 << 21)
    assert_equal(plan, ref)
    st = col.last_stats()
    assert st["table_slots"] == 1 << 21 and 1 < st["max_probe"] < 200
    assert len(ref["copy"]) > 100000 and len(ref["new_bundle_size"]) > 1000


@pytest.fixture(scope="module")
def big_case():
    rng = np.random.default_rng(99)
    N, U, P = 1 << 20, 1 << 19, 700000
    pool = rng.integers(0, 256, (P, 24), dtype=np.uint8)
    pool_size = rng.integers(1, 65537, P).astype(np.uint32)
    draw = rng.integers(0, P, N)
    ids, sizes = pool[draw], pool_size[draw]
    lens = rng.integers(0, 65, N // 24)
    bundle_first = np.concatenate([[0], np.minimum(np.cumsum(lens), N)])
    bundle_first = np.concatenate([bundle_first[bundle_first < N], [N]]).astype(np.uint64)
    B = len(bundle_first) - 1
    bundle_ids = rng.integers(0, 256, (B, 24), dtype=np.uint8)
    index_first = np.array([0, B // 4, B // 2, B // 2, B], dtype=np.uint64)  # one index file without bundles
    used = np.concatenate([pool[rng.integers(0, P, U * 3 // 4)], rng.integers(0, 256, (U // 4, 24), dtype=np.uint8)])
    blob = ids.tobytes()
    id_list = [blob[24 * k:24 * k + 24] for k in range(N)]
    size_list = sizes.tolist()
    bf = bundle_first.tolist()
    bundles = [(bundle_ids[b].tobytes(), list(zip(id_list[bf[b]:bf[b + 1]], size_list[bf[b]:bf[b + 1]])))
               for b in range(B)]
    xf = index_first.tolist()
    indexes = [bundles[xf[i]:xf[i + 1]] for i in range(4)]
    ublob = used.tobytes()
    used_list = [ublob[24 * k:24 * k + 24] for k in range(len(used))]
    return ids, sizes, bundle_first, bundle_ids, index_first, used, indexes, used_list


def test_errors_found_on_the_device_and_after(comp):
    from zbackup_amd import ZcError
    rng = np.random.default_rng(8)
    pool = random_ids(rng, 300)
    size_of = {c: int(rng.integers(1, 5000)) for c in pool}
    indexes = random_indexes(rng, 900, pool, size_of)
    used = pool[::2]
    check(comp, indexes, used)
    # the same id with another size, far from its first registration
    first_id, first_size = next(r[0] for _, r in indexes[0] if r)
    bad = [indexes[0], indexes[1] + [(random_ids(rng, 1)[0], [(pool[0], size_of[pool[0]]), (first_id, first_size + 1)])]]
    with pytest.raises(gc_ref.SizeMismatch):
        gc_ref.plan(bad, used)
    with pytest.raises(ZcError, match="same chunk id and different sizes"):
        collector(comp, used).plan(bad)
    # a copy list that does not fit: the error names the count needed, which then works
    ref = gc_ref.plan(indexes, used, gc_ref.REPACK)
    need = len(ref["copy"])
    assert need > 10
    flat = collector(comp, used).plan(indexes, repack=True)
    col = collector(comp, used)
    with pytest.raises(ZcError, match=f"{need} copy entries in {len(ref['new_bundle_size'])} new bundles"):
        col.plan_arrays(flat.ids, flat.sizes, flat.bundle_first, flat.bundle_ids, flat.index_first, repack=True,
                        copy_cap=need - 1)
    assert_equal(col.plan_arrays(flat.ids, flat.sizes, flat.bundle_first, flat.bundle_ids, flat.index_first,
                                 repack=True, copy_cap=need), ref)


def test_collect_end_to_end(torch_cuda, comp):
    """Two backups that share half their bytes are chunked, bundled and
    compressed on the GPU; backup 2 is forgotten; the plan's REPACK bundles are
    decoded by liblzo2 (the reference's decoder), repacked on the GPU and
    compressed; backup 1 then restores byte for byte from the kept and the new
    bundles alone."""
    if lzo_oracle.lzo_lib() is None:
        pytest.skip("liblzo2 not in this image")
    from zbackup_amd import ZC_CHUNK_NEW, BackupCreator, Collector, Restorer, Sha256
    from zbackup_amd.bundle import lzo_capacity, plan_bundles
    torch = torch_cuda
    W, MAXP = 4096, 128 << 10
    common = [payload("text" if k % 2 else "random", 50 * W, 30 + k) for k in range(8)]
    own2 = [payload("runs" if k % 2 else "random", 100 * W + W // 2, 40 + k) for k in range(8)]
    # backup 2 (made first): its own pieces between the shared ones; backup 1: the shared bytes in one run
    data2 = np.concatenate([x for pair in zip(common, own2) for x in pair] + [payload("random", 13, 50)])
    data1 = np.concatenate([payload("text", 1 << 20, 51)] + common + [payload("random", (1 << 20) + 80, 52)])
    n2 = (len(data2) + 15) & ~15
    both = np.concatenate([data2, np.zeros(n2 - len(data2), np.uint8), data1])
    d = torch.from_numpy(both).cuda()
    stored, backup_data, seen = [], [], set()  # stored: (offset in `both`, size, id), in Writer::add's order
    with BackupCreator(chunk_max_size=W, sha1=True) as bc:
        for base, n in ((0, len(data2)), (n2, len(data1))):
            bc.chunk_device(d.data_ptr() + base, n)
            recs = bc.records()
            backup_data.append(bc.get_backup_data())
            for r in recs[recs["kind"] == ZC_CHUNK_NEW]:
                cid = bytes(r["sha1"]) + int(r["rolling"]).to_bytes(8, "little")
                if cid not in seen:
                    seen.add(cid)
                    stored.append((base + int(r["offset"]), int(r["size"]), cid))
    offs, sizes, ids = (list(v) for v in zip(*stored))
    bundle_of, nb = plan_bundles(sizes, MAXP)
    assert nb > 30
    d_payload = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    comp.gather(d.data_ptr(), offs, sizes, d_payload.data_ptr())
    pay_size = np.bincount(bundle_of, weights=sizes, minlength=nb).astype(np.uint64)
    pay_off = np.concatenate([[0], np.cumsum(pay_size)[:-1]]).astype(np.uint64)
    z_off = np.concatenate([[0], np.cumsum([lzo_capacity(int(s)) for s in pay_size])]).astype(np.uint64)
    d_z = torch.empty(int(z_off[-1]), dtype=torch.uint8, device="cuda")
    z_size = comp.compress(d_payload.data_ptr(), pay_off, pay_size, d_z.data_ptr(), z_off[:-1])
    z = d_z.cpu().numpy()
    framed = [z[int(z_off[k]):int(z_off[k]) + int(z_size[k])].tobytes() for k in range(nb)]
    members = [np.nonzero(bundle_of == k)[0] for k in range(nb)]
    infos = [[(ids[i], sizes[i]) for i in members[k]] for k in range(nb)]
    names = [hashlib.sha1(b"bundle %d" % k).digest() + bytes(4) for k in range(nb)]
    cut = nb * 2 // 3  # two index files
    indexes = [[(names[k], infos[k]) for k in range(cut)], [(names[k], infos[k]) for k in range(cut, nb)]]

    # forget backup 2
    with Collector(ctx=comp._ctx) as col:
        col.mark(backup_data[1])
        plan = col.plan(indexes, max_payload=MAXP)
        ref = gc_ref.plan(indexes, [bytes(u) for u in col.used_ids()], 0, MAXP)
        assert_equal(plan, ref)
        act = plan.bundle_action
        repack = np.nonzero(act == gc_ref.REPACK_BUNDLE)[0]
        assert len(repack) >= 4 and (act == gc_ref.REMOVE).sum() >= 4 and (act == gc_ref.KEEP).sum() >= 4
        # the REPACK bundles decoded as the reference decodes them, one upload
        work_off, pos = {}, 0
        for b in repack:
            work_off[int(b)] = pos
            pos += (int(pay_size[b]) + 15) & ~15
        work = np.zeros(pos, dtype=np.uint8)
        for b in repack:
            p = lzo_oracle.unframe(framed[b])
            assert len(p) == int(pay_size[b])
            work[work_off[int(b)]:work_off[int(b)] + len(p)] = np.frombuffer(p, dtype=np.uint8)
        d_work = torch.from_numpy(work).cuda()
        total_new = int(plan.new_bundle_size.sum())
        d_new = torch.full((total_new + 32,), CANARY, dtype=torch.uint8, device="cuda")
        new_infos, new_off, new_size = col.repack(plan, d_work.data_ptr(), work_off, d_new.data_ptr() + 16)
    got_new = d_new.cpu().numpy()
    assert (got_new[:16] == CANARY).all() and (got_new[16 + total_new:] == CANARY).all()
    # each new payload: the bytes gc_ref's copy list predicts (records number the stored chunks)
    assert len(new_infos) == len(ref["new_bundle_size"]) >= 2
    for j in range(len(new_infos)):
        recs = [r for r, cb in zip(ref["copy"], ref["copy_bundle"]) if cb == j]
        want = np.concatenate([both[offs[r]:offs[r] + sizes[r]] for r in recs])
        at = 16 + int(new_off[j])
        assert int(new_size[j]) == len(want) == ref["new_bundle_size"][j]
        assert np.array_equal(got_new[at:at + len(want)], want), f"new bundle {j}"
        assert new_infos[j] == [(ids[r], sizes[r]) for r in recs]
    # the payload bytes saved: what gc_ref says is dropped
    flags = np.array(ref["record_flags"])
    gone = np.isin(bundle_of, np.nonzero(act != gc_ref.KEEP)[0]) & ((flags & gc_ref.COPIED) == 0)
    dropped = int(np.array(sizes)[gone].sum())
    kept = np.nonzero(act == gc_ref.KEEP)[0]
    assert dropped > 1 << 20
    assert int(pay_size.sum()) - (int(pay_size[kept].sum()) + total_new) == dropped
    # the new bundles compressed; backup 1 restored from the kept and the new bundles alone
    nz_off = np.concatenate([[0], np.cumsum([lzo_capacity(int(s)) for s in new_size])]).astype(np.uint64)
    d_nz = torch.empty(int(nz_off[-1]), dtype=torch.uint8, device="cuda")
    nz_size = comp.compress(d_new.data_ptr() + 16, new_off, new_size, d_nz.data_ptr(), nz_off[:-1])
    nz = d_nz.cpu().numpy()
    repo_framed = [framed[k] for k in kept] + [nz[int(nz_off[j]):int(nz_off[j]) + int(nz_size[j])].tobytes()
                                                for j in range(len(new_infos))]
    repo_infos = [infos[k] for k in kept] + new_infos
    rplan = Restorer.plan(backup_data[1], repo_infos)
    assert rplan.length == len(data1)
    payloads = [lzo_oracle.unframe(repo_framed[b]) for b in rplan.used]
    d_rwork = torch.from_numpy(rplan.host_image(payloads)).cuda()
    d_out = torch.full((len(data1) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    with Restorer(ctx=comp._ctx) as rs:
        n = rs.replay(rplan, d_rwork.data_ptr(), d_out.data_ptr() + 16, len(data1))
    out = d_out.cpu().numpy()
    assert n == len(data1) and np.array_equal(out[16:16 + n], data1)
    assert (out[:16] == CANARY).all() and (out[16 + n:] == CANARY).all()
    h = Sha256()
    h.add(out[16:16 + n])
    assert h.finish() == hashlib.sha256(data1.tobytes()).digest()
    # backup 2 no longer restores: its own chunks are gone
    from zbackup_amd import ZcError
    with pytest.raises(ZcError, match="is in none of"):
        Restorer.plan(backup_data[0], repo_infos)
