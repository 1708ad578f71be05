"""TEST INFRASTRUCTURE: the stream of test_restore_end_to_end (tests/test_gpu_unlzo.py)
-- W = 4,096, 22 MiB of text, random bytes, repeats, zeros and runs -- chunked on
the GPU and cut into bundles by Writer::add's rule, for the random-access
restore's tests."""
import numpy as np

from tests.lzo_inputs import payload

W = 4096


def mixed_stream():
    a, b = payload("text", 6 << 20, 11), payload("random", 5 << 20, 12)
    return np.concatenate([a, b, a[3:3 << 20], np.zeros(2 << 20, np.uint8), b[:2 << 20], payload("runs", 4 << 20, 13),
                           a[:2 * W], payload("random", 77, 14)])  # two whole chunks again, then a short tail


def chunk_and_bundle(d, n):
    """The n-byte stream at device tensor d -> (backup data, per stored chunk
    its id blob, offset and size, its bundle, the number of bundles)."""
    from zbackup_amd import ZC_BYTES, ZC_CHUNK_NEW, BackupCreator
    from zbackup_amd.bundle import plan_bundles
    with BackupCreator(chunk_max_size=W, sha1=True) as bc:
        bc.chunk_device(d.data_ptr(), n)
        recs = bc.records()
        backup_data = bc.get_backup_data()
    kinds = recs["kind"]
    assert (kinds == ZC_BYTES).sum() >= 1 and int(recs["size"].sum()) == n
    # Writer::add: the saved chunks whose id the index does not hold yet
    seen, offs, sizes, ids = set(), [], [], []
    for r in recs[kinds == ZC_CHUNK_NEW]:
        cid = bytes(r["sha1"]) + int(r["rolling"]).to_bytes(8, "little")
        if cid not in seen:
            seen.add(cid)
            offs.append(int(r["offset"]))
            sizes.append(int(r["size"]))
            ids.append(cid)
    bundle_of, nb = plan_bundles(sizes)
    assert nb > 4
    return backup_data, ids, offs, sizes, bundle_of, nb


def random_reads(rng, total, count, max_size):
    reads = []
    for _ in range(count):
        n = int(rng.integers(0, max_size + 1))
        reads.append((int(rng.integers(0, total - n + 1)), n))
    return reads
