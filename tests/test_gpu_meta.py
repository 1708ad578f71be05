"""GPU tests of repository adoption: zc_chunk_meta_compute (zc_meta.hip) computes
every chunk's metadata record and full ChunkId from bundle payloads -- chunks
back to back at arbitrary byte offsets -- and compares the ids with the ones the
bundles claim.

Every field of every record is compared with tests/meta_ref.py (hashlib's
SHA-1, integers mod 2^64), and with the engine's own export for chunks a
context cut itself: zc_export_chunk_meta is the existing definition."""
import ctypes
import struct

import numpy as np
import pytest

from oracle import oracle
from tests import meta_ref

pytestmark = pytest.mark.gpu

W = 4096
SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 1023, 1024, 1025, 4095, 4096]
NO = meta_ref.NO_ANCHOR
STREAM_SPEC = "R1:2000000,Z:300000,C77:200000,R2:600000"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    return torch


@pytest.fixture(scope="module")
def adopter(torch_cuda):
    from zbackup_amd import Adopter
    with Adopter(W) as a:
        yield a


def place(chunks, residues, lead=0):
    """One payload holding chunks[i] at the next offset that is residues[i] mod 16
    (the gaps hold 0xA5, so a byte read from outside a chunk shows): (payload, off, size)."""
    buf, off = bytearray(b"\xa5" * lead), []
    for c, r in zip(chunks, residues):
        while len(buf) % 16 != r:
            buf.append(0xA5)
        off.append(len(buf))
        buf += c
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array(off, dtype=np.uint64), \
        np.array([len(c) for c in chunks], dtype=np.uint32)


def on_device(torch, payload):
    """A device tensor of exactly the payload's bytes."""
    t = torch.from_numpy(np.ascontiguousarray(payload)).to("cuda")
    assert t.numel() == payload.size
    return t


def expect_of(rec):
    from zbackup_amd.chunker import SEED_DTYPE
    e = np.zeros(len(rec), dtype=SEED_DTYPE)
    e["sha1"], e["rolling"], e["size"] = rec["sha1"], rec["rolling"], rec["size"]
    return e


def assert_records(got, want):
    assert got.dtype == want.dtype and len(got) == len(want)
    for name in want.dtype.names:
        differ = np.nonzero((got[name] != want[name]).reshape(len(want), -1).any(axis=1))[0]
        assert not len(differ), (name, differ[:8].tolist(), got[name][differ[:4]], want[name][differ[:4]])
    assert got.tobytes() == want.tobytes()


def anchored(n, positions):
    b = bytearray(n)
    for q in positions:
        b[q - 14] = 0xFF
    return bytes(b)


@pytest.mark.parametrize("kind", ["random", "zero", "ff"])
def test_every_size_at_every_start_residue(torch_cuda, adopter, kind):
    rng = np.random.default_rng(11)
    chunks, residues = [], []
    for n in SIZES:
        for r in range(16):
            chunks.append({"random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zero": bytes(n),
                           "ff": b"\xff" * n}[kind])
            residues.append(r)
    payload, off, size = place(chunks, residues)
    assert sorted(set((off % 16).tolist())) == list(range(16))
    want = meta_ref.records(chunks, W)
    t = on_device(torch_cuda, payload)
    got, status = adopter.chunk_meta(t.data_ptr(), payload.size, off, size)
    assert_records(got, want)
    assert not status.any() and adopter.n_bad == 0
    if kind == "random":  # 1 position in 256: the 16 full-size chunks all but surely hold an anchor
        assert (got["anchor"][-16:] != NO).all() and (got["anchor"][:-16] == NO).all()
    else:
        assert (got["anchor"] == NO).all()  # a run of one byte never holds an anchor


def test_anchor_positions(torch_cuda, adopter):
    chunks, residues, answers = [], [], []
    for q in (62, 63, 64, 1023, 1024, 1025, 1039, 1040, 4094, 4095):
        c = anchored(W, [q])
        hits = [p for p in range(30, W) if meta_ref.is_anchor(c, p, W)]
        assert hits == [q] and meta_ref.st(c, q) == 0x7F80  # the only one
        for r in (0, 1, 7, 15):
            chunks.append(c)
            residues.append(r)
            answers.append(NO if q < 63 else q)
    extra = [(anchored(W, [62, 700]), 700), (anchored(W, [100, 101]), 100), (anchored(W - 1, [500]), NO)]
    for c, a in extra:
        for r in (0, 1, 7, 15):
            chunks.append(c)
            residues.append(r)
            answers.append(a)
    payload, off, size = place(chunks, residues, lead=3)
    want = meta_ref.records(chunks, W)
    assert want["anchor"].tolist() == answers
    t = on_device(torch_cuda, payload)
    got, _ = adopter.chunk_meta(t.data_ptr(), payload.size, off, size)
    assert_records(got, want)
    hit = got[got["anchor"] != NO]
    assert (hit["gear"] >> 16 == 0x7F80).all() and (hit["gear"][:-4] & 0xFFFF == 0).all()


def test_chunk_size_65536(torch_cuda):
    from zbackup_amd import Adopter
    W64 = 65536
    assert meta_ref.anchor_lo(W64) == 0x7FF0
    rng = np.random.default_rng(12)

    def crafted(q):
        # 0xFF at q - 14 gives 0x7F80, 7 at q - 8 adds 0x70: st(q) = 0x7FF0, the threshold itself
        b = bytearray(W64)
        b[q - 14], b[q - 8] = 0xFF, 7
        assert meta_ref.st(b, q) == 0x7FF0 and meta_ref.first_anchor(bytes(b), W64)[0] == q
        assert sum(meta_ref.is_anchor(b, p, W64) for p in range(max(30, q - 40), min(W64, q + 41))) == 1
        return bytes(b)

    chunks = [rng.integers(0, 256, W64, dtype=np.uint8).tobytes() for _ in range(5)]
    chunks += [bytes(W64), crafted(63), crafted(65535)]
    buf, off = bytearray(), []
    for c in chunks:
        buf += b"\xa5" * (1 if len(buf) % 2 == 0 else 2)  # every chunk starts at an odd offset
        off.append(len(buf))
        buf += c
    assert all(o % 2 == 1 for o in off) and len(set(o % 16 for o in off)) > 1
    payload = np.frombuffer(bytes(buf), dtype=np.uint8)
    want = meta_ref.records(chunks, W64)
    assert want["anchor"][5:].tolist() == [NO, 63, 65535]
    t = on_device(torch_cuda, payload)
    with Adopter(W64) as a:
        got, _ = a.chunk_meta(t.data_ptr(), payload.size, off, [W64] * 8)
        assert_records(got, want)
        # the same bytes under W = 4096: no chunk is W bytes, so none carries an anchor
    with Adopter(W) as a:
        small, _ = a.chunk_meta(t.data_ptr(), payload.size, off, [W64] * 8)
    assert (small["anchor"] == NO).all() and (small["rolling"] == want["rolling"]).all()
    assert (small["sha1"] == want["sha1"]).all() and (small["anchor_def"] == meta_ref.anchor_def(W)).all()


@pytest.mark.parametrize("Wc", [63, 64])
def test_chunk_sizes_with_no_or_one_anchor_position(torch_cuda, Wc):
    from zbackup_amd import Adopter
    rng = np.random.default_rng(Wc)
    chunks = [rng.integers(0, 256, Wc, dtype=np.uint8).tobytes() for _ in range(200)]
    chunks += [bytes(Wc), rng.integers(0, 256, Wc - 1, dtype=np.uint8).tobytes(),
               rng.integers(0, 256, Wc + 1, dtype=np.uint8).tobytes()]
    payload, off, size = place(chunks, [i % 16 for i in range(len(chunks))], lead=1)
    want = meta_ref.records(chunks, Wc)
    if Wc == 63:
        assert (want["anchor"] == NO).all()
    else:
        assert set(want["anchor"].tolist()) == {63, NO}  # 1 in 16 of 200 random chunks
    t = on_device(torch_cuda, payload)
    with Adopter(Wc) as a:
        got, _ = a.chunk_meta(t.data_ptr(), payload.size, off, size)
    assert_records(got, want)


def _edited(base, seed, every=150_001):
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < base.size:
        out.append(base[pos:pos + every])
        out.append(rng.integers(0, 256, int(rng.integers(1, 101)), dtype=np.uint8))
        pos += every
    return np.concatenate(out)


@pytest.fixture(scope="module")
def backup(torch_cuda):
    """A 3 MiB stream's first backup: the stream, its NEW chunks' records, the
    engine's exported metadata, and the chunks packed as bundles."""
    from zbackup_amd import BackupCreator, chunk_id_blob
    from zbackup_amd.bundle import plan_bundles
    data = oracle.gen(STREAM_SPEC)
    t = torch_cuda.from_numpy(np.ascontiguousarray(data)).to("cuda")
    with BackupCreator(W, sha1=True) as bc:
        bc.chunk_device(t.data_ptr(), data.size)
        recs = bc.records()
        exported = bc.export_chunk_meta()
    new = recs[recs["kind"] == 0]
    assert len(exported) > 500
    bundle_of, nb = plan_bundles(new["size"])
    assert nb >= 2
    bundles, payloads = [[] for _ in range(nb)], [bytearray() for _ in range(nb)]
    for r, b in zip(new, bundle_of):
        bundles[b].append((chunk_id_blob(bytes(r["sha1"]), int(r["rolling"])), int(r["size"])))
        payloads[b] += data[int(r["offset"]):int(r["offset"]) + int(r["size"])].tobytes()
    return data, new, exported, bundles, [bytes(p) for p in payloads]


def test_against_the_engines_own_export(torch_cuda, adopter, backup):
    data, new, exported, bundles, payloads = backup
    image = np.frombuffer(b"\xa5" * 5 + b"".join(payloads), dtype=np.uint8)  # back to back from offset 5
    size = new["size"].astype(np.uint32)
    off = 5 + np.concatenate([[0], np.cumsum(size.astype(np.uint64))[:-1]]).astype(np.uint64)
    t = on_device(torch_cuda, image)
    got, status = adopter.chunk_meta(t.data_ptr(), image.size, off, size, expect=expect_of(new))
    assert not status.any() and adopter.n_bad == 0
    assert (got["sha1"] == new["sha1"]).all() and (got["rolling"] == new["rolling"]).all()
    full = got[got["size"] == W]
    assert full.tobytes() == exported.tobytes()  # byte for byte, in the same order
    assert (got["anchor"][got["size"] != W] == NO).all()
    rep = adopter.adopt(bundles, payloads)
    assert rep.meta.tobytes() == exported.tobytes() and rep.bad == []
    assert rep.chunks == len(new) and rep.bytes == int(size.sum())


def test_adopted_metadata_seeds_the_anchor_path(torch_cuda, adopter, backup):
    from zbackup_amd import BackupCreator
    data, new, exported, bundles, payloads = backup
    adopted = adopter.adopt(bundles, payloads).meta
    edited = _edited(data, 77)
    seeds = [(bytes(r["sha1"]), int(r["rolling"]), int(r["size"])) for r in new]
    want = oracle.chunk(edited, W, seeds=seeds)
    assert sum(1 for r in want if r[0] == "D") > 0.5 * len(exported)
    t = torch_cuda.from_numpy(np.ascontiguousarray(edited)).to("cuda")
    runs = []
    for meta in (adopted, exported):
        with BackupCreator(W, sha1=True) as bc:
            bc.seed_index_meta(new["sha1"], new["rolling"], new["size"], meta)
            st0 = bc.stats()
            bc.chunk_device(t.data_ptr(), edited.size)
            runs.append((bc.record_tuples(), st0["hist_seeded"], st0["by_value"]))
    assert runs[0][0] == want
    assert runs[0] == runs[1]
    assert runs[0][1] == int((exported["anchor"] != NO).sum()) > 0


def test_scrub_reports_exactly_the_damaged_chunks(torch_cuda, adopter, backup):
    data, new, exported, bundles, payloads = backup
    size = new["size"].astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(size.astype(np.uint64))]).astype(np.int64)
    image = np.frombuffer(b"".join(payloads), dtype=np.uint8).copy()
    expect = expect_of(new)
    n = len(new)
    first, middle, last = 3, n // 2, n - 1
    image[start[first]] ^= 0x01                                # the first byte of a chunk
    image[start[middle] + int(size[middle]) // 2] ^= 0x10      # a middle byte
    image[start[last + 1] - 1] ^= 0x80                         # the last byte of the last chunk
    wrong_size, wrong_rolling = 10, 20
    expect["size"][wrong_size] += 1
    expect["rolling"][wrong_rolling] ^= np.uint64(1 << 40)
    want = np.zeros(n, dtype=np.uint8)
    want[[first, middle, last]] = meta_ref.BAD_SHA1 | meta_ref.BAD_ROLLING
    want[wrong_size], want[wrong_rolling] = meta_ref.BAD_SIZE, meta_ref.BAD_ROLLING
    t = on_device(torch_cuda, image)
    got, status = adopter.chunk_meta(t.data_ptr(), image.size, start[:-1].astype(np.uint64), size, expect=expect)
    assert status.tolist() == want.tolist() and adopter.n_bad == 5
    # the record carries the computed id, never the expected one
    k = int(start[first])
    assert_records(got[first:first + 1], meta_ref.record(image[k:k + int(size[first])].tobytes(), W))
    assert got["rolling"][wrong_rolling] == new["rolling"][wrong_rolling]
    # adopt(): the same damage through the bundle form
    sizes_b = [sum(s for _, s in b) for b in bundles]
    cuts = np.concatenate([[0], np.cumsum(sizes_b)])
    damaged = [image[cuts[b]:cuts[b + 1]].tobytes() for b in range(len(bundles))]
    rep = adopter.adopt(bundles, damaged)
    where = []
    for i in (first, middle, last):
        b = max(bb for bb in range(len(bundles)) if sum(len(x) for x in bundles[:bb]) <= i)
        where.append((b, i - sum(len(x) for x in bundles[:b]), 3))
    assert rep.bad == where and adopter.n_bad == 3
    keep = np.ones(n, bool)
    keep[[first, middle, last]] = False
    assert rep.meta.tobytes() == got[keep & (size == W)].tobytes()
    assert len(rep.meta) == len(exported) - int((size[[first, middle, last]] == W).sum())


def test_overlapping_unordered_extents_and_the_payloads_last_byte(torch_cuda, adopter):
    rng = np.random.default_rng(13)
    payload = rng.integers(0, 256, 3 * W + 77, dtype=np.uint8)
    n = payload.size
    ext = [(n - W, W), (0, W), (1, W), (W // 2, W), (n - 1, 1), (0, n), (n - 17, 17), (2 * W + 60, 17), (0, 1),
           (n - W, W)]
    off = np.array([o for o, _ in ext], dtype=np.uint64)
    size = np.array([s for _, s in ext], dtype=np.uint32)
    want = meta_ref.records([payload[o:o + s].tobytes() for o, s in ext], W)
    t = on_device(torch_cuda, payload)  # exactly n bytes: the last chunk ends at the tensor's end
    got, _ = adopter.chunk_meta(t.data_ptr(), n, off, size)
    assert_records(got, want)
    again, _ = adopter.chunk_meta(t.data_ptr(), n, off, size)  # two calls on one context agree
    assert again.tobytes() == got.tobytes()
    host, _ = adopter.chunk_meta_host(payload, off, size)       # host and device forms agree
    assert host.tobytes() == got.tobytes()
    # a payload that starts at an odd device address: the same chunks, seen from 3 bytes in
    inner = [(o - 3, s) for o, s in ext if o >= 3]
    got3, _ = adopter.chunk_meta(t.data_ptr() + 3, n - 3, [o for o, _ in inner], [s for _, s in inner])
    assert_records(got3, want[[i for i, (o, _) in enumerate(ext) if o >= 3]])
    # expected ids, no status array: n_bad alone reports
    bad = ctypes.c_size_t(99)
    e = expect_of(want)
    e["rolling"][2] ^= np.uint64(1)
    out = np.zeros(len(ext), dtype=meta_ref.META_DTYPE)
    L = adopter._L
    rc = L.zc_chunk_meta_compute(adopter._ctx, ctypes.c_void_p(t.data_ptr()), n, off.ctypes.data, size.ctypes.data,
                                 len(ext), e.ctypes.data, out.ctypes.data, None, ctypes.byref(bad))
    assert rc == 0 and bad.value == 1 and out.tobytes() == got.tobytes()
    st = adopter.last_stats()
    assert st["meta_ms"] > 0 and st["sha1_ms"] > 0 and st["total_ms"] >= st["meta_ms"] + st["sha1_ms"]


def test_no_chunks_and_argument_errors(torch_cuda, adopter):
    from zbackup_amd import ZcError
    payload = np.arange(100, dtype=np.uint8)
    t = on_device(torch_cuda, payload)
    got, status = adopter.chunk_meta(t.data_ptr(), 100, [], [])
    assert len(got) == 0 and len(status) == 0 and adopter.n_bad == 0
    assert adopter._L.zc_chunk_meta_compute(adopter._ctx, None, 0, None, None, 0, None, None, None, None) == 0
    rep = adopter.adopt([], [])
    assert rep.chunks == 0 and rep.bad == [] and len(rep.meta) == 0
    L, ctx = adopter._L, adopter._ctx
    off, size = np.array([0, 10], dtype=np.uint64), np.array([10, 20], dtype=np.uint32)
    out, st = np.zeros(2, dtype=meta_ref.META_DTYPE), np.zeros(2, dtype=np.uint8)
    e = np.zeros(64, dtype=np.uint8)
    p = ctypes.c_void_p(t.data_ptr())
    cases = [
        ((None, 100, off.ctypes.data, size.ctypes.data, 2, None, out.ctypes.data, st.ctypes.data, None), "null payload"),
        ((p, 100, None, size.ctypes.data, 2, None, out.ctypes.data, st.ctypes.data, None), "null payload, off"),
        ((p, 100, off.ctypes.data, None, 2, None, out.ctypes.data, st.ctypes.data, None), "null payload, off, size"),
        ((p, 100, off.ctypes.data, size.ctypes.data, 2, None, None, st.ctypes.data, None), "or out with n > 0"),
        ((p, 100, off.ctypes.data, size.ctypes.data, 2, e.ctypes.data, out.ctypes.data, None, None),
         "expected ids given, but neither status nor n_bad"),
        ((p, 29, off.ctypes.data, size.ctypes.data, 2, None, out.ctypes.data, st.ctypes.data, None),
         "chunk 1 [10, +20) ends past the payload's 29 bytes"),
    ]
    for fn in ("zc_chunk_meta_compute", "zc_chunk_meta_compute_host"):
        for args, text in cases:
            a = list(args)
            if fn.endswith("_host") and a[0] is not None:
                a[0] = ctypes.c_void_p(payload.ctypes.data)
            assert getattr(L, fn)(ctx, *a) == -1
            msg = L.zc_last_error(ctx).decode()
            assert msg.startswith(fn + ": ") and text in msg, msg
    size[0] = 0
    assert L.zc_chunk_meta_compute(ctx, p, 100, off.ctypes.data, size.ctypes.data, 2, None, out.ctypes.data,
                                   st.ctypes.data, None) == -1
    assert L.zc_last_error(ctx).decode() == "zc_chunk_meta_compute: size[0] is 0"
    with pytest.raises(ZcError, match="bundle 0 decoded to 5 bytes, its chunks take 6"):
        adopter.adopt([[(bytes(16) + struct.pack("<Q", 1), 6)]], [bytes(5)])
    # the context still works after the refusals
    got, _ = adopter.chunk_meta(t.data_ptr(), 100, [0, 10], [10, 90])
    assert_records(got, meta_ref.records([payload[:10].tobytes(), payload[10:].tobytes()], W))
