"""Every device-form entry point called straight after work queued on the
default stream, with no synchronisation in between (tests/stream_order.py has
the staging): the input buffer holds a stale input A while the fresh input B is
still on its way behind tens of milliseconds of queued fills, and every caller
output buffer has a fill with 0xEE queued over it.  A call that does not order
its stream after the default stream reads A, or has its output overwritten.

The expected values are the references the other tests of each call use, for B.
Each case prints the queued work's time and the idle call's time."""
import lzma
import random
import zlib

import numpy as np
import pytest

from oracle import lzo_oracle, oracle
from tests import aes_ref, meta_ref
from tests import index_ref as IR
from tests import stream_order as S
from tests import xz_inputs as XI
from tests import xz_ref as XR
from tests import xzenc_ref as E
from tests.lzo_inputs import payload as lzo_payload

pytestmark = pytest.mark.gpu

CANARY = S.CANARY
KEY = bytes(range(0x40, 0x50))
RND = bytes(range(0xA0, 0xB0))
W = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    S.require_default_stream(torch)
    return torch


@pytest.fixture(scope="module")
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


def dev(torch, a):
    a = a if isinstance(a, np.ndarray) else np.frombuffer(bytes(a), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def buffers(torch, stale, fresh):
    """(d_in, d_stale, d_fresh) of two host images of one size."""
    assert len(stale) == len(fresh) and bytes(stale) != bytes(fresh)
    d_stale, d_fresh = dev(torch, stale), dev(torch, fresh)
    return torch.empty_like(d_fresh), d_stale, d_fresh


def canaries(torch, n):
    return torch.full((n,), CANARY, dtype=torch.uint8, device="cuda")


def image(total, pieces):
    """The expected output buffer: canaries with `pieces` = [(offset, bytes)] on top."""
    want = np.full(total, CANARY, dtype=np.uint8)
    for o, b in pieces:
        want[int(o):int(o) + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return want


def same(d_out, want, what):
    got = d_out.cpu().numpy()
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        kind = "a canary" if got[at] == CANARY else "not the expected byte"
        pytest.fail(f"{what}: first wrong byte at {at} of {len(want)} ({kind}: {got[at]:#x}, expected {want[at]:#x})")


# ---- the staging tests itself ----

def test_control_an_unordered_copy_sees_the_stale_input(torch_cuda):
    """In place of a mutant build: the same staging, a raw copy on a fresh
    stream.  With no wait it sees A while the queued work still runs; after
    wait_stream(default) it sees B."""
    c = S.control(torch_cuda)
    assert c["inputs_differ"]
    assert c["running_before"], "the queued work had ended before the unordered copy was issued"
    assert c["unordered_sees_stale"] and not c["unordered_sees_fresh"], \
        "a copy that does not wait saw the fresh input: this staging cannot tell a missing wait"
    assert c["ordered_sees_fresh"]
    assert c["queued_ms"] >= S.MIN_MS


# ---- the chunker ----

def test_chunk_device(torch_cuda):
    """1 MiB at W = 4096 behind a busy default stream: zc_chunk_device's
    hipStreamQuery finds it busy and takes the event branch."""
    from zbackup_amd import BackupCreator
    torch = torch_cuda
    n = 1 << 20
    a = oracle.gen(f"R41:{n}")
    b = oracle.gen(f"R42:500000,C1000:300000,Z:100000,R43:{n - 900000}")
    assert len(a) == len(b) == n
    want = oracle.chunk(b, W)
    assert want != oracle.chunk(a, W)
    d_in, d_a, d_b = buffers(torch, a, b)
    ran = []
    with BackupCreator(W, sha1=True) as bc:
        def call():
            if ran:
                bc.reset()
                bc.forget_stream_chunks()  # every call sees the index a first stream sees
            ran.append(1)
            bc.chunk_device(d_in.data_ptr(), n)
            return bc.record_tuples()
        got, idle = S.staged_call(torch, "chunk_device", call, [(d_in, d_a, d_b)])
    assert idle == want
    assert got == want, f"{len(got)} records, the oracle gives {len(want)} (the stale stream gives " \
                        f"{len(oracle.chunk(a, W))})"


# ---- payload assembly, checksums, lzo ----

EXT_OFF = [1, 4099, 70001, 200000, 333333, 600001, 900000, 1048000]
EXT_SIZE = [4096, 1, 65537, 0, 100003, 4095, 33, 576]


def test_gather(torch_cuda, comp):
    torch = torch_cuda
    a, b = rand(51, 1 << 20), rand(52, 1 << 20)
    d_in, d_a, d_b = buffers(torch, a, b)
    total = sum(EXT_SIZE)
    d_out = canaries(torch, total + 128)
    S.staged_call(torch, "gather", lambda: comp.gather(d_in.data_ptr(), EXT_OFF, EXT_SIZE, d_out.data_ptr() + 64),
                  [(d_in, d_a, d_b)], [d_out])
    same(d_out, image(total + 128, [(64, np.concatenate([b[o:o + s] for o, s in zip(EXT_OFF, EXT_SIZE)]))]), "gather")


def test_scatter(torch_cuda, comp):
    torch = torch_cuda
    a, b = rand(53, 1 << 20), rand(54, 1 << 20)
    d_in, d_a, d_b = buffers(torch, a, b)
    dst_off, pos = [], 64
    for k, s in enumerate(EXT_SIZE):
        dst_off.append(pos + k % 3)
        pos += s + 40
    d_out = canaries(torch, pos + 64)
    S.staged_call(torch, "scatter",
                  lambda: comp.scatter(d_in.data_ptr(), EXT_OFF, EXT_SIZE, d_out.data_ptr(), dst_off),
                  [(d_in, d_a, d_b)], [d_out])
    same(d_out, image(pos + 64, [(t, b[o:o + s]) for t, o, s in zip(dst_off, EXT_OFF, EXT_SIZE)]), "scatter")


def test_adler32(torch_cuda, comp):
    torch = torch_cuda
    a, b = rand(55, 1 << 20), rand(56, 1 << 20)
    d_in, d_a, d_b = buffers(torch, a, b)
    got, idle = S.staged_call(torch, "adler32", lambda: comp.adler32(d_in.data_ptr(), EXT_OFF, EXT_SIZE),
                              [(d_in, d_a, d_b)])
    want = [zlib.adler32(b[o:o + s].tobytes()) for o, s in zip(EXT_OFF, EXT_SIZE)]
    assert idle.tolist() == want
    assert got.tolist() == want, "the stale input's sums" if got.tolist() == [
        zlib.adler32(a[o:o + s].tobytes()) for o, s in zip(EXT_OFF, EXT_SIZE)] else "neither input's sums"


def test_lzo_compress(torch_cuda, comp):
    from zbackup_amd.bundle import lzo_capacity
    if lzo_oracle.lzo_lib() is None:
        pytest.skip("liblzo2 not in this image")
    torch = torch_cuda
    kinds, sizes = ("text", "repeats", "random", "runs"), (60000, 49173, 20, 30001)
    pa = [lzo_payload(k, n, 60 + j) for j, (k, n) in enumerate(zip(kinds, sizes))]
    pb = [lzo_payload(k, n, 70 + j) for j, (k, n) in enumerate(zip(kinds, sizes))]
    pay_off = [1 + sum(sizes[:j]) + 3 * j for j in range(4)]
    host = [np.zeros(pay_off[-1] + sizes[-1] + 8, dtype=np.uint8) for _ in range(2)]
    for img, ps in zip(host, (pa, pb)):
        for o, p in zip(pay_off, ps):
            img[o:o + len(p)] = p
    d_in, d_a, d_b = buffers(torch, host[0], host[1])
    out_off, pos = [], 64
    for n in sizes:
        out_off.append(pos)
        pos += lzo_capacity(n) + 64
    d_out = canaries(torch, pos)
    got, _ = S.staged_call(torch, "lzo compress",
                           lambda: comp.compress(d_in.data_ptr(), pay_off, sizes, d_out.data_ptr(), out_off),
                           [(d_in, d_a, d_b)], [d_out])
    out = d_out.cpu().numpy()
    keep = np.ones(pos, dtype=bool)
    for j, (o, n, p) in enumerate(zip(out_off, sizes, pb)):
        want = lzo_oracle.frame(p.tobytes())
        assert int(got[j]) == len(want) and out[o:o + len(want)].tobytes() == want, \
            f"payload {j}: not liblzo2's frame of the fresh payload" + \
            (" but of the stale one" if out[o:o + int(got[j])].tobytes() == lzo_oracle.frame(pa[j].tobytes()) else "")
        keep[o:o + lzo_capacity(n)] = False
    assert (out[keep] == CANARY).all()


# ---- AES and the bundle file ----

CHAIN = [16, 4096, 16384, 48]


def _chains(seed):
    n = sum(CHAIN)
    in_off = [sum(CHAIN[:k]) for k in range(4)]
    out_off, pos = [], 32
    for ln in CHAIN:
        out_off.append(pos)
        pos += ln + 32
    ivs = rand(seed, 64).tobytes()
    return n, in_off, out_off, pos, ivs


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_aes(torch_cuda, comp, decrypt):
    torch = torch_cuda
    n, in_off, out_off, total, ivs = _chains(80)
    plain = [rand(81, n), rand(82, n)]
    enc = [b"".join(aes_ref.cbc_encrypt(KEY, ivs[16 * k:16 * k + 16], p[o:o + ln].tobytes())
                    for k, (o, ln) in enumerate(zip(in_off, CHAIN))) for p in plain]
    src = [np.frombuffer(e, dtype=np.uint8) for e in enc] if decrypt else plain
    want = plain[1].tobytes() if decrypt else enc[1]
    d_in, d_a, d_b = buffers(torch, src[0], src[1])
    d_out = canaries(torch, total)
    fn = comp.aes_decrypt if decrypt else comp.aes_encrypt
    S.staged_call(torch, "aes_decrypt" if decrypt else "aes_encrypt",
                  lambda: fn(KEY, d_in.data_ptr(), in_off, CHAIN, d_out.data_ptr(), out_off, iv=ivs),
                  [(d_in, d_a, d_b)], [d_out])
    same(d_out, image(total, [(t, want[o:o + ln]) for t, o, ln in zip(out_off, in_off, CHAIN)]), "aes")


BODY = [5000, 1, 12345, 4088]


def _files(keyed, seed):
    """Four bundle files' prefixes, bodies and reference bytes; the prefixes are the call's arguments."""
    rng = np.random.default_rng(seed)
    pre = []
    for k in range(4):
        lead = rng.integers(0, 256, 16, dtype=np.uint8).tobytes() if keyed else b""
        pre.append(lead + aes_ref.message(b"\x08\x01") +
                   aes_ref.message(rng.integers(0, 256, 28 * (k + 1), dtype=np.uint8).tobytes()))
    return pre


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_seal(torch_cuda, comp, keyed):
    torch = torch_cuda
    key = KEY if keyed else None
    pre = _files(keyed, 90)
    body_off = [8 + sum(BODY[:k]) + 8 * k for k in range(4)]
    imgs = [rand(91, body_off[-1] + BODY[-1] + 8), rand(92, body_off[-1] + BODY[-1] + 8)]
    want = [aes_ref.seal_ref(key, p, imgs[1][o:o + n].tobytes()) for p, o, n in zip(pre, body_off, BODY)]
    file_off, pos = [], 32
    for f in want:
        file_off.append(pos)
        pos += (len(f) + 15) // 16 * 16 + 32
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    d_out = canaries(torch, pos)
    got, _ = S.staged_call(torch, f"seal ({'keyed' if keyed else 'plain'})",
                           lambda: comp.seal(key, pre, d_in.data_ptr(), body_off, BODY, d_out.data_ptr(), file_off),
                           [(d_in, d_a, d_b)], [d_out])
    assert [int(s) for s in got] == [len(f) for f in want]
    same(d_out, image(pos, list(zip(file_off, want))), "seal")


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_unseal(torch_cuda, comp, keyed):
    torch = torch_cuda
    key = KEY if keyed else None
    pre = _files(keyed, 93)
    sealed = [[aes_ref.seal_ref(key, p, rand(seed + k, n).tobytes()) for k, (p, n) in enumerate(zip(pre, BODY))]
              for seed in (94, 98)]
    sizes = [len(f) for f in sealed[1]]
    assert sizes == [len(f) for f in sealed[0]]
    caps = [(s + 15) // 16 * 16 for s in sizes]
    file_off = [16 + sum(caps[:k]) + 16 * k for k in range(4)]
    plain_off, pos = [], 32
    for c in caps:
        plain_off.append(pos)
        pos += c + 32
    imgs = [np.zeros(file_off[-1] + caps[-1] + 16, dtype=np.uint8) for _ in range(2)]
    for img, files in zip(imgs, sealed):
        for o, f in zip(file_off, files):
            img[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    d_out = canaries(torch, pos)
    lay, _ = S.staged_call(torch, f"unseal ({'keyed' if keyed else 'plain'})",
                           lambda: comp.unseal(key, d_in.data_ptr(), file_off, sizes, d_out.data_ptr(), plain_off),
                           [(d_in, d_a, d_b)], [d_out])
    pieces = []
    for k, f in enumerate(sealed[1]):
        st, ref_lay, plain = aes_ref.unseal_ref(key, f)
        assert st == aes_ref.OK and int(lay[k]["status"]) == 0, (k, int(lay[k]["status"]))
        for name, v in ref_lay.items():
            assert int(lay[k][name]) == v, (k, name)
        pieces.append((plain_off[k], plain))
    same(d_out, image(pos, pieces), "unseal")


# ---- adoption ----

def test_chunk_meta(torch_cuda):
    from zbackup_amd import Adopter
    from zbackup_amd.chunker import SEED_DTYPE
    torch = torch_cuda
    sizes = [W, W, 1, 17, W - 1, W, 1024, W]
    off = [3 + sum(sizes[:k]) + 5 * k for k in range(8)]
    imgs, chunks = [], []
    for seed in (100, 101):
        img = rand(seed, off[-1] + sizes[-1] + 7)
        imgs.append(img)
        chunks.append([img[o:o + s].tobytes() for o, s in zip(off, sizes)])
    want = meta_ref.records(chunks[1], W)
    expect = np.zeros(8, dtype=SEED_DTYPE)
    expect["sha1"], expect["rolling"], expect["size"] = want["sha1"], want["rolling"], want["size"]
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    with Adopter(W) as ad:
        (got, status), _ = S.staged_call(torch, "chunk_meta",
                                         lambda: ad.chunk_meta(d_in.data_ptr(), len(imgs[1]), off, sizes, expect),
                                         [(d_in, d_a, d_b)])
        n_bad = ad.n_bad
    assert status.tolist() == [0] * 8 and n_bad == 0, f"statuses {status.tolist()}: the ids are not the fresh chunks'"
    assert got.tobytes() == want.tobytes()


# ---- index files and BundleInfo bodies ----

INDEX_ARRAYS = ("status", "index_first", "bundle_ids", "bundle_first", "sizes", "ids")


def _index_files(key):
    """Two sets of four index files of equal sizes, with other ids."""
    out = []
    for seed in (110, 111):
        rng = random.Random(seed)
        out.append([IR.write(IR.rand_bundles(rng, counts, [65536]), key, RND)
                    for counts in ([3, 0, 40], [1], [], [7, 7])])
    assert [len(f) for f in out[0]] == [len(f) for f in out[1]]
    return out


def _same_index(got, files, key):
    ref = IR.read_many(files, key)
    assert ref["status"].tolist() == [0] * len(files)
    for name in INDEX_ARRAYS:
        g, w = getattr(got, name), ref[name]
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
@pytest.mark.parametrize("resident", [False, True], ids=["load_device", "load_resident_device"])
def test_index_load(torch_cuda, comp, keyed, resident):
    from zbackup_amd import IndexLoader
    torch = torch_cuda
    key = KEY if keyed else None
    files = _index_files(key)
    packed = [IndexLoader._pack(f) for f in files]
    off, size = packed[1][1], packed[1][2]
    d_in, d_a, d_b = buffers(torch, packed[0][0], packed[1][0])
    ld = IndexLoader(ctx=comp._ctx, key=key)

    def call():
        if not resident:
            return ld.load_device(d_in.data_ptr(), off, size)
        with ld.load_resident_device(d_in.data_ptr(), off, size) as rs:
            assert rs.n_files == 4
            return rs.fetch()
    got, _ = S.staged_call(torch, ("load_resident_device" if resident else "load_device") +
                           (" (keyed)" if keyed else " (plain)"), call, [(d_in, d_a, d_b)])
    _same_index(got, files[1], key)


def test_bundle_infos_device(torch_cuda, comp):
    from zbackup_amd import IndexLoader
    torch = torch_cuda
    counts = [5, 0, 130, 1]
    bodies = []
    for seed in (120, 121):
        rng = random.Random(seed)
        bodies.append([IR.bundle_info(recs) for _, recs in IR.rand_bundles(rng, counts, [65536])])
    lens = [len(x) for x in bodies[1]]
    assert lens == [len(x) for x in bodies[0]]
    info_off = [7 + sum(lens[:k]) + 3 * k for k in range(4)]
    imgs = [np.full(info_off[-1] + lens[-1] + 9, 0xA5, dtype=np.uint8) for _ in range(2)]
    for img, bs in zip(imgs, bodies):
        for o, x in zip(info_off, bs):
            img[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    ld = IndexLoader(ctx=comp._ctx)
    got, _ = S.staged_call(torch, "bundle_infos_device",
                           lambda: ld.bundle_infos_device(d_in.data_ptr(), info_off, lens), [(d_in, d_a, d_b)])
    assert got.status.tolist() == [0] * 4
    for k, x in enumerate(bodies[1]):
        want = IR.read_bundle_info(x)
        assert len(want) == counts[k] and got[k] == [(bytes(c), int(s)) for c, s in want], k


# ---- LZMA bundles ----

def test_xz_decode(torch_cuda, comp):
    from zbackup_amd.bundle import BundleDecompressor
    if not XR.available():
        pytest.skip(XR.why_not())
    torch = torch_cuda
    kinds, sizes = ("text", "halfdup", "random", "period65"), (30000, 20001, 2049, 65537)
    pays = [[XI.payload(k, n, seed + j).tobytes() for j, (k, n) in enumerate(zip(kinds, sizes))] for seed in (130, 140)]
    streams = [[XR.compress(p) for p in ps] for ps in pays]
    room = [(max(len(x), len(y)) + 15) // 16 * 16 for x, y in zip(*streams)]
    in_off = [sum(room[:k]) for k in range(4)]
    imgs = [np.zeros(sum(room), dtype=np.uint8) for _ in range(2)]
    for img, ss in zip(imgs, streams):
        for o, s in zip(in_off, ss):
            img[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    in_size = [len(s) for s in streams[1]]
    out_off, pos = [], 64
    for n in sizes:
        out_off.append(pos + 1)
        pos += n + 64
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    d_out = canaries(torch, pos)
    with BundleDecompressor(ctx=comp._ctx) as dec:
        res, _ = S.staged_call(torch, "xz decode",
                               lambda: dec.decode(d_in.data_ptr(), in_off, in_size, d_out.data_ptr(), out_off, sizes,
                                                  strict=False), [(d_in, d_a, d_b)], [d_out])
    assert [int(r["status"]) for r in res] == [XR.OK] * 4, "the streams read are not the fresh ones"
    assert [int(r["consumed"]) for r in res] == in_size and [int(r["decoded"]) for r in res] == list(sizes)
    same(d_out, image(pos, [(o, lzma.decompress(s)) for o, s in zip(out_off, streams[1])]), "xz decode")
    assert [lzma.decompress(s) for s in streams[1]] == pays[1]


def test_upload(torch_cuda, comp):
    """Write after write alone: the fill queued over the destination must not land after the upload."""
    from zbackup_amd.bundle import BundleDecompressor
    torch = torch_cuda
    data = rand(150, (1 << 20) - 5)
    d_out = canaries(torch, len(data) + 128)
    with BundleDecompressor(ctx=comp._ctx) as dec:
        S.staged_call(torch, "upload", lambda: dec.upload(d_out.data_ptr() + 64, data), [], [d_out])
    same(d_out, image(len(data) + 128, [(64, data)]), "upload")


def test_xz_encode(torch_cuda, comp, tmp_path):
    torch = torch_cuda
    kinds = ("text", "halfdup", "alphabet4", "random")
    pays = [[XI.payload(k, 2048 - j, seed + j).tobytes() for j, k in enumerate(kinds)] for seed in (160, 170)]
    ref, _ = E.run(E.build_exe(tmp_path, sanitize=False), tmp_path, [(4, p) for p in pays[1]])
    sizes = [len(p) for p in pays[1]]
    pay_off = [1 + sum(sizes[:k]) + 3 * k for k in range(4)]
    imgs = [np.zeros(pay_off[-1] + sizes[-1] + 8, dtype=np.uint8) for _ in range(2)]
    for img, ps in zip(imgs, pays):
        for o, p in zip(pay_off, ps):
            img[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    caps = [comp.xz_capacity(n) for n in sizes]
    out_off, pos = [], 64
    for c in caps:
        out_off.append(pos + 3)
        pos += c + 64
    d_in, d_a, d_b = buffers(torch, imgs[0], imgs[1])
    d_out = canaries(torch, pos + 64)
    res, _ = S.staged_call(torch, "xz encode",
                           lambda: comp.compress_xz(d_in.data_ptr(), pay_off, sizes, d_out.data_ptr(), out_off,
                                                    out_cap=caps, strict=False), [(d_in, d_a, d_b)], [d_out])
    assert [int(r["status"]) for r in res] == [XR.OK] * 4
    assert [int(r["size"]) for r in res] == [len(s) for _, _, s in ref]
    same(d_out, image(pos + 64, [(o, s) for o, (_, _, s) in zip(out_off, ref)]), "xz encode")
    for (_, _, s), p in zip(ref, pays[1]):
        assert lzma.decompress(s) == p
