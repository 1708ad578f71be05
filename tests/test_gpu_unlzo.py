"""GPU tests of the restore replay, through the C ABI: zc_bundle_scatter puts
every extent where it belongs (odd offsets, extents over the 64 KiB piece
size, one source extent to many destinations, empty extents) and writes
nothing else, and the Restorer replays a chunked stream's BackupInstruction
stream over its bundles -- written on the GPU, read back through liblzo2's
lzo1x_decompress_safe as the reference reads them, given in shuffled order --
to exactly the original bytes.  Outputs lie between 0xEE canaries, which are
checked."""
import numpy as np
import pytest

from oracle import lzo_oracle, oracle
from tests.lzo_inputs import payload

pytestmark = pytest.mark.gpu

CANARY = 0xEE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    if lzo_oracle.lzo_lib() is None:
        pytest.skip("liblzo2 not in this image")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    return torch


@pytest.fixture(scope="module")
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


def test_scatter_extents(torch_cuda, comp):
    """Sizes around the copy kernel's paths (the 16-byte head and tail, the
    four-loads-in-flight loop, the 64 KiB piece split), every source and
    destination alignment, each extent to one to three destinations."""
    torch = torch_cuda
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, 3 << 20, dtype=np.uint8)
    sizes = [0, 1, 2, 15, 16, 17, 31, 33, 255, 1024, 4095, 4096, 4097, 16383, 65535, 65536, 65537, 131072 + 5, 300001]
    src_off, size, dst_off, pos = [], [], [], 16
    for i, n in enumerate(sizes * 3):
        o = int(rng.integers(0, len(src) - n))
        for _ in range(1 + i % 3):  # the same source extent again
            pos += int(rng.integers(1, 40))
            src_off.append(o)
            size.append(n)
            dst_off.append(pos)
            pos += n
    order = rng.permutation(len(size))  # destinations in no particular order
    src_off, size, dst_off = [[v[k] for k in order] for v in (src_off, size, dst_off)]
    want = np.full(pos + 16, CANARY, dtype=np.uint8)
    for o, n, t in zip(src_off, size, dst_off):
        want[t:t + n] = src[o + 1:o + 1 + n]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((pos + 16,), CANARY, dtype=torch.uint8, device="cuda")
    comp.scatter(d_src.data_ptr() + 1, src_off, size, d_dst.data_ptr(), dst_off)  # an odd base pointer
    got = d_dst.cpu().numpy()
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"first wrong byte at {at} of {len(want)}")
    comp.scatter(d_src.data_ptr(), [], [], d_dst.data_ptr(), [])  # nothing to do
    assert np.array_equal(d_dst.cpu().numpy(), want)


def test_scatter_is_the_inverse_of_gather(torch_cuda, comp):
    torch = torch_cuda
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, 5 << 20, dtype=np.uint8)
    cuts = np.sort(rng.choice(np.arange(1, len(data)), 700, replace=False))
    offs = np.concatenate([[0], cuts])
    sizes = np.diff(np.concatenate([offs, [len(data)]]))
    perm = rng.permutation(len(offs))
    d = torch.from_numpy(data).cuda()
    d_pay = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    comp.gather(d.data_ptr(), offs[perm], sizes[perm], d_pay.data_ptr())  # the extents back to back, shuffled
    pay_off = np.concatenate([[0], np.cumsum(sizes[perm])[:-1]])
    d_back = torch.full((len(data) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    comp.scatter(d_pay.data_ptr(), pay_off, sizes[perm], d_back.data_ptr() + 16, offs[perm])
    assert torch.equal(d_back[16:-16], d)
    assert (d_back[:16] == CANARY).all() and (d_back[-16:] == CANARY).all()


def test_restore_end_to_end(torch_cuda, comp):
    """stream -> records -> Writer::add bundles -> gather -> lzo1x_1 (all on
    the GPU) -> get_backup_data(); then the restore: the bundles the stream
    names decoded by liblzo2 (the reference's decoder), one upload, and the
    Restorer's scatter over the shuffled bundles gives the original stream."""
    import hashlib

    from zbackup_amd import ZC_BYTES, ZC_CHUNK_DUP, ZC_CHUNK_NEW, BackupCreator, Restorer, Sha256
    from zbackup_amd.bundle import frame_info, lzo_capacity, plan_bundles
    torch = torch_cuda
    W = 4096
    a, b = payload("text", 6 << 20, 11), payload("random", 5 << 20, 12)
    data = np.concatenate([a, b, a[3:3 << 20], np.zeros(2 << 20, np.uint8), b[:2 << 20], payload("runs", 4 << 20, 13),
                           a[:2 * W], payload("random", 77, 14)])  # two whole chunks again, then a short tail
    d = torch.from_numpy(data).cuda()
    with BackupCreator(chunk_max_size=W, sha1=True) as bc:
        bc.chunk_device(d.data_ptr(), len(data))
        recs = bc.records()
        backup_data = bc.get_backup_data()
    kinds = recs["kind"]
    assert (kinds == ZC_CHUNK_DUP).sum() > 100 and (kinds == ZC_BYTES).sum() >= 1
    assert int(recs["size"].sum()) == len(data)
    # Writer::add: the saved chunks whose id the index does not hold yet
    seen, offs, sizes, ids = set(), [], [], []
    for r in recs[kinds == ZC_CHUNK_NEW]:
        cid = bytes(r["sha1"]) + int(r["rolling"]).to_bytes(8, "little")
        if cid not in seen:
            seen.add(cid)
            offs.append(int(r["offset"]))
            sizes.append(int(r["size"]))
            ids.append(cid)
    assert (kinds != ZC_BYTES).sum() > len(ids) + 100  # stored extents emitted more than once
    bundle_of, nb = plan_bundles(sizes)
    assert nb > 4
    d_payload = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    comp.gather(d.data_ptr(), offs, sizes, d_payload.data_ptr())
    pay_size = np.bincount(bundle_of, weights=sizes, minlength=nb).astype(np.uint64)
    pay_off = np.concatenate([[0], np.cumsum(pay_size)[:-1]]).astype(np.uint64)
    z_off = np.concatenate([[0], np.cumsum([lzo_capacity(int(s)) for s in pay_size])]).astype(np.uint64)
    d_z = torch.empty(int(z_off[-1]), dtype=torch.uint8, device="cuda")
    z_size = comp.compress(d_payload.data_ptr(), pay_off, pay_size, d_z.data_ptr(), z_off[:-1])
    z = d_z.cpu().numpy()
    order = np.random.default_rng(6).permutation(nb)
    framed = [z[int(z_off[k]):int(z_off[k]) + int(z_size[k])].tobytes() for k in order]
    infos = [[(ids[i], sizes[i]) for i in np.nonzero(bundle_of == k)[0]] for k in order]
    # the restore
    plan = Restorer.plan(backup_data, infos)
    assert plan.length == len(data) and sorted(plan.used) == list(range(nb))
    payloads = []
    for k, b_ in enumerate(plan.used):
        assert frame_info(framed[b_]) == (plan.pay_size[k], len(framed[b_]) - 16)
        payloads.append(lzo_oracle.unframe(framed[b_]))
    d_work = torch.from_numpy(plan.host_image(payloads)).cuda()
    d_out = torch.full((len(data) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    with Restorer(ctx=comp._ctx) as rs:
        n = rs.replay(plan, d_work.data_ptr(), d_out.data_ptr() + 16, len(data))
        with pytest.raises(Exception, match="room for"):
            rs.replay(plan, d_work.data_ptr(), d_out.data_ptr() + 16, len(data) - 1)
    assert n == len(data)
    assert torch.equal(d_out[16:16 + n], d)
    assert (d_out[:16] == CANARY).all() and (d_out[16 + n:] == CANARY).all()
    h = Sha256()
    h.add(d_out[16:16 + n].cpu().numpy())
    assert h.finish() == hashlib.sha256(data.tobytes()).digest()
