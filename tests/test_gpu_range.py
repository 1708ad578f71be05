"""GPU tests of the random-access restore (zc_range_read, IndexedRestorer):
batches of reads at every entry edge and destination alignment, thousands of
tiny entries under one piece, stream positions past 2^32, slots that come and
go between calls, and a chunked stream's bundles served range by range with
only the bundles each batch needs resident.  Every destination lies between
0xEE canaries, which are checked."""
import numpy as np
import pytest

from oracle import lzo_oracle, oracle
from tests import range_ref

pytestmark = pytest.mark.gpu

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
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


def _layout(rng, reads):
    """Destinations for the reads, in shuffled order, 1-40 canary bytes apart,
    the k-th placed at alignment k mod 16; returns (dst_off, bytes in all)."""
    dst_off, pos = [0] * len(reads), 16
    for k, i in enumerate(rng.permutation(len(reads))):
        pos += int(rng.integers(1, 40))
        pos += (k % 16 - pos) % 16
        dst_off[i] = pos
        pos += reads[i][1]
    return dst_off, pos + 16


def _serve(torch, index, reads, dst_off, room):
    d_dst = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    index.read(reads, d_dst.data_ptr(), dst_off)
    return d_dst.cpu().numpy()


def _compare(got, reads, dst_off, room, expect):
    """expect(offset, size) -> the bytes; everything else must be canary."""
    want = np.full(room, CANARY, dtype=np.uint8)
    for (o, n), t in zip(reads, dst_off):
        want[t:t + n] = expect(o, n)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        t, i = max([(t, k) for k, t in enumerate(dst_off) if t <= at], default=(None, None))
        raise AssertionError(f"first wrong byte at {at} of {room}; the destination before it is {t}, of read "
                             f"{i}: {reads[i] if i is not None else None}")


def test_edges(torch_cuda, comp):
    """The first test to run the kernel: every entry edge, every size class of
    the copy body, every destination alignment."""
    from zbackup_amd import RangeIndex, Restorer
    from zbackup_amd.restore import RestorePlan
    torch = torch_cuda
    rng = np.random.default_rng(21)
    sizes = [0, 1, 2, 15, 16, 17, 31, 33, 255, 1024, 4095, 4096, 4097, 16383, 65535, 65536, 65537, 131072 + 5, 300001]
    sizes = [sizes[k % len(sizes)] for k in rng.permutation(3 * len(sizes))]
    # three slots inside one buffer, so the same bytes can go through Restorer.replay; sources
    # at odd offsets, and the second slot's base pointer is odd
    slot_size = [1 << 20, (1 << 20) - 7, 700001]
    slot_base = [16, (1 << 20) + 33, (2 << 20) + 64]
    work = rng.integers(0, 256, (3 << 20), dtype=np.uint8)
    slot = [int(rng.integers(0, 3)) for _ in sizes]
    off = [int(rng.integers(0, (slot_size[s] - n) // 2)) * 2 + 1 for s, n in zip(slot, sizes)]
    assert all(o + n <= slot_size[s] for o, n, s in zip(off, sizes, slot))
    stream = np.concatenate([work[slot_base[s] + o:slot_base[s] + o + n] for s, o, n in zip(slot, off, sizes)])
    total = len(stream)
    pos = range_ref.positions(sizes)
    reads = []
    for edge in pos:
        for d in (-1, 0, 1):
            for n in (1, 17, 4097, 65537):
                o = int(edge) + d
                if 0 <= o and o + n <= total:
                    reads.append((o, n))
    assert len(reads) > 600
    dst_off, room = _layout(rng, reads)
    assert {t % 16 for t in dst_off} == set(range(16))
    d_work = torch.from_numpy(work).cuda()
    with RangeIndex(slot_size, slot, off, sizes, comp=comp) as index:
        assert index.total == total
        for k in range(3):
            index.set_slot(k, d_work.data_ptr() + slot_base[k])
        assert (d_work.data_ptr() + slot_base[1]) % 2 == 1
        got = _serve(torch, index, reads, dst_off, room)
        _compare(got, reads, dst_off, room, lambda o, n: stream[o:o + n])
        assert index.last_stats()[2] == sum((n + 65535) // 65536 for _, n in reads)
        # the whole stream in one read is what Restorer.replay writes for the same plan
        whole = _serve(torch, index, [(0, total)], [16], total + 32)
    plan = RestorePlan()
    plan.length = total
    plan.src_off = np.array([slot_base[s] + o for s, o in zip(slot, off)], dtype=np.uint64)
    plan.sizes = np.array(sizes, dtype=np.uint64)
    plan.dst_off = pos[:-1].copy()
    d_out = torch.full((total + 32,), CANARY, dtype=torch.uint8, device="cuda")
    with Restorer(ctx=comp._ctx) as rs:
        assert rs.replay(plan, d_work.data_ptr(), d_out.data_ptr() + 16, total) == total
    assert np.array_equal(whole, d_out.cpu().numpy())
    assert np.array_equal(whole[16:-16], stream) and (whole[:16] == CANARY).all() and (whole[-16:] == CANARY).all()


def test_tiny_entries(torch_cuda, comp):
    """5,000 entries of 0-3 bytes between two 64 KiB chunks: one piece walks
    thousands of entries."""
    from zbackup_amd import RangeIndex
    torch = torch_cuda
    rng = np.random.default_rng(22)
    sizes = [65536] + [int(v) for v in rng.integers(0, 4, 5000)] + [65536]
    slots = [rng.integers(0, 256, 200000, dtype=np.uint8), rng.integers(0, 256, 9001, dtype=np.uint8)]
    slot = [0] + [1] * 5000 + [0]
    off = [3] + [int(v) for v in rng.integers(0, 8990, 5000)] + [100001]
    stream = np.concatenate([slots[s][o:o + n] for s, o, n in zip(slot, off, sizes)])
    total = len(stream)
    reads = [(int(rng.integers(0, total - n + 1)), n) for n in (1, 100, 20000) for _ in range(200)]
    reads += [(65536 - 50, 20000), (total - 65536 - 10000, 20000)]  # across all of the tiny entries' ends
    dst_off, room = _layout(rng, reads)
    d_slots = [torch.from_numpy(s).cuda() for s in slots]
    with RangeIndex([len(s) for s in slots], slot, off, sizes, comp=comp) as index:
        for k, d in enumerate(d_slots):
            index.set_slot(k, d.data_ptr())
        got = _serve(torch, index, reads, dst_off, room)
    _compare(got, reads, dst_off, room, lambda o, n: stream[o:o + n])


def test_past_4gib(torch_cuda, comp):
    """One 1 MiB extent emitted 4,200 times: a 4.1 GiB stream over a 1 MiB slot."""
    from zbackup_amd import RangeIndex
    torch = torch_cuda
    rng = np.random.default_rng(23)
    ext, reps = 1 << 20, 4200
    data = rng.integers(0, 256, ext, dtype=np.uint8)
    total = ext * reps
    assert total > 1 << 32
    reads = []
    for n in (1, 16, 131077):
        reads += [((1 << 32) - n // 2 - d, n) for d in (0, 1)]  # straddling 2^32 (n = 1: at and below it)
        reads += [((1 << 32) - n, n), (1 << 32, n), (total - n, n)]
    dst_off, room = _layout(rng, reads)
    d_data = torch.from_numpy(data).cuda()
    with RangeIndex([ext], [0] * reps, [0] * reps, [ext] * reps, comp=comp) as index:
        assert index.total == total
        index.set_slot(0, d_data.data_ptr())
        got = _serve(torch, index, reads, dst_off, room)
    _compare(got, reads, dst_off, room, lambda o, n: data[(o + np.arange(n, dtype=np.int64)) % ext])


def test_residency(torch_cuda, comp):
    """Slots cleared, set and moved between calls; what the host refuses writes nothing."""
    from zbackup_amd import RangeIndex, ZcError
    torch = torch_cuda
    rng = np.random.default_rng(24)
    slots = [rng.integers(0, 256, n, dtype=np.uint8) for n in (5000, 70000, 333)]
    slot, off, sizes = [0, 1, 2, 1, 0], [10, 0, 3, 100, 0], [4000, 70000, 330, 65000, 5000]
    stream = np.concatenate([slots[s][o:o + n] for s, o, n in zip(slot, off, sizes)])
    total = len(stream)
    reads = [(3990, 20), (74000, 331), (0, 1), (total - 5001, 5001)]  # slots 0+1, 1+2+1, 0, 1+0
    dst_off, room = _layout(rng, reads)
    d_slots = [torch.from_numpy(s).cuda() for s in slots]
    d_dst = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")

    def all_canary():
        return bool((d_dst == CANARY).all())

    with RangeIndex([len(s) for s in slots], slot, off, sizes, comp=comp) as index:
        index.set_slot(0, d_slots[0].data_ptr())
        index.set_slot(1, d_slots[1].data_ptr())
        assert index.needs(reads) == [0, 1, 2] and index.needs(reads[:1]) == [0, 1]
        with pytest.raises(ZcError, match=r"zc_range_read failed \(-1\): zc_range_read: slot 2 is not resident"):
            index.read(reads, d_dst.data_ptr(), dst_off)
        assert all_canary()
        index.read(reads[:1], d_dst.data_ptr(), dst_off[:1])  # a batch that does not touch slot 2 is served
        assert not all_canary()
        d_dst.fill_(CANARY)
        index.set_slot(2, d_slots[2].data_ptr())
        index.read(reads, d_dst.data_ptr(), dst_off)
        _compare(d_dst.cpu().numpy(), reads, dst_off, room, lambda o, n: stream[o:o + n])
        # the slot's pointer replaced by a copy at another address (an odd one), the old one scribbled over
        moved = torch.empty(len(slots[1]) + 1, dtype=torch.uint8, device="cuda")
        moved[1:] = d_slots[1]
        index.set_slot(1, moved.data_ptr() + 1)
        d_slots[1].fill_(0x55)
        d_dst.fill_(CANARY)
        index.read(reads, d_dst.data_ptr(), dst_off)
        _compare(d_dst.cpu().numpy(), reads, dst_off, room, lambda o, n: stream[o:o + n])
        # an index-owned copy replaces that one; dropping it makes the slot absent again
        index.upload_slot(1, slots[1].tobytes())
        moved.fill_(0x55)
        d_dst.fill_(CANARY)
        index.read(reads, d_dst.data_ptr(), dst_off)
        _compare(d_dst.cpu().numpy(), reads, dst_off, room, lambda o, n: stream[o:o + n])
        assert index.read_host(reads) == [stream[o:o + n].tobytes() for o, n in reads]
        d_dst.fill_(CANARY)
        # out of range: nothing is written, not even the reads before it
        for bad in ((total - 5, 6), (total + 1, 0), (2 ** 64 - 1, 2)):
            with pytest.raises(ZcError, match="out of range"):
                index.read(reads + [bad], d_dst.data_ptr(), dst_off + [0])
        with pytest.raises(ZcError, match="out of range"):
            index.read_host([(total, 1)])
        # no reads, and reads of no bytes (one at the very end), succeed and write nothing
        index.read([], d_dst.data_ptr(), [])
        index.read([(0, 0), (total, 0), (4000, 0)], d_dst.data_ptr(), [16, 17, 18])
        assert index.read_host([(total, 0)]) == [b""] and index.read_host([]) == []
        assert all_canary()
        index.drop_slot(1)
        with pytest.raises(ZcError, match="slot 1 is not resident"):
            index.read(reads, d_dst.data_ptr(), dst_off)
        assert all_canary()


def test_end_to_end(torch_cuda, comp):
    """test_restore_end_to_end's stream and bundles -- written on the GPU, read
    back through liblzo2, given in shuffled order -- served range by range by
    an IndexedRestorer with only the bundles each batch needs resident."""
    if lzo_oracle.lzo_lib() is None:
        pytest.skip("liblzo2 not in this image")
    from tests.range_stream import chunk_and_bundle, mixed_stream, random_reads
    from zbackup_amd import IndexedRestorer
    from zbackup_amd.bundle import lzo_capacity
    torch = torch_cuda
    oracle.build()
    data = mixed_stream()
    d = torch.from_numpy(data).cuda()
    backup_data, ids, offs, sizes, bundle_of, nb = chunk_and_bundle(d, len(data))
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
    rng = np.random.default_rng(25)
    reads = random_reads(rng, len(data), 300, 200000)
    resident, uploads = set(), 0
    with IndexedRestorer(backup_data, infos, ctx=comp._ctx) as ir:
        assert ir.size == len(data)
        at = 0
        for batch in (1, 7, 292):
            part = reads[at:at + batch]
            at += batch
            want = set(ir.needs(part))
            assert want and want <= set(range(nb))
            for k in resident - want:
                ir.drop_payload(k)
            for k in want - resident:
                ir.upload_payload(k, lzo_oracle.unframe(framed[k]))
                uploads += 1
            resident = want
            dst_off, room = _layout(rng, part)
            got = _serve(torch, ir, part, dst_off, room)
            _compare(got, part, dst_off, room, lambda o, n: data[o:o + n])
        assert at == 300 and uploads >= len(resident)
        for o, n in reads[-20:]:
            assert ir.read_host(o, n) == data[o:o + n].tobytes()


def test_read_host_follows_default_stream_work(torch_cuda, comp):
    """A caller-owned slot filled on the default stream and read straight away,
    with no synchronisation in between: both forms of the read come after the fill.
    The device form's destination has a fill queued over it as well: the read
    lands on top of it, not under it."""
    from zbackup_amd import RangeIndex
    torch = torch_cuda
    n = 64 << 20
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    filler = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    d_slot = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((4096 + 32,), CANARY, dtype=torch.uint8, device="cuda")
    snap = torch.zeros_like(d_dst)
    want = src[-4096:].cpu().numpy()
    with RangeIndex([n], [0], [0], [n], comp=comp) as index:
        index.set_slot(0, d_slot.data_ptr())
        for form in ("host", "device"):
            d_slot.zero_()
            torch.cuda.synchronize()
            for _ in range(8):  # a few milliseconds of queued work ahead of the fill
                filler.fill_(1)
            d_slot.copy_(src)
            if form == "host":
                got = np.frombuffer(index.read_host([(n - 4096, 4096)])[0], dtype=np.uint8)
            else:
                # the destination too: a fill queued over it and a reader of that fill, both before the read
                d_dst.fill_(CANARY)
                snap.copy_(d_dst)
                index.read([(n - 4096, 4096)], d_dst.data_ptr(), [16])
                assert bool((snap == CANARY).all()), "the read wrote under a reader queued before it"
                whole = d_dst.cpu().numpy()
                assert (whole[:16] == CANARY).all() and (whole[-16:] == CANARY).all()
                got = whole[16:-16]
            assert np.array_equal(got, want), form


def test_more_pieces_than_one_launch_takes(torch_cuda, comp):
    """2^20 + 5 one-byte reads: the piece list is cut into two launches, the
    second starting in the middle of the batch."""
    from zbackup_amd import RangeIndex
    torch = torch_cuda
    rng = np.random.default_rng(27)
    sizes = rng.integers(0, 300, 2000)
    slots = [rng.integers(0, 256, 4000, dtype=np.uint8) for _ in range(3)]
    slot = rng.integers(0, 3, len(sizes))
    off = rng.integers(0, 3700, len(sizes))
    stream = np.concatenate([slots[s][o:o + n] for s, o, n in zip(slot, off, sizes)])
    count = (1 << 20) + 5
    offsets = rng.integers(0, len(stream), count)
    offsets[-5:] = [0, len(stream) - 1, 1, len(stream) - 2, 7]  # the second launch's reads
    reads = np.stack([offsets, np.ones(count, dtype=np.int64)], axis=1).astype(np.uint64)
    d_slots = [torch.from_numpy(s).cuda() for s in slots]
    d_dst = torch.full((count + 32,), CANARY, dtype=torch.uint8, device="cuda")
    with RangeIndex([len(s) for s in slots], slot, off, sizes, comp=comp) as index:
        for k, d in enumerate(d_slots):
            index.set_slot(k, d.data_ptr())
        index.read(reads, d_dst.data_ptr(), 16 + np.arange(count, dtype=np.uint64))
        assert index.last_stats()[2] == count
    got = d_dst.cpu().numpy()
    assert np.array_equal(got[16:-16], stream[offsets])
    assert (got[:16] == CANARY).all() and (got[-16:] == CANARY).all()
