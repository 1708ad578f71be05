"""GPU tests of the paths that start from LZMA bundles as they lie on disk:
Restorer.replay_bodies, IndexedRestorer.decode_payload and
Adopter.adopt_bodies give what replay, upload_payload and adopt give from
payloads a host decoder produced -- with the payloads decoded on the device."""
import hashlib

import numpy as np
import pytest

from tests import xz_inputs as XI
from tests import xz_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason=R.why_not())]

W = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


def make_repo():
    """Three bundles of chunks cut from text-like, half-duplicated and random
    bytes (chunk sizes around W, the last of each short), their xz bodies, and
    an instruction stream that names most chunks, one twice, in shuffled order,
    with bytes_to_emit runs between them."""
    from zbackup_amd import chunk_id_blob, serialize_instruction
    rng = np.random.default_rng(4)
    bundles, payloads, chunks = [], [], []
    for b, (kind, n) in enumerate((("text", 70001), ("halfdup", 33000), ("random", 9000))):
        data = XI.payload(kind, n, 40 + b).tobytes()
        payloads.append(data)
        recs, pos = [], 0
        while pos < n:
            size = min(W if pos % (3 * W) else W - 1, n - pos)
            piece = data[pos:pos + size]
            blob = chunk_id_blob(hashlib.sha1(piece).digest()[:16], int(rng.integers(0, 2 ** 63)))
            recs.append((blob, size))
            chunks.append((blob, piece))
            pos += size
        bundles.append(recs)
    bodies = [R.compress(p) for p in payloads]
    order = list(rng.permutation(len(chunks)))[:len(chunks) - 3] + [1]
    stream, want = b"", b""
    for j, c in enumerate(order):
        blob, piece = chunks[c]
        raw = bytes(rng.integers(0, 256, j % 5, dtype=np.uint8)) if j % 4 == 0 else None
        stream += serialize_instruction(chunk_blob=blob, raw=raw if raw else None)
        want += piece + (raw or b"")
    return bundles, payloads, bodies, stream, want


@pytest.fixture(scope="module")
def repo():
    return make_repo()


def true_ids(adopter, fake, payloads):
    """The same chunks under their true ids (SHA-1 and rolling hash)."""
    from zbackup_amd import chunk_id_blob
    bundles = []
    for chunks, data in zip(fake, payloads):
        size = [s for _, s in chunks]
        off = np.concatenate([[0], np.cumsum(size)[:-1]])
        meta, _ = adopter.chunk_meta_host(data, off, size)
        bundles.append([(chunk_id_blob(m["sha1"].tobytes(), int(m["rolling"])), s) for m, s in zip(meta, size)])
    return bundles


def test_replay_bodies_restores_the_stream(torch_cuda, repo):
    from zbackup_amd import Restorer, ZcError
    torch = torch_cuda
    bundles, payloads, bodies, stream, want = repo
    with Restorer() as r:
        plan = r.plan(stream, bundles)
        used = [bodies[b] for b in plan.used]
        assert plan.bodies_work_size(used) == ((plan.work_size + 15) & ~15) + sum((len(b) + 15) & ~15 for b in used)
        d_work = torch.full((plan.bodies_work_size(used),), 0xEE, dtype=torch.uint8, device="cuda")
        d_out = torch.full((len(want) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        assert r.replay_bodies(plan, used, d_work.data_ptr(), d_out.data_ptr(), len(want)) == len(want)
        got = d_out.cpu().numpy()
        assert got[:len(want)].tobytes() == want and np.all(got[len(want):] == 0xEE)
        # the scratch buffer holds what host_image would have uploaded; the alignment gaps are untouched
        img = plan.host_image([payloads[b] for b in plan.used])
        work = d_work.cpu().numpy()
        gap = np.ones(plan.work_size, dtype=bool)
        for o, n in list(zip(plan.pay_off, plan.pay_size)) + [(plan.instr_off, len(stream))]:
            assert np.array_equal(work[o:o + n], img[o:o + n])
            gap[o:o + n] = False
        assert np.all(work[:plan.work_size][gap] == 0xEE)
        # a body with bytes behind its stream, and another bundle's body
        with pytest.raises(ZcError, match="bundle 0: the stream ends after"):
            r.replay_bodies(plan, [used[0] + b"\0"] + used[1:], d_work.data_ptr(), d_out.data_ptr(), len(want))
        with pytest.raises(ZcError, match="bundle"):
            r.replay_bodies(plan, used[::-1], d_work.data_ptr(), d_out.data_ptr(), len(want))


def test_indexed_restorer_decodes_a_payload(torch_cuda, repo):
    from zbackup_amd import IndexedRestorer, ZcError
    bundles, payloads, bodies, stream, want = repo
    with IndexedRestorer(stream, bundles) as ir:
        assert ir.size == len(want)
        for b in ir.plan.used:
            ir.decode_payload(b, bodies[b])
        for off, n in ((0, 1), (0, len(want)), (4095, 9000), (len(want) - 17, 17)):
            assert ir.read_host(off, n) == want[off:off + n]
        b0 = ir.plan.used[0]
        ir.decode_payload(b0, bodies[b0])  # again: the old buffer goes
        assert ir.read_host(100, 5000) == want[100:5100]
        with pytest.raises(ZcError, match="ZC_XZ_E_"):
            ir.decode_payload(b0, bodies[b0][:-5])
        assert ir.read_host(100, 5000) == want[100:5100]  # the slot kept its payload
        # an uploaded or caller-owned payload in its place, or a drop, frees the decoded buffer
        slot = ir.plan.used.index(b0)
        assert slot in ir._decoded
        ir.upload_payload(b0, payloads[b0])
        assert slot not in ir._decoded and ir.read_host(100, 5000) == want[100:5100]
        ir.decode_payload(b0, bodies[b0])
        ir.drop_payload(b0)
        assert not ir._decoded or slot not in ir._decoded


def test_adopt_bodies_equals_adopt(torch_cuda, repo):
    from zbackup_amd import Adopter
    fake, payloads, bodies, _, _ = repo
    damaged = bytearray(payloads[1])
    damaged[5000] ^= 1
    with Adopter(W) as a:
        bundles = true_ids(a, fake, payloads)
        payloads = [payloads[0], bytes(damaged), payloads[2]]
        bodies = [bodies[0], R.compress(damaged), bodies[2]]
        want = a.adopt(bundles, payloads)
        got = a.adopt_bodies(bundles, bodies)
        assert a.xz_stats["decode_ms"] > 0
    assert got.bad == want.bad and len(got.bad) == 1 and got.bad[0][0] == 1
    assert got.chunks == want.chunks and got.bytes == want.bytes
    assert np.array_equal(got.meta, want.meta)
