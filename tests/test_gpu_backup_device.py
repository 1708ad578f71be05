"""GPU tests of BackupCreator.backup_device: a backup whose data stays in HBM
from the chunker through backupFromFileHandle's shrink loop (zutils.cc:137-166),
against the same loops over the oracle (tests/test_gpu_adapter.py's _expected):
the final backup data, the iteration count, the length of every pass and the
NEW chunk ids handed to on_new, in order.  The figures of CASES were taken on the
CPU with the oracle; every comparison is exact."""
import hashlib

import numpy as np
import pytest

from oracle import oracle
from tests.test_gpu_adapter import _expected

pytestmark = pytest.mark.gpu

# (W, spec, data size, first pass N, iterations, final length, adds); None: not recorded, the oracle decides
CASES = [
    (256, "R1:65536,C0:65536,C0:65536,C0:65536", 262144, 256, 3, 98, 290),
    (256, "R1:40000,B7:50,C0:40000,R2:90,C0:40000,C100:30000,Z:3000,C0:40000", 193140, 160, 3, 44, 190),
    (128, "R1:20000,B7:50,C0:20000,R2:90,C0:20000,C100:15000,Z:3000,C0:20000,C0:20000,C0:20000", 138140, 158, 5, 68,
     221),
    (4096, "R3:600000,C5:300000,B9:2000,C0:600000,R4:100,C0:600000", 2102100, None, 1, 108, None),
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


def pass_lengths(data, W):
    """The length of the stream every pass of the oracle loops writes, the last, discarded one included."""
    from zbackup_amd.chunker import chunk_id_blob, serialize_instruction
    index, lengths = [], []
    buf = data
    while True:
        out = bytearray()
        for (k, off, size, h, sha) in oracle.chunk(buf, W, seeds=index):
            if k == "B":
                out += serialize_instruction(raw=buf[off:off + size].tobytes())
                continue
            if k == "N":
                index.append((bytes.fromhex(sha), h, size))
            out += serialize_instruction(chunk_blob=chunk_id_blob(bytes.fromhex(sha), h))
        lengths.append(len(out))
        if len(lengths) > 1 and len(out) >= len(buf):
            return lengths
        buf = np.frombuffer(bytes(out), dtype=np.uint8)


def run(torch, data, W):
    """backup_device on a fresh context: (data, iterations, pass lengths, [(pass, blobs)])."""
    from zbackup_amd import BackupCreator, chunk_id_blob
    t = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0") if data.size else None
    news = []
    with BackupCreator(W) as bc:
        def on_new(recs, d_stream, pass_no):
            assert (recs["kind"] == 0).all()
            news.append((pass_no, [chunk_id_blob(bytes(r["sha1"]), int(r["rolling"])) for r in recs]))
            if len(recs):  # the pass's stream is readable where it lies: the last NEW chunk's bytes give its id
                r = recs[-1]
                chunk = bc._download(d_stream + int(r["offset"]), int(r["size"]))
                assert hashlib.sha1(chunk).digest()[:16] == bytes(r["sha1"])
        got = bc.backup_device(t.data_ptr() if t is not None else 0, int(data.size), on_new=on_new)
        assert len(bc.records()) == 0  # the context refers to no buffer of the call
    return got + (news,)


@pytest.mark.parametrize("W,spec,size,first_new,iterations,final,adds", CASES, ids=[f"W{c[0]}" + f"-{c[2]}" for c in CASES])
def test_backup_device_vs_oracle_loops(torch_cuda, W, spec, size, first_new, iterations, final, adds):
    data = oracle.gen(spec)
    assert data.size == size
    want_data, want_it, want_adds, _ = _expected(data, W, [])
    want_lengths = pass_lengths(data, W)
    # the recorded figures are the oracle's
    assert (want_it, len(want_data)) == (iterations, final) and want_lengths[want_it] == final
    assert len(want_lengths) == want_it + 2 and want_lengths[-1] >= final
    assert adds is None or len(want_adds) == adds
    got, it, lengths, news = run(torch_cuda, data, W)
    assert it == want_it
    assert got == want_data
    assert lengths == want_lengths
    assert [k for k, _ in news] == list(range(it + 2))  # one call a pass, the discarded pass included
    assert first_new is None or len(news[0][1]) == first_new
    assert [b for _, blobs in news for b in blobs] == want_adds


def test_an_empty_stream(torch_cuda):
    data = np.zeros(0, dtype=np.uint8)
    want_data, want_it, want_adds, _ = _expected(data, 4096, [])
    assert (want_data, want_it, want_adds) == (b"", 0, [])
    got, it, lengths, news = run(torch_cuda, data, 4096)
    assert (got, it, lengths) == (b"", 0, [0, 0])
    assert news == [(0, []), (1, [])]


def test_a_stream_that_does_not_shrink(torch_cuda):
    data = oracle.gen("R5:65536")
    want_data, want_it, want_adds, _ = _expected(data, 65536, [])
    assert want_it == 0 and len(want_data) == 27 and len(want_adds) == 1
    got, it, lengths, news = run(torch_cuda, data, 65536)
    assert (got, it) == (want_data, 0)
    assert lengths == [27, 30] == pass_lengths(data, 65536)  # the 27 bytes come back as one bytes_to_emit
    assert [b for _, blobs in news for b in blobs] == want_adds


def test_backup_device_makes_no_host_round_trip(torch_cuda, monkeypatch):
    """No per-record read, no host serializer and no re-upload of a stream: the
    library's three entry points that would do them are never reached."""
    from zbackup_amd import BackupCreator, _lib
    L = _lib.load()
    calls = {}

    def counting(name):
        real = getattr(L, name)

        def shim(*args):
            calls[name] = calls.get(name, 0) + 1
            return real(*args)
        return shim

    for name in ("zc_read_stream", "zc_serialize_records", "zc_upload"):
        monkeypatch.setattr(L, name, counting(name))
    W, spec = CASES[1][:2]
    data = oracle.gen(spec)
    t = torch_cuda.from_numpy(data).to("cuda:0")
    with BackupCreator(W) as bc:
        got, it, lengths = bc.backup_device(t.data_ptr(), data.size)
        assert (it, len(got)) == CASES[1][4:6] and calls == {}
        # the shims do count: the host route through the same wrapper reaches two of them
        bc.chunk_device(t.data_ptr(), data.size)
        bc._serialize(bc.records())
        assert calls["zc_serialize_records"] == 2 and "zc_upload" not in calls
        bc.read_stream(0, 10)
        assert calls["zc_read_stream"] == 1
