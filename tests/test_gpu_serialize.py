"""GPU tests of zc_serialize_records_device: hand-built record arrays over a
stream of a few MiB in HBM, the downloaded output compared byte for byte with
b"".join(serialize_instruction(...)) and, for the records chunk_device cuts from
the same stream, with zc_serialize_records, the host serializer.  Guard bytes
stand before and after d_out and stay intact.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from tests import stream_order as S

pytestmark = pytest.mark.gpu

NAME = "zc_serialize_records_device: "
STAGE = 128          # zcser::kStage: the longest payload assembled in LDS
GUARD = 256
FILL = 0xA5
A_BYTES = 1 << 20    # the stream: A, 37 bytes, A again, then random bytes up to 3 MiB + 37
STREAM_BYTES = (3 << 20) + 37


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


@pytest.fixture(scope="module")
def stream(torch_cuda):
    """(host bytes, device tensor): random, with a repeat so that chunk_device cuts NEW, DUP and BYTES records."""
    rng = np.random.default_rng(1234)
    host = rng.integers(0, 256, STREAM_BYTES, dtype=np.uint8)
    host[A_BYTES + 37:2 * A_BYTES + 37] = host[:A_BYTES]
    return host, torch_cuda.from_numpy(host).to("cuda:0")


@pytest.fixture(scope="module")
def bc(torch_cuda):
    from zbackup_amd import BackupCreator
    with BackupCreator(65536) as c:
        yield c


def chunk_rec(rng, kind=0):
    from zbackup_amd import RECORD_DTYPE
    r = np.zeros(1, dtype=RECORD_DTYPE)
    r["kind"], r["size"] = kind, rng.integers(1, 1 << 32)  # a chunk's size and offset are not serialized
    r["offset"], r["rolling"] = rng.integers(0, 1 << 64, 2, dtype=np.uint64)
    r["sha1"] = rng.integers(0, 256, 16)
    return r


def bytes_rec(offset, size):
    from zbackup_amd import RECORD_DTYPE, ZC_BYTES
    r = np.zeros(1, dtype=RECORD_DTYPE)
    r["kind"], r["size"], r["offset"] = ZC_BYTES, size, offset
    return r


def cat(parts):
    from zbackup_amd import RECORD_DTYPE
    return np.concatenate(parts) if parts else np.zeros(0, dtype=RECORD_DTYPE)


def expected(recs, host):
    from zbackup_amd import ZC_BYTES, chunk_id_blob, serialize_instruction
    out = []
    for r in recs:
        if r["kind"] == ZC_BYTES:
            out.append(serialize_instruction(raw=host[int(r["offset"]):int(r["offset"]) + int(r["size"])].tobytes()))
        else:
            out.append(serialize_instruction(chunk_blob=chunk_id_blob(bytes(r["sha1"]), int(r["rolling"]))))
    return b"".join(out)


def device_call(torch, bc, recs, d_stream, stream_len, cap=None, shift=0):
    """The call with guards around d_out (which starts `shift` bytes off a 256-byte boundary).
    Returns (rc, message, n_out, guard before, output room, guard after)."""
    from zbackup_amd import serialized_size
    recs = np.ascontiguousarray(recs)
    need = serialized_size(recs)
    cap = need if cap is None else cap
    buf = torch.full((GUARD + shift + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    wrote = ctypes.c_uint64(1 << 60)
    rc = bc._L.zc_serialize_records_device(bc._ctx, recs.ctypes.data if len(recs) else None, len(recs),
                                           d_stream.data_ptr(), stream_len, buf.data_ptr() + GUARD + shift, cap,
                                           ctypes.byref(wrote))
    got = buf.cpu().numpy()
    at = GUARD + shift
    return rc, bc._L.zc_last_error(bc._ctx).decode(), wrote.value, got[:at], got[at:at + cap], got[at + cap:]


def check(torch, bc, stream, recs, what, shift=0):
    host, dev = stream
    want = expected(recs, host)
    rc, msg, n_out, before, body, after = device_call(torch, bc, recs, dev, len(host), shift=shift)
    assert rc == 0, (what, msg)
    assert n_out == len(want) == len(body), what
    assert (before == FILL).all() and (after == FILL).all(), f"{what}: a guard byte was written"
    if body.tobytes() != want:
        w = np.frombuffer(want, dtype=np.uint8)
        at = int(np.nonzero(body != w)[0][0])
        raise AssertionError(f"{what}: byte {at} of {len(want)} differs ({body[at]:#x}, expected {w[at]:#x})")
    st = bc.serialize_stats()
    big = int(((recs["kind"] == 2) & (recs["size"] > STAGE)).sum())
    pieces = int(sum((int(s) + 65535) // 65536 for s in recs["size"][(recs["kind"] == 2) & (recs["size"] > STAGE)]))
    assert (st["staged_msgs"], st["copy_pieces"]) == (len(recs) - big, pieces), what


SMALL = [0, 1, 15, 16, 17, 125, 126, 127, 128, 129, 130, 3, 64, 100]


def mix_records(rng, n, mix, host_len):
    """n records: chunks only ("chunk"), BYTES only ("bytes"), or alternating ("alt")."""
    parts = []
    for i in range(n):
        if mix == "chunk" or (mix == "alt" and i % 2 == 0):
            parts.append(chunk_rec(rng, kind=int(rng.integers(0, 2))))
        else:
            size = SMALL[i % len(SMALL)]
            parts.append(bytes_rec(int(rng.integers(0, host_len - size)), size))
    return cat(parts)


@pytest.mark.parametrize("mix", ["chunk", "bytes", "alt"])
def test_record_counts_around_the_group(torch_cuda, bc, stream, mix):
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 4097):
        check(torch_cuda, bc, stream, mix_records(rng, n, mix, STREAM_BYTES), f"{n} records, {mix}")


def test_bytes_sizes_at_every_step(torch_cuda, bc, stream):
    rng = np.random.default_rng(8)
    sizes = [0, 1, 15, 16, 17, 125, 126, 127, 128, 129, STAGE - 1, STAGE, STAGE + 1, 16381, 16382, 16383, 16384,
             65535, 65536, 65537, 2097151, 2097152]
    for size in sizes:
        off = int(rng.integers(0, STREAM_BYTES - size))
        check(torch_cuda, bc, stream, bytes_rec(off, size), f"one BYTES of {size}")
        check(torch_cuda, bc, stream, cat([chunk_rec(rng), bytes_rec(off, size), chunk_rec(rng, 1), bytes_rec(5, 9)]),
              f"a BYTES of {size} between chunks")
    # the whole stream as one bytes_to_emit, and the range that ends at its last byte
    check(torch_cuda, bc, stream, bytes_rec(0, STREAM_BYTES), "the whole stream")
    check(torch_cuda, bc, stream, cat([bytes_rec(STREAM_BYTES - 130, 130), bytes_rec(STREAM_BYTES, 0)]), "the last bytes")


def test_large_bytes_at_every_residue(torch_cuda, bc, stream):
    """16 destination residues (a leading BYTES of 0 to 15 bytes: 3 + k bytes of
    message, then the 5-byte header) crossed with 16 source residues."""
    rng = np.random.default_rng(9)
    for lead in range(16):
        for src in range(16):
            recs = cat([bytes_rec(40, lead), bytes_rec(4096 + src, 70001 + lead), chunk_rec(rng)])
            check(torch_cuda, bc, stream, recs, f"lead {lead} source residue {src}")
    # and an output that does not start on a 16-byte boundary
    for shift in (1, 7, 15):
        check(torch_cuda, bc, stream, mix_records(rng, 200, "alt", STREAM_BYTES), f"200 records, shift {shift}", shift)
        check(torch_cuda, bc, stream, cat([chunk_rec(rng), bytes_rec(33, 70000)]), f"a large BYTES, shift {shift}", shift)


def test_large_bytes_at_a_groups_ends(torch_cuda, bc, stream):
    rng = np.random.default_rng(10)
    for at in (0, 63, 64, 127, 128, 191):  # the first and the last record of a group
        parts = [chunk_rec(rng) if i % 3 else bytes_rec(100 + i, SMALL[i % len(SMALL)]) for i in range(192)]
        parts[at] = bytes_rec(1000 + at, 66000 + at)
        check(torch_cuda, bc, stream, cat(parts), f"a large BYTES as record {at}")
    # both ends of every group, and a group of large records only
    parts = [bytes_rec(i, 200 + i) if i % 64 in (0, 63) else chunk_rec(rng) for i in range(192)]
    check(torch_cuda, bc, stream, cat(parts), "large BYTES at both ends")
    check(torch_cuda, bc, stream, cat([bytes_rec(i, STAGE + 1 + i) for i in range(130)]), "large records only")


def test_every_other_kind_is_a_chunk(torch_cuda, bc, stream):
    rng = np.random.default_rng(11)
    recs = cat([chunk_rec(rng, kind) for kind in (0, 1, 7, 3, 0xFFFFFFFF, 7)])
    check(torch_cuda, bc, stream, recs, "kinds 0, 1, 7")
    host = stream[0]
    assert expected(recs, host)[54:57] == bytes([26, 0x0A, 24])  # kind 7: a 27-byte chunk message


@pytest.mark.parametrize("sha1", [True, False])
def test_against_the_host_serializer(torch_cuda, stream, sha1):
    """The records chunk_device cuts from the stream (kinds 0, 1 and 2, with and
    without ZC_FLAG_SHA1), through zc_serialize_records and through the device."""
    from zbackup_amd import BackupCreator
    host, dev = stream
    with BackupCreator(65536, sha1=sha1) as c:
        c.chunk_device(dev.data_ptr(), len(host))
        recs = c.records()
        assert set(recs["kind"].tolist()) == {0, 1, 2}
        assert bool(recs["sha1"].any()) == sha1
        for sub in (recs, recs[:5], recs[recs["kind"] != 0], recs[::-1]):
            want = c._serialize(sub)
            assert want == expected(sub, host)
            rc, msg, n_out, before, body, after = device_call(torch_cuda, c, sub, dev, len(host))
            assert rc == 0, msg
            assert body.tobytes() == want and (before == FILL).all() and (after == FILL).all()


def test_random_record_lists(torch_cuda, bc, stream):
    from zbackup_amd import RECORD_DTYPE
    for seed in range(50):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(1, 2001))
        recs = np.zeros(n, dtype=RECORD_DTYPE)
        u = rng.random(n)
        recs["kind"] = np.where(u < 0.5, rng.integers(0, 2, n), 2)
        recs["rolling"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        recs["sha1"] = rng.integers(0, 256, (n, 16))
        size = rng.integers(0, 140, n)
        large = np.nonzero(u > 0.97)[0][:6]  # a few payloads beyond the staging bound, some of several pieces
        size[large] = rng.integers(129, 200000, len(large))
        recs["size"] = size
        recs["offset"] = (rng.random(n) * (STREAM_BYTES - size + 1)).astype(np.uint64)
        assert int((recs["offset"] + recs["size"]).max()) <= STREAM_BYTES
        check(torch_cuda, bc, stream, recs, f"random list {seed} ({n} records)")


def test_refusals_leave_the_output_untouched(torch_cuda, bc, stream):
    host, dev = stream
    rng = np.random.default_rng(12)
    good = cat([chunk_rec(rng), bytes_rec(STREAM_BYTES - 300, 300), bytes_rec(7, 100)])
    bad = good.copy()
    bad["offset"][1] += 1
    rc, msg, n_out, before, body, after = device_call(torch_cuda, bc, bad, dev, len(host))
    assert (rc, msg) == (-1, NAME + f"record 1: bytes [{STREAM_BYTES - 299}, +300) past the end of a stream of "
                         f"{STREAM_BYTES} bytes")
    assert n_out == 1 << 60 and (body == FILL).all() and (before == FILL).all() and (after == FILL).all()
    need = len(expected(good, host))
    for cap in (0, need - 1):
        rc, msg, n_out, before, body, after = device_call(torch_cuda, bc, good, dev, len(host), cap=cap)
        assert (rc, msg) == (-1, NAME + f"the stream takes {need} bytes, the output has room for {cap}")
        assert n_out == need and (body == FILL).all() and (before == FILL).all() and (after == FILL).all()
    # more room than needed: only the stream's bytes are written
    rc, msg, n_out, before, body, after = device_call(torch_cuda, bc, good, dev, len(host), cap=need + 100)
    assert rc == 0 and n_out == need and body[:need].tobytes() == expected(good, host)
    assert (body[need:] == FILL).all() and (after == FILL).all()


def test_a_call_right_after_default_stream_work(torch_cuda, bc):
    """The stream is written on the default stream, the records are serialized at
    once: the call must read the fresh bytes and write under no queued fill."""
    torch = torch_cuda
    n = 1 << 20
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    stale = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    fresh = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    d_in = torch.empty_like(stale)
    rng = np.random.default_rng(13)
    recs = cat([chunk_rec(rng), bytes_rec(11, 90), bytes_rec(1000, 300001), chunk_rec(rng, 1), bytes_rec(n - 77, 77)])
    host = fresh.cpu().numpy()
    want = expected(recs, host)
    d_out = torch.empty(len(want) + 64, dtype=torch.uint8, device="cuda")
    wrote = ctypes.c_uint64()

    def call():
        return bc._L.zc_serialize_records_device(bc._ctx, recs.ctypes.data, len(recs), d_in.data_ptr(), n,
                                                 d_out.data_ptr(), len(want), ctypes.byref(wrote))

    staged, idle = S.staged_call(torch, "zc_serialize_records_device", call, inputs=[(d_in, stale, fresh)],
                                 outputs=[d_out])
    assert staged == 0 and idle == 0 and wrote.value == len(want)
    got = d_out.cpu().numpy()
    assert got[:len(want)].tobytes() == want, "the call read the stream before the default stream had written it"
    assert (got[len(want):] == S.CANARY).all()


def test_a_large_call_a_small_one_a_refused_one_and_reset(torch_cuda, bc, stream):
    """No position or piece of an earlier call carries over on a warm context."""
    rng = np.random.default_rng(14)
    large = cat([mix_records(rng, 3000, "alt", STREAM_BYTES), bytes_rec(0, 500000), bytes_rec(9, 1 << 20)])
    small = cat([bytes_rec(3, 2), chunk_rec(rng)])
    one_big = bytes_rec(77, 129)
    bad = bytes_rec(STREAM_BYTES, 1)
    host, dev = stream
    for _ in range(2):
        check(torch_cuda, bc, stream, large, "large")
        check(torch_cuda, bc, stream, small, "small")
        check(torch_cuda, bc, stream, one_big, "one piece")
        assert device_call(torch_cuda, bc, bad, dev, len(host))[0] == -1
        check(torch_cuda, bc, stream, small, "small after a refusal")
        check(torch_cuda, bc, stream, cat([]), "no records")
        assert bc.serialize_stats()["write_ms"] == 0  # no device work for no records
        bc.reset()
        check(torch_cuda, bc, stream, large, "large after reset")
    st = bc.serialize_stats()
    assert st["upload_ms"] > 0 and st["size_ms"] > 0 and st["write_ms"] > 0


def test_serialize_device_returns_a_buffer_of_its_own(torch_cuda, bc, stream):
    host, dev = stream
    rng = np.random.default_rng(15)
    recs = cat([chunk_rec(rng), bytes_rec(5, 1000), bytes_rec(0, 3)])
    ptr, n = bc.serialize_device(recs, dev.data_ptr(), len(host))
    try:
        assert bc._download(ptr, n) == expected(recs, host)
    finally:
        bc.free_device(ptr)
    ptr, n = bc.serialize_device(cat([]), dev.data_ptr(), len(host))
    assert n == 0
    bc.free_device(ptr)
    from zbackup_amd import ZcError
    with pytest.raises(ZcError, match="record 0: bytes"):
        bc.serialize_device(bytes_rec(STREAM_BYTES, 1), dev.data_ptr(), len(host))
