"""Sequences of streams on one warm context, against the oracle.

Every other chunking test makes a context, runs one stream (or two of about
one size) and drops it.  A context that lives on -- what bench.py measures and
a backup daemon would hold -- keeps state between streams: every device buffer
at the size of the largest stream so far, the epoch tables and the flag that
says they were left clear, the key arrays the scan writes, the historic index
and its reservation, the by-value seed set with its screen tables, the feed
window, and whether the last stream came through it.  Here one context runs
many streams of very different sizes through all four paths (device-resident,
zc_chunk_host from pinned memory, the feed through the smallest window, the
feed with window 0), with reset / forget_stream_chunks / seed_index between
them.  tests/seq_model.py keeps the context's index on the host and predicts
every stream with the oracle; every comparison is bit-exact.

zc_last_stream_paths (BackupCreator.last_paths()) says which form the first
epoch's index insert took.  The fused form (tables found clear, every grid key
from the scan) is the headline path of bench.py and runs only on a warm
context; test_fused_insert_* is its oracle comparison at the smallest shapes
that reach it.  A stream that reallocates an epoch table must never take it
(the new buffer holds anything): asserted after every stream here."""
import os

import numpy as np
import pytest

from oracle import oracle
from tests import seq_model as sm
from tests.seq_model import CLEARED, FUSED, REALLOC, SCAN_KEYS, STILE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    return torch


def _rand(n, seed):
    return oracle.splitmix64(n, seed)


class Context:
    """A BackupCreator and its model, stream after stream."""

    def __init__(self, torch, W, sha1, seeds=()):
        from zbackup_amd import BackupCreator
        self.torch = torch
        self.bc = BackupCreator(W, seeds=seeds, sha1=sha1)
        self.m = sm.ContextModel(W, sha1, seeds)
        self.ran = False
        self.win = None  # the window last set
        self.log = []

    def close(self):
        self.bc.close()

    def _window(self, want):
        if self.win != want:
            self.bc.set_window(want)
            self.win = want

    def _feed(self, data, path):
        torch, bc, n = self.torch, self.bc, int(data.size)
        if path == "device":
            t = torch.from_numpy(np.ascontiguousarray(data)).to("cuda") if n else None
            bc.chunk_device(t.data_ptr() if n else 0, n)
            torch.cuda.synchronize()
        elif path == "host":
            h = torch.from_numpy(np.ascontiguousarray(data)).pin_memory() if n else None
            bc.chunk_host(h.data_ptr() if n else 0, n)
        elif path == "window":  # ragged pieces through the smallest window (8 W + 16 MiB)
            self._window(1)
            rng = np.random.default_rng(n)
            pos = 0
            while pos < n:
                buf = bc.get_input_buffer()
                take = min(int(rng.integers(1, 3 << 20)), bc.get_input_buffer_size(), n - pos)
                np.frombuffer(buf, dtype=np.uint8, count=take)[:] = data[pos:pos + take]
                bc.handle_more_data(take)
                pos += take
            bc.finish()
        else:  # the whole stream kept in HBM and resolved at finish()
            assert path == "feed0"
            self._window(0)
            bc.feed(data)
            bc.finish()

    def run(self, data, path, recs=None, forget=False, extra=()):
        """The next stream of the context: reset() (always), forget / seed as
        asked, the stream through `path`, and every check that holds after any
        stream.  recs: the model's prediction when the caller has it already.
        Returns the stream's path bits."""
        bc, m, n = self.bc, self.m, int(data.size)
        if self.ran:
            bc.reset()
        self.ran = True
        if forget:
            bc.forget_stream_chunks()
            m.forget()
        if extra:
            bc.seed_index(extra)
            m.seed(extra)
        fused = m.fused(n, path)
        bits_needed = sm.table_bits(n, m.W)
        grows, fits = bits_needed > m.bits, bits_needed <= m.bits_sure
        if recs is None:
            recs = m.predict(data)
        self._feed(data, path)
        got, bits, st = bc.record_tuples(), bc.last_paths(), bc.stats()
        self.log.append(f"{path} n={n} forget={forget} seed_index={len(extra)} bits={bits:#x} "
                        f"predicted fused={fused} tables grow={grows}")
        m.commit(recs, n, path)
        assert got == m.expect(recs), self.log[-1]
        # a reallocated table holds anything: never the form that trusts it clear
        assert not (bits & REALLOC and bits & FUSED), self.log[-1]
        # the fused form runs exactly when the code's condition holds
        assert bool(bits & FUSED) == (fused and not bits & REALLOC), self.log[-1]
        if fused and fits:  # (tables as large were made by an earlier whole-stream epoch)
            assert bits & FUSED and not bits & REALLOC, self.log[-1]
        if grows and path != "window":  # (a window's epochs are sized by its segments)
            assert bits & REALLOC and bits & CLEARED, self.log[-1]
        if bits_needed and path != "window":  # (keys of the grid chunks inside the scanned full tiles)
            assert bool(bits & SCAN_KEYS) == (sm.in_scan_key_set(m.W) and n >= STILE), self.log[-1]
        if n < m.W:
            assert bits == 0, self.log[-1]  # (no chunk of size W: no index launch at all)
        # every W-byte chunk the streams saved is a historic entry, and nothing else
        assert st["hist_entries"] == m.count_added(), self.log[-1]
        assert st["bytes"] == n
        return bits


def test_last_paths_before_and_after_a_stream(torch_cuda):
    """ZC_ERR_STATE with a message until the context has finished a stream; the
    last stream's bits from then on, across reset() and while the next is fed."""
    import ctypes
    from zbackup_amd import BackupCreator, _lib
    data = _rand(5 * 4096 + 1, 7401)
    with BackupCreator(4096, sha1=False) as bc:
        bits = ctypes.c_uint32(0xABCD)
        assert bc._L.zc_last_stream_paths(bc._ctx, ctypes.byref(bits)) == _lib.ZC_ERR_STATE
        assert b"no stream" in bc._L.zc_last_error(bc._ctx) and bits.value == 0xABCD
        assert bc._L.zc_last_stream_paths(bc._ctx, None) == _lib.ZC_ERR_ARG
        with pytest.raises(_lib.ZcError, match="no stream"):
            bc.last_paths()
        bc.set_window(0)
        bc.feed(data)
        with pytest.raises(_lib.ZcError, match="no stream"):  # fed, not finished
            bc.last_paths()
        bc.finish()
        assert bc.last_paths() == REALLOC | CLEARED  # its first tables, cleared by the launch itself
        assert bc._L.zc_last_error(bc._ctx) == b""
        bc.reset()
        bc.feed(data[:100])
        assert bc.last_paths() == REALLOC | CLEARED
        bc.finish()
        assert bc.last_paths() == 0 and bc.record_tuples() == sm.strip_sha(oracle.chunk(data[:100], 4096))


# ---- B1: the fused index insert at its smallest shapes ---------------------

# launch_epoch_index is fused when (zc_kernels.hip, epoch_index_fused): the
# tables were left clear -- a later stream of the context -- no confirmed refs
# (the first epoch), and every grid key came from the scan: W in the scan-key
# set (a multiple of 4 KiB dividing 256 KiB) and n mod 2 MiB < W.  12288 is a
# multiple of the 4 KiB lane span but does not divide the 256 KiB wave-tile
# (scan_key_lshift_or_none), so its grid keys come from the metadata kernel
# and its first epoch never fuses; nothing else (a historic index, seeds,
# ZC_FLAG_SHA1) enters the condition.
FUSED_ON_WARM = {4096: True, 12288: False, 65536: True, 262144: True}


def _stream_b(W, a, n):
    parts = [_rand((1 << 20) + 333, 7001)]
    parts.append(parts[0][12345:12345 + 2 * W + 777])              # its own range, off the grid
    parts.append(np.zeros(2 * W + 4099, dtype=np.uint8))          # a zero run longer than 2 W
    parts.append(a[W + 17:W + 17 + 3 * W + 55])                    # a range of stream A
    used = sum(p.size for p in parts)
    parts.append(_rand(n - used, 7002))
    b = np.concatenate(parts)
    assert b.size == n
    return b


@pytest.mark.parametrize("sha1", [True, False])
@pytest.mark.parametrize("W", sorted(FUSED_ON_WARM))
def test_fused_insert_on_a_warm_context(torch_cuda, W, sha1):
    a = np.concatenate([_rand(3 * STILE // 2, 7003), np.zeros(W + 5, dtype=np.uint8),
                        _rand(2 * STILE + 700001 - 3 * STILE // 2 - W - 5, 7004)])
    assert a.size == 2 * STILE + 700001 and a.size % STILE >= 2 * W  # a partial tile of two chunks or more
    b0 = _stream_b(W, a, 3 * STILE)
    b1 = np.concatenate([b0, _rand(W - 1, 7005)])
    ctx = Context(torch_cuda, W, sha1)
    try:
        bits_a = ctx.run(a, "device")
        assert not bits_a & FUSED and bits_a & REALLOC and bits_a & CLEARED  # the context's first stream
        for b in (b0, b1):
            # the condition, restated: a later stream, W in the scan-key set, n mod 2 MiB < W, tables clear
            want_fused = ctx.m.tables and sm.in_scan_key_set(W) and b.size % STILE < W
            assert want_fused == FUSED_ON_WARM[W] == ctx.m.fused(b.size, "device")
            recs = ctx.m.predict(b)
            if sha1:  # the range of A is found through the carried index: two whole chunks of A's grid
                at = (1 << 20) + 333 + 2 * W + 777 + 2 * W + 4099
                assert ((recs["kind"] == 1) & (recs["offset"] >= at) & (recs["offset"] < at + 3 * W + 55)).sum() >= 2
            bits = ctx.run(b, "device", recs)
            assert not bits & REALLOC  # (A's tables are large enough)
            assert bool(bits & FUSED) == FUSED_ON_WARM[W], hex(bits)
            # (fused or not, a later epoch of the stream -- after a match moved
            # the grid -- clears the tables itself, so both bits may be set)
            assert bits & (FUSED | CLEARED), hex(bits)
        # A again, now warm: its partial tile holds grid chunks the scan wrote no
        # key for (key_from < nsref), so the tables being clear is not enough
        bits = ctx.run(a, "device")
        assert not bits & FUSED and bits & CLEARED and bool(bits & SCAN_KEYS) == sm.in_scan_key_set(W)
        warm_b = None
        if not sha1:
            warm_b = ctx.m.expect(ctx.m.predict(b0))
    finally:
        ctx.close()
    # B on a fresh context: not fused, and (no carried index to differ) the same records
    fresh = Context(torch_cuda, W, sha1)
    try:
        recs = fresh.m.predict(b0)
        bits = fresh.run(b0, "device", recs)
        assert not bits & FUSED and bits & CLEARED
        if warm_b is not None:
            assert fresh.m.expect(recs) == warm_b
    finally:
        fresh.close()


@pytest.mark.parametrize("path", ["device", "host", "feed0"])
def test_small_stream_then_large_one_reallocates_and_does_not_fuse(torch_cuda, path):
    """The open finding this file closes: a small stream leaves small tables,
    clear; the next stream, with nothing allocated in between, needs larger
    ones and meets every other condition of the fused form (W = 4096, whole
    tiles).  The larger buffers may come back at the old addresses, so only
    the allocation itself can say that they hold anything."""
    W = 4096
    small = _rand(70000, 7101)
    large = np.concatenate([_rand(3 * STILE, 7102), small[1000:1000 + 3 * W], _rand(STILE - 3 * W, 7103)])
    ctx = Context(torch_cuda, W, True)
    try:
        ctx.run(small, path)
        assert ctx.m.fused(large.size, path)  # all of the condition but the tables' size
        bits = ctx.run(large, path)
        assert bits & REALLOC and bits & CLEARED and not bits & FUSED
        bits = ctx.run(large, path)  # and once they are large enough
        assert bits & FUSED and not bits & REALLOC
    finally:
        ctx.close()


@pytest.mark.parametrize("path", ["device", "window"])
def test_id_seeded_after_a_stream_added_it_survives_forget(torch_cuda, path):
    """Found by the sequence fuzz (plan 8): zc_seed_index of an id that one of
    the context's streams had added already -- here an all-zero chunk, which
    has no anchor and is kept by value, and a random chunk, kept in the
    historic index -- left the by-value entry marked as the stream's, and
    zc_forget_stream_chunks dropped a seeded id."""
    W = 4096
    a = np.concatenate([_rand(3 * W, 7301), np.zeros(3 * W, dtype=np.uint8), _rand(W + 9, 7302)])
    ids = [sm.chunk_id(np.zeros(W, dtype=np.uint8)), sm.chunk_id(a[W:2 * W])]
    b = _rand(5 * W, 7303)
    c = np.concatenate([_rand(35, 7304), np.zeros(2 * W + 1, dtype=np.uint8), _rand(777, 7305), a[W:2 * W],
                        _rand(2 * W, 7306)])
    ctx = Context(torch_cuda, W, True)
    try:
        ctx.run(a, path)
        assert ctx.bc.stats()["by_value"] == 1  # the zero chunk
        ctx.run(b, path, extra=ids)
        recs = ctx.m.predict(c, carried=False)
        assert (recs["kind"] == 1).sum() >= 3 and tuple(recs[0])[:3] == (0, 35, 2)  # B 35, then the zero chunk
        ctx.run(c, path, recs, forget=True)
        assert ctx.bc.stats()["by_value"] == 2
    finally:
        ctx.close()


# ---- B2: grow, shrink, grow ------------------------------------------------

_GROW = {}


def _grow_streams(W):
    """The eight streams for W (made once): random bytes with ranges of the
    stream before them at odd offsets; the 12 MiB one also a 1 MiB zero run."""
    if W in _GROW:
        return _GROW[W]
    sizes = [70000, (8 << 20) + 5, 1, 0, W - 1, 2 << 20, 12 << 20, 300000]
    out, prev = [], np.zeros(0, dtype=np.uint8)
    for k, n in enumerate(sizes):
        d = _rand(n, 7200 + 16 * W + k)
        last = [p for p in out if p.size >= 3 * W]  # (the 1- and 0-byte streams have nothing to copy)
        src = prev if prev.size >= 3 * W or not last else last[-1]
        pos = 4321
        for j in range(3):
            ln = min(src.size, 3 * W + 100 + 17 * j)
            if ln and pos + ln <= n:
                off = (src.size - ln) * j // 3
                d[pos:pos + ln] = src[off:off + ln]
            pos += max(n // 3, 1) + 7
        if n == 12 << 20:
            d[(5 << 20) + 11:(6 << 20) + 11] = 0
        out.append(d)
        prev = d
    _GROW[W] = out
    return out


_GROW_RECS = {}


def _grow_recs(W, sha1):
    """The model's records of the eight streams (once per W and mode: the path
    a stream takes does not change what it must report)."""
    if (W, sha1) not in _GROW_RECS:
        m, recs = sm.ContextModel(W, sha1), []
        for d in _grow_streams(W):
            r = m.predict(d)
            m.commit(r, d.size, "device")
            recs.append(r)
        if sha1:  # the streams do find the stream before them
            assert sum(1 for r in recs[1:] if (r["kind"] == 1).any()) >= 4
        _GROW_RECS[(W, sha1)] = recs
    return _GROW_RECS[(W, sha1)]


@pytest.mark.parametrize("path", sm.PATHS)
@pytest.mark.parametrize("sha1", [True, False])
@pytest.mark.parametrize("W", [256, 4096, 65536])
def test_grow_shrink_grow(torch_cuda, W, sha1, path):
    streams, recs = _grow_streams(W), _grow_recs(W, sha1)
    assert streams[6].size // W >= 64 * (streams[0].size // W)  # (180-fold the first stream's refs at W = 256)
    ctx = Context(torch_cuda, W, sha1)
    try:
        seen = [ctx.run(d, path, r) for d, r in zip(streams, recs)]
    finally:
        ctx.close()
    # the large stream right after the small one, nothing allocated in between
    if path != "window":
        assert seen[1] & REALLOC and not seen[1] & FUSED, ctx.log
        if sm.in_scan_key_set(W):  # 2 MiB exactly, on tables the 8 MiB stream left: fused
            assert seen[5] & FUSED, ctx.log
        # 12 MiB: larger tables again at W = 256 and 4096; at 65536 the 8 MiB stream's do, and it is fused
        big = sm.table_bits(streams[6].size, W) > sm.table_bits(streams[1].size, W)
        assert big == (W != 65536) and bool(seen[6] & REALLOC) == big and bool(seen[6] & FUSED) == (not big), ctx.log
    assert seen[2] == seen[3] == seen[4] == 0, ctx.log


# ---- B3: seeded sequence fuzz ----------------------------------------------

# ZC_SEQ_SEEDS / ZC_SEQ_BASE widen or move the sweep (a longer run by hand)
@pytest.mark.parametrize("seed", range(int(os.environ.get("ZC_SEQ_SEEDS", "32"))))
def test_sequence_fuzz(torch_cuda, seed):
    seed += int(os.environ.get("ZC_SEQ_BASE", "0"))
    plan, out = sm.make_plan(seed), sm.plan_records(seed)
    ctx = Context(torch_cuda, plan["W"], plan["sha1"], plan["seeds"])
    try:
        for i, (st, o) in enumerate(zip(plan["steps"], out)):
            bits = ctx.run(st["data"], st["path"], o["recs"], st["forget"], st["extra"])
            assert ctx.m.count_added() == o["added"]
            if o["fused"] and not o["grows"] and o["fits"]:
                assert bits & FUSED
    except BaseException:
        print(sm.describe(plan))
        print(f"failed at step {i}; the steps as run:")
        print("\n".join(f"  {j}: {line}" for j, line in enumerate(ctx.log)))
        raise
    finally:
        ctx.close()
