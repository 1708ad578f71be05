"""GPU tests of the restore that stays in HBM: zc_restore_resolve_device against
zc_restore_resolve on one stream through both paths, zc_restore_replay against
a restore done with Python dicts, its refusals, and Restorer.restore_iterations
over synthetic repositories of 0 to 3 iterations."""
import ctypes
import lzma

import numpy as np
import pytest

from tests import resolve_cases as RC
from tests.instr_cases import ser

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = 0xEE
COUNTS = ("n_entries", "n_used", "length", "n_missing", "first_missing", "n_dup_used", "first_dup")


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


@pytest.fixture()
def restorer(comp):
    from zbackup_amd import Restorer
    with Restorer(ctx=comp._ctx) as r:
        yield r


def to_device(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data) or b"\0", dtype=np.uint8).copy()).to("cuda:0")


def make_index(comp, bundles):
    from zbackup_amd import ChunkIndex
    ids, sizes, first = RC.arrays(bundles)
    return ChunkIndex.from_arrays(ids, sizes, first, ctx=comp._ctx)


def stream_of(entries, seed=5):
    """The case's entries serialized: a chunk_to_emit per chunk entry, e[2] random bytes per bytes entry."""
    rng = np.random.default_rng(seed)
    return b"".join(ser(chunk_blob=e[1]) if e[0] == "chunk"
                    else ser(raw=rng.integers(0, 256, e[2], dtype=np.uint8).tobytes()) for e in entries)


def device_plan(torch, comp, restorer, cx, data):
    """(InstructionSet, DevicePlan) of data through the device path, nothing raised on a missing id."""
    from zbackup_amd.restore import DevicePlan
    t = to_device(torch, data)
    ins = restorer.parse_device(t.data_ptr(), len(data))
    handle = ctypes.c_void_p()
    rc = comp._L.zc_restore_resolve_device(comp._ctx, cx._live(), ins._live(), ctypes.byref(handle))
    assert rc == 0, comp._L.zc_last_error(comp._ctx)
    return t, ins, DevicePlan(comp._L, handle)


RESOLVE_CASES = [(f.__name__, f) for f in RC.SMALL] + [(f"scan_edge_{n}", (lambda n=n: RC.scan_edge(n)))
                                                       for n in RC.SCAN_EDGES]


@pytest.mark.parametrize("make", [m for _, m in RESOLVE_CASES], ids=[n for n, _ in RESOLVE_CASES])
def test_resolve_device_equals_resolve(torch_cuda, comp, restorer, monkeypatch, make):
    from zbackup_amd import parse_backup_data
    case = make()
    if case["bits"] is not None:
        monkeypatch.setenv("ZC_TEST_RESOLVE_BITS", str(case["bits"]))
    data = stream_of(case["entries"])
    with make_index(comp, case["bundles"]) as cx:
        want = cx.resolve(parse_backup_data(data), len(data))
        t, ins, got = device_plan(torch_cuda, comp, restorer, cx, data)
        with ins, got:
            assert ins.n_entries == want.n_entries == len(case["entries"])
            for name in COUNTS:
                assert getattr(got, name) == getattr(want, name), name
            for name in ("used", "used_size", "slot", "off", "size", "dst"):
                g, w = getattr(got, name), getattr(want, name)
                assert g.dtype == w.dtype and g.shape == w.shape, name
                if not np.array_equal(g, w):
                    at = int(np.nonzero(g != w)[0][0])
                    raise AssertionError(f"{name}[{at}] = {g[at]}, expected {w[at]}")
            n = want.n_entries
            some = range(n) if n <= 300 else [0, 1, n // 2, n - 2, n - 1] + list(range(255, n, n // 40))
            for e in some:
                assert got.entry(e) == (int(want.slot[e]), int(want.off[e]), int(want.size[e]), int(want.dst[e])), e
            with pytest.raises(Exception, match=f"entry {n} of {n}"):
                got.entry(n)


# ---- replay ----

SIZES = [0, 1, 15, 16, 17, 65535, 65536, 65537]
BYTES_RUN = 200000


def replay_repo():
    """Bundles whose chunks have the sizes above, and a stream over them: every
    size at every destination residue mod 16, one chunk 1,000 times, one
    bytes_to_emit of 200,000 bytes and short ones between."""
    rng = np.random.default_rng(77)
    ids = RC.rand_ids(rng, 2 * len(SIZES) + 1)
    chunks = {c: rng.integers(0, 256, s, dtype=np.uint8).tobytes() for c, s in zip(ids, SIZES + SIZES + [17])}
    order = list(chunks)
    bundles = [[(c, len(chunks[c])) for c in order[:5]], [], [(c, len(chunks[c])) for c in order[5:11]],
               [(c, len(chunks[c])) for c in order[11:]]]
    parts, want = [], []

    def chunk(c):
        parts.append(ser(chunk_blob=c))
        want.append(chunks[c])

    def raw(n):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        parts.append(ser(raw=b))
        want.append(b)

    for shift in range(16):  # after each round the destination has moved one residue on
        for c in order[:len(SIZES)]:
            chunk(c)
        raw(1 + (16 - sum(SIZES) % 16) % 16)
    raw(BYTES_RUN)
    for _ in range(1000):
        chunk(order[-1])  # 17 bytes: every residue again
    parts.append(ser(chunk_blob=order[9], raw=b"both"))
    want += [chunks[order[9]], b"both"]
    payloads = [b"".join(chunks[c] for c, _ in b) for b in bundles]
    data = b"".join(parts)
    sizes = [len(w) for w in want]
    residues = {(int(d) % 16, s) for d, s in zip(np.cumsum([0] + sizes[:-1]), sizes)}
    assert all((r, s) in residues for r in range(16) for s in SIZES[1:])
    return bundles, payloads, data, b"".join(want)


def guarded(torch, n):
    return torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda:0")


def host_plan(comp, cx, data):
    from zbackup_amd import parse_backup_data
    ins = parse_backup_data(data)
    handle = ctypes.c_void_p()
    rc = comp._L.zc_restore_resolve(comp._ctx, cx._live(), ins.ctypes.data if len(ins) else None, len(ins), len(data),
                                    ctypes.byref(handle))
    assert rc == 0
    return handle


def test_replay_equals_a_dict_restore(torch_cuda, comp, restorer):
    from zbackup_amd.restore import DevicePlan
    bundles, payloads, data, want = replay_repo()
    with make_index(comp, bundles) as cx:
        t, ins, plan = device_plan(torch_cuda, comp, restorer, cx, data)
        hplan = DevicePlan(comp._L, host_plan(comp, cx, data))
        with ins, plan, hplan:
            assert plan.length == hplan.length == len(want) and plan.n_missing == 0
            assert [int(b) for b in plan.used] == [0, 2, 3]  # bundle 1 is empty
            pays = [to_device(torch_cuda, payloads[int(b)]) for b in plan.used]
            ptrs = [p.data_ptr() for p in pays] + [t.data_ptr()]
            for which in (plan, hplan, hplan, plan):  # a host-made plan's second replay reuses its uploaded lists
                out = guarded(torch_cuda, len(want))
                assert restorer.replay_device(which, ptrs, out.data_ptr() + GUARD, len(want)) == len(want)
                got = out.cpu().numpy()
                assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all()
                assert got[GUARD:-GUARD].tobytes() == want


def test_replay_refusals_leave_the_output_untouched(torch_cuda, comp, restorer):
    from zbackup_amd import _lib
    bundles, payloads, data, want = replay_repo()
    L, ctx = comp._L, comp._ctx
    out = guarded(torch_cuda, len(want))

    def refused(plan, ptrs, cap, text):
        with pytest.raises(_lib.ZcError, match=text):
            restorer.replay_device(plan, ptrs, out.data_ptr() + GUARD, cap)
        assert L.zc_last_error(ctx).decode().startswith("zc_restore_replay: ")
        assert bool((out == CANARY).all())

    with make_index(comp, bundles) as cx:
        t, ins, plan = device_plan(torch_cuda, comp, restorer, cx, data)
        with ins, plan:
            pays = [to_device(torch_cuda, payloads[int(b)]) for b in plan.used]
            ptrs = [p.data_ptr() for p in pays] + [t.data_ptr()]
            refused(plan, ptrs, len(want) - 1, f"{len(want)} bytes to restore, room for {len(want) - 1}")
            refused(plan, ptrs[:1] + [None] + ptrs[2:], len(want), r"slot 1 \(bundle 2\) has no payload")
            refused(plan, ptrs[:-1] + [None], len(want), "the instruction stream's slot is null")
            refused(plan, ptrs[:-1], len(want), "3 slots, the plan has 3 used bundles and the instruction stream")
            refused(plan, ptrs + ptrs[:1], len(want), "5 slots, the plan has 3 used bundles")
        # a missing id
        rng = np.random.default_rng(3)
        gone = ser(chunk_blob=RC.rand_ids(rng, 1)[0])
        t2, ins2, plan2 = device_plan(torch_cuda, comp, restorer, cx, data[:27] + gone + data[27:])
        with ins2, plan2:
            assert (plan2.n_missing, plan2.first_missing) == (1, 1)
            refused(plan2, ptrs[:-1] + [t2.data_ptr()], len(want), "1 entries whose chunk id is missing")
    # a used bundle that holds an id twice
    case = RC.dup_used()
    data = stream_of(case["entries"])
    with make_index(comp, case["bundles"]) as cx:
        t, ins, plan = device_plan(torch_cuda, comp, restorer, cx, data)
        with ins, plan:
            assert plan.n_dup_used == case["n_dup_used"]
            ptrs = [out.data_ptr()] * plan.n_used + [t.data_ptr()]
            refused(plan, ptrs, 1 << 20, "uses a bundle that holds a chunk id twice")


# ---- iterations ----

USER_BYTES = 300000


class Repo:
    """A synthetic repository: bundles of (id, size) records with their
    payloads, and streams[k] = the instruction stream of iteration k
    (streams[0] restores to the user data, streams[k + 1] to streams[k])."""

    def __init__(self, iterations, seed=9):
        self.rng = np.random.default_rng(seed)
        self.bundles, self.payloads, self._next = [], [], 0
        self.user = self.rng.integers(0, 256, USER_BYTES, dtype=np.uint8).tobytes()
        self.shared = self.new_bundle()  # holds chunks of the user data and of streams[0]
        self.streams = [self.backup(self.user, mean=1500, shared_share=0.2)]
        for k in range(iterations):  # ever shorter chunks, so that every stream has more than a few entries
            self.streams.append(self.backup(self.streams[-1], mean=(300, 60, 40)[min(k, 2)],
                                            shared_share=0.3 if k == 0 else 0))

    def new_bundle(self):
        self.bundles.append([])
        self.payloads.append(b"")
        return len(self.bundles) - 1

    def backup(self, data, mean, shared_share):
        """data cut at arbitrary points into chunks and byte runs; the chunks go to fresh bundles (and
        some to the shared one); returns the stream that restores to data."""
        rng, parts, pos = self.rng, [], 0
        cur = self.new_bundle()
        while pos < len(data):
            n = min(len(data) - pos, int(rng.integers(1, 2 * mean)))
            piece = data[pos:pos + n]
            pos += n
            if rng.random() < 0.25:
                parts.append(ser(raw=piece[:min(n, 40)]))  # a byte run; the rest of the piece becomes a chunk
                piece = piece[min(n, 40):]
                if not piece:
                    continue
            self._next += 1
            cid = self._next.to_bytes(8, "little") + rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            if len(self.bundles[cur]) >= 12:
                cur = self.new_bundle()
            b = self.shared if rng.random() < shared_share else cur
            self.bundles[b].append((cid, len(piece)))
            self.payloads[b] += piece
            parts.append(ser(chunk_blob=cid))
        return b"".join(parts)


@pytest.fixture(scope="module")
def repo3():
    return Repo(3)


def test_synthetic_repository_is_what_it_claims(repo3):
    """By the host parser and Python dicts alone: streams[k + 1] restores to streams[k], the shared
    bundle serves two iterations."""
    from zbackup_amd import parse_backup_data
    from zbackup_amd.restore import chunk_map
    cmap = chunk_map(repo3.bundles)
    users = []
    want = [repo3.user] + repo3.streams
    for k, s in enumerate(repo3.streams):
        out, used = [], set()
        for e in parse_backup_data(s):
            if e["kind"] == 0:
                b, off, size = cmap[e["id"].tobytes()]
                used.add(b)
                out.append(repo3.payloads[b][off:off + size])
            else:
                out.append(s[int(e["data_off"]):int(e["data_off"]) + int(e["size"])])
        assert b"".join(out) == want[k]
        users.append(used)
    assert len(repo3.user) == USER_BYTES and len(repo3.streams) == 4
    assert [k for k, u in enumerate(users) if repo3.shared in u] == [0, 1]


def counted(monkeypatch, L, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(L, n)

        def wrapper(*a, _real=real, _n=n):
            calls[_n] += 1
            return _real(*a)
        monkeypatch.setattr(L, n, wrapper, raising=True)
    return calls


@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_restore_iterations_with_plain_pointers(torch_cuda, comp, restorer, monkeypatch, iterations):
    repo = Repo(iterations)
    pays = [to_device(torch_cuda, p) for p in repo.payloads]
    asked = []

    def payloads(used, used_size):
        asked.append([int(b) for b in used])
        assert [int(s) for s in used_size] == [len(repo.payloads[int(b)]) for b in used]
        return [pays[int(b)].data_ptr() for b in used]

    with make_index(comp, repo.bundles) as cx:
        calls = counted(monkeypatch, comp._L, ["zc_instr_set_fetch", "zc_restore_plan_fetch", "zc_restore_plan_entry",
                                               "zc_parse_instructions", "zc_restore_resolve", "zc_bundle_scatter",
                                               "zc_parse_instructions_device", "zc_restore_replay"])
        d_out, n = restorer.restore_iterations(repo.streams[-1], iterations, cx, payloads, USER_BYTES)
        seen = dict(calls)
        try:
            assert n == USER_BYTES and len(asked) == iterations + 1
            got = fetch_bytes(torch_cuda, comp, d_out, n)
        finally:
            restorer.free(d_out)
        assert got == repo.user
        # nothing per entry crossed to the host, and the host path was not taken
        assert seen["zc_parse_instructions_device"] == seen["zc_restore_replay"] == iterations + 1
        for name in ("zc_instr_set_fetch", "zc_restore_plan_fetch", "zc_restore_plan_entry", "zc_parse_instructions",
                     "zc_restore_resolve", "zc_bundle_scatter"):
            assert seen[name] == 0, name


def fetch_bytes(torch, comp, d_ptr, n):
    """n bytes of device memory to the host: one device copy into a tensor, then the tensor's."""
    t = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda:0")
    if n:
        comp.scatter(d_ptr, [0], [n], t.data_ptr(), [0])
    return t.cpu().numpy()[:n].tobytes()


def test_restore_iterations_from_xz_bodies(torch_cuda, comp, restorer, repo3, monkeypatch):
    """The three-iteration repository from its bundles' xz bodies: the bytes, the shared bundle decoded
    once, and no per-entry array fetched."""
    from zbackup_amd import XzBodiesPayloads
    bodies = {b: lzma.compress(p, check=lzma.CHECK_CRC64, preset=6) for b, p in enumerate(repo3.payloads)}
    with make_index(comp, repo3.bundles) as cx, XzBodiesPayloads(bodies, ctx=comp._ctx) as provider:
        asked = []

        def payloads(used, used_size):
            asked.extend(int(b) for b in used)
            return provider(used, used_size)

        calls = counted(monkeypatch, comp._L, ["zc_instr_set_fetch", "zc_restore_plan_fetch", "zc_xz_decode"])
        d_out, n = restorer.restore_iterations(repo3.streams[-1], 3, cx, payloads, USER_BYTES)
        try:
            assert fetch_bytes(torch_cuda, comp, d_out, n) == repo3.user
        finally:
            restorer.free(d_out)
        assert asked.count(repo3.shared) == 2  # two rounds use the shared bundle
        assert provider.decodes == len(set(asked)) < len(asked)  # each bundle decoded once
        assert calls["zc_xz_decode"] == 4 and calls["zc_instr_set_fetch"] == calls["zc_restore_plan_fetch"] == 0


def test_restore_iterations_names_a_missing_chunk(torch_cuda, comp, restorer, repo3):
    """streams[1] with one more instruction, whose chunk no bundle holds: the round that parses it raises
    with that id."""
    from zbackup_amd import _lib
    gone = bytes(range(200, 224))
    pays = [to_device(torch_cuda, p) for p in repo3.payloads]
    with make_index(comp, repo3.bundles) as cx:
        with pytest.raises(_lib.ZcError, match=f"restore: chunk id {gone.hex()} is in none of the "
                                               f"{len(repo3.bundles)} bundles"):
            restorer.restore_iterations(repo3.streams[1] + ser(chunk_blob=gone), 1, cx,
                                        lambda used, size: [pays[int(b)].data_ptr() for b in used], 1 << 20)
