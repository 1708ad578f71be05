"""GPU parity with the reference's own BackupCreator and ChunkIndex.

The fixtures read here were written by oracle/_ref/zbc_ref_cli, which compiles
backup_creator.cc and chunk_index.cc of the reference unmodified
(tests/golden/make_golden.py): tests/golden/refbc_corpus (100 recorded fuzz
streams) and the directed cases tests/golden/rp_*.txt (one named edge each:
stream lengths around W, matches on the last byte, the 128-byte rule, the finish
split, refused adds, same-key chains, odd seeds).  No test here reads the
reference or the restated oracle's verdict: the expected records are the
fixture's, and every comparison is exact -- kind, offset, size, rolling hash and
SHA-1 prefix.

A NEW record is a Writer::add call, not an added chunk: the reference calls add
for a chunk whose id the index already holds and add returns false (the X lines
of a fixture).  The engine must report such a chunk as NEW, not as a duplicate.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import golden_io, refpin_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(HERE, "adapter", "adapter_main")


def _load():
    groups = {}
    for p in refpin_cases.corpus_paths():
        with open(p) as f:
            groups["corpus_" + os.path.basename(p)[:-4]] = refpin_cases.parse_cases(f.read())
    directed = [golden_io.load_case(refpin_cases.fixture_path(n)) for n in refpin_cases.DIRECTED_NAMES
                if n not in refpin_cases.DIVERGENT_NAMES]
    for k in range(0, len(directed), 25):
        groups[f"directed_{k // 25}"] = directed[k:k + 25]
    return groups


GROUPS = _load()
ALL = [c for g in GROUPS.values() for c in g]
BY_NAME = {c[0]["case"]: c for c in ALL}
REFUSED = [c[0]["case"] for c in ALL if c[0]["refused"]]
PATHS = ["device", "feed_cap", "feed_ragged", "window"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    return torch


def test_the_fixtures_are_there():
    assert sum(len(g) for k, g in GROUPS.items() if k.startswith("corpus_")) == 100
    assert len(ALL) == 100 + len(refpin_cases.DIRECTED) - len(refpin_cases.DIVERGENT_NAMES) and len(BY_NAME) == len(ALL)
    assert len(refpin_cases.DIVERGENT_NAMES) == 2
    assert len(REFUSED) >= 15
    assert all("zbc_ref_cli" in m["generator"] for m, _, _ in ALL)


def _to_device(torch, data):
    if not data.size:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.ascontiguousarray(data)).to("cuda")


def _feed(bc, data, piece):
    """The zero-copy contract of zutils.cc:100-124; piece(room) gives the size of the next piece."""
    pos = 0
    while pos < data.size:
        buf = bc.get_input_buffer()
        take = min(piece(bc.get_input_buffer_size()), bc.get_input_buffer_size(), data.size - pos)
        np.frombuffer(buf, dtype=np.uint8, count=take)[:] = data[pos:pos + take]
        bc.handle_more_data(take)
        pos += take
    bc.finish()


def _run(torch, meta, data, path, seed=None):
    """The records of one stream through one entry point; seed(bc) seeds the fresh context."""
    from zbackup_amd import BackupCreator
    W = meta["W"]
    window = {"device": None, "feed_cap": 0, "feed_ragged": 0, "window": 1}[path]
    with BackupCreator(W, window=window) as bc:
        if seed is not None:
            seed(bc)
        if path == "device":
            t = _to_device(torch, data)
            bc.chunk_device(t.data_ptr(), data.size)
        elif path == "feed_cap":
            cap = meta["feed_max"]
            _feed(bc, data, lambda room: cap or room)
        else:
            rng = np.random.default_rng(data.size + W)
            top = max(2, min(3 * W, data.size // 3 + 2))
            _feed(bc, data, lambda room: int(rng.integers(1, top)))
        return bc.record_tuples()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_records_equal_the_reference_built_chunker(torch_cuda, group, path):
    """Every corpus stream and every directed case through one entry point, seeded by value."""
    for meta, seeds, want in GROUPS[group]:
        data = oracle.gen(meta["spec"])
        assert data.size == meta["n"]
        got = _run(torch_cuda, meta, data, path, lambda bc: bc.seed_index(seeds))
        assert got == want, (meta["case"], path)


def _seed_windows(meta, data, seeds):
    """Offsets of the W-byte windows of the stream whose true ids are among the seeds."""
    name, W = meta["case"], meta["W"]
    if name.startswith("fuzz"):
        i = int(name[4:]) - 5000
        offs = refpin_cases.fuzz_case(i, offsets=True)[2]
        assert refpin_cases.fuzz_case(i)[2] == seeds  # the recorded seeds are these windows' ids
        return offs
    desc = next(c[3] for c in refpin_cases.DIRECTED if c[0] == name)
    assert refpin_cases.build_seeds(data, W, desc) == seeds
    return [d[1] for d in desc if d[0] == "win" or (d[0] == "sized" and d[2] == W)]


SEEDED = [c[0]["case"] for c in ALL if c[1]]
SEEDED_PARTS = {f"part{k}": SEEDED[k::4] for k in range(4)}


@pytest.mark.parametrize("part", sorted(SEEDED_PARTS))
def test_seeds_with_anchor_metadata(torch_cuda, part):
    """The seeded cases again with their seeds given through seed_index_meta: the
    metadata of each seed that is a window of the stream comes from a context that
    saved that window as a chunk (export_chunk_meta); ids without metadata (another
    id under the same key, a sub-W chunk, W < 128) go by value in the same call."""
    from zbackup_amd import BackupCreator
    joined = 0
    for name in SEEDED_PARTS[part]:
        meta, seeds, want = BY_NAME[name]
        W = meta["W"]
        data = oracle.gen(meta["spec"])
        with BackupCreator(W) as bc:
            for off in _seed_windows(meta, data, seeds):
                t = _to_device(torch_cuda, data[off:off + W])
                bc.chunk_device(t.data_ptr(), W)
                bc.reset()
            cmeta = bc.export_chunk_meta()
        sha = np.frombuffer(b"".join(s[0] for s in seeds), dtype=np.uint8).reshape(-1, 16)
        rolling = np.array([s[1] for s in seeds], dtype=np.uint64)
        size = np.array([s[2] for s in seeds], dtype=np.uint32)
        stats = {}

        def seed(bc):
            bc.seed_index_meta(sha, rolling, size, cmeta)
            stats.update(bc.stats())
        for path in ("device", "window"):
            assert _run(torch_cuda, meta, data, path, seed) == want, (name, path)
        joined += stats["hist_seeded"]
    assert joined > 0  # some seeds did join the anchor-probed index


@pytest.mark.parametrize("order", ["true_first", "flip_first"])
@pytest.mark.parametrize("W", [256, 4097])
def test_same_key_chain_in_both_seed_orders(torch_cuda, W, order):
    """Two ids under one rolling key, the key of a real window: the window matches
    whichever of the two was registered first, in one seeding call or in two."""
    meta, seeds, want = BY_NAME[f"rp_w{W}_samekey_{order}"]
    assert len(seeds) == 2 and seeds[0][1] == seeds[1][1] and seeds[0][0] != seeds[1][0]
    assert [r[0] for r in want] == list("DBDNB") and want[0][3] == seeds[0][1]
    data = oracle.gen(meta["spec"])

    def two_calls(bc):
        bc.seed_index(seeds[:1])
        bc.seed_index(seeds[1:])
    for path in PATHS:
        assert _run(torch_cuda, meta, data, path, lambda bc: bc.seed_index(seeds)) == want, path
        assert _run(torch_cuda, meta, data, path, two_calls) == want, path
    # the wrong id alone never matches: the window is saved, and matched from then on
    meta, seeds, want = BY_NAME[f"rp_w{W}_samekey_flip_only"]
    assert [r[0] for r in want] == list("NBDNB")
    assert _run(torch_cuda, meta, data, "device", lambda bc: bc.seed_index(seeds)) == want


@pytest.mark.parametrize("path", PATHS + ["meta"])
@pytest.mark.parametrize("W", [256, 4097])
def test_a_seed_of_another_size_than_w_is_not_registered(torch_cuda, W, path):
    """The engine's one documented divergence (include/zchunk.h at zc_seed_index).  The
    index holds the first window's true id registered with size W - 1.  The
    reference matches it, since findChunk never reads the size: D B D N B
    (tests/golden/refpin_divergent).  The engine registers W-byte ids only: it
    chunks the stream as the reference does when the index cannot match that
    window -- the records of the same stream's flip_only fixture, N B D N B,
    which differ from the reference's verdict in the kind of the first record and
    in nothing else."""
    meta, seeds, ref = golden_io.load_case(refpin_cases.fixture_path(f"rp_w{W}_seed_size_not_w"))
    assert [s[2] for s in seeds] == [W - 1] and [r[0] for r in ref] == list("DBDNB")
    meta2, _, unmatched = BY_NAME[f"rp_w{W}_samekey_flip_only"]
    assert meta2["spec"] == meta["spec"] and [r[0] for r in unmatched] == list("NBDNB")
    assert unmatched[0] == ("N",) + ref[0][1:] and unmatched[1:] == ref[1:]
    data = oracle.gen(meta["spec"])
    stats = {}

    def seed(bc):
        if path == "meta":
            bc.seed_index_meta(np.frombuffer(seeds[0][0], dtype=np.uint8).reshape(1, 16),
                               np.array([seeds[0][1]], dtype=np.uint64), np.array([W - 1], dtype=np.uint32),
                               np.zeros(0, dtype=bc.export_chunk_meta().dtype))
        else:
            bc.seed_index(seeds)
        stats.update(bc.stats())
    assert _run(torch_cuda, meta, data, "device" if path == "meta" else path, seed) == unmatched
    assert stats["by_value"] == 0 and stats["hist_seeded"] == 0  # nothing registered: no per-byte screen


# --- refused adds ----------------------------------------------------------------

@pytest.mark.parametrize("name", REFUSED)
def test_a_refused_add_is_a_new_record(torch_cuda, name):
    from zbackup_amd import BackupCreator, chunk_id_blob
    meta, seeds, want = BY_NAME[name]
    data = oracle.gen(meta["spec"])
    got = _run(torch_cuda, meta, data, "device", lambda bc: bc.seed_index(seeds))
    for x in meta["refused"]:
        k, _, _, h, sha = got[x]
        assert k == "N"
        earlier = {(r[3], r[4]) for r in got[:x] if r[0] == "N"} | {(s[1], s[0].hex()) for s in seeds}
        assert (h, sha) in earlier
    assert got == want
    # backup_device hands every NEW record of the stream to on_new, the refused ones included
    # (on_new is called once a pass; pass 0 is this stream, the later ones the shrink loop's)
    news = []
    t = _to_device(torch_cuda, data)
    with BackupCreator(meta["W"], seeds=seeds) as bc:
        bc.backup_device(t.data_ptr(), data.size,
                         on_new=lambda recs, d, k: news.append((k, [chunk_id_blob(bytes(r["sha1"]), int(r["rolling"]))
                                                                    for r in recs])))
    assert [k for k, _ in news] == list(range(len(news)))  # each pass once: none of pass 0's records comes later
    assert news[0][1] == [chunk_id_blob(bytes.fromhex(r[4]), r[3]) for r in want if r[0] == "N"]
    for x in meta["refused"]:  # the refused add's id is among what the GPU run handed over, twice if a record came first
        blob = chunk_id_blob(bytes.fromhex(got[x][4]), got[x][3])
        earlier_new = sum(1 for r in got[:x] if r[0] == "N" and (r[3], r[4]) == (got[x][3], got[x][4]))
        assert news[0][1].count(blob) >= 1 + earlier_new


@pytest.mark.parametrize("name", ["rp_w4097_tail_twice", "rp_w256_tail_seeded"])
def test_adapter_calls_add_for_a_known_id(torch_cuda, tmp_path, name):
    """tests/adapter over the zutils.cc loops: Writer::add is called for the chunk
    whose id the index holds, a Writer that answers as the reference's does
    returns false there, and the backup data does not depend on the answer."""
    from zbackup_amd import chunk_id_blob
    if not os.path.exists(BIN):
        pytest.fail("tests/adapter/adapter_main not built (run __graft_entry__.build())")
    meta, seeds, want = BY_NAME[name]
    data = oracle.gen(meta["spec"])
    inp = tmp_path / "in.bin"
    data.tofile(inp)
    sf = "-"
    if seeds:
        sf = str(tmp_path / "seeds.bin")
        with open(sf, "wb") as f:
            for sha, h, s in seeds:
                f.write(sha + struct.pack("<QII", h, s, 0))
    runs = {}
    for mode in ("always_true", "reference"):
        out = str(tmp_path / mode)
        env = dict(os.environ)
        env.pop("ADAPTER_WRITER_ANSWERS", None)
        if mode == "reference":
            env["ADAPTER_WRITER_ANSWERS"] = "reference"
        r = subprocess.run([BIN, str(meta["W"]), str(inp), sf, out], capture_output=True, text=True, timeout=120,
                           env=env)
        assert r.returncode == 0, r.stderr
        runs[mode] = tuple(open(out + ext, "rb").read() for ext in (".data", ".adds", ".answers"))
    assert runs["always_true"][:2] == runs["reference"][:2]  # same backup data, same calls
    data_out, adds, answers = runs["reference"]
    first_pass = [(i, chunk_id_blob(bytes.fromhex(r[4]), r[3])) for i, r in enumerate(want) if r[0] == "N"]
    assert len(adds) == 24 * len(answers) and len(answers) >= len(first_pass)
    # the first pass's calls are the fixture's NEW records, answered as the reference answered them
    assert adds[:24 * len(first_pass)] == b"".join(b for _, b in first_pass)
    assert [bool(a) for a in answers[:len(first_pass)]] == [i not in meta["refused"] for i, _ in first_pass]
    assert not all(answers[:len(first_pass)])
    assert set(runs["always_true"][2]) == {1}
