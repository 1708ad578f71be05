"""The inputs of the chunk-index tests (test infrastructure only): each case is
{"name", "bundles", "entries", "data_len", "bits", ...claims}, bundles and
entries in tests/resolve_ref.py's form; `bits` is the ZC_TEST_RESOLVE_BITS the
case wants (None: the default tables).  tests/test_resolve.py checks that the
cases are what they claim to be; tests/test_gpu_resolve.py runs them.  The slot
hash is restated here from zc_gc_core.h so that colliding ids can be built:
id_fold is a xor of rotations."""
import numpy as np

M64 = (1 << 64) - 1
SCAN_EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 65537]
SHAPE_COUNTS = [0, 1, 64, 65, 5000, 0, 3]
COLLIDE_BITS, COLLIDE_N, COLLIDE_START, FOREIGN_N = 6, 40, 58, 8


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def words(blob):
    return [int.from_bytes(blob[8 * k:8 * k + 8], "little") for k in range(3)]


def id_fold(blob):
    w = words(blob)
    return w[0] ^ rotl(w[1], 21) ^ rotl(w[2], 42)


def mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ x >> 33


def slot_hash(blob, mask):
    return (mix64(id_fold(blob)) >> 20) & mask


def rand_ids(rng, n):
    raw = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    return [raw[i].tobytes() for i in range(n)]


def ids_with_fold(rng, n, fold):
    """n distinct ids whose id_fold is `fold`: they share every slot hash."""
    out = []
    for _ in range(n):
        w1, w2 = (int(x) for x in rng.integers(0, 1 << 63, 2))
        w0 = fold ^ rotl(w1, 21) ^ rotl(w2, 42)
        out.append(b"".join(w.to_bytes(8, "little") for w in (w0, w1, w2)))
    assert len(set(out)) == n
    return out


def entries_for(rng, ids, n, data_len, bytes_share=0.2):
    """n entries: chunks drawn from ids, and bytes runs inside data_len."""
    out = []
    for _ in range(n):
        if not ids or rng.random() < bytes_share:
            off = int(rng.integers(0, data_len + 1))
            out.append(("bytes", off, int(rng.integers(0, min(40, data_len - off) + 1))))
        else:
            out.append(("chunk", ids[int(rng.integers(0, len(ids)))]))
    return out


def split(rng, recs, max_records):
    """recs cut into bundles of 0..max_records records."""
    bundles, at = [], 0
    while at < len(recs):
        k = int(rng.integers(0, max_records + 1))
        bundles.append(recs[at:at + k])
        at += k
    return bundles


def case(name, bundles, entries, data_len=1000, bits=None, **claims):
    return dict(name=name, bundles=bundles, entries=entries, data_len=data_len, bits=bits, **claims)


def scan_edge(n):
    """n records and n entries, a tenth of the ids held by two bundles."""
    rng = np.random.default_rng(1000 + n)
    distinct = n - n // 10
    ids = rand_ids(rng, distinct)
    recs = [(c, int(s)) for c, s in zip(ids, rng.integers(0, 70000, distinct))]
    recs += [recs[int(j)] for j in rng.integers(0, max(distinct, 1), n // 10)]
    recs = [recs[int(j)] for j in rng.permutation(n)]
    bundles = split(rng, recs, 9 if n < 1000 else 700)
    # an id may fall twice into one bundle: the flag is then part of the answer
    return case(f"scan_edge_{n}", bundles, entries_for(rng, [c for c, _ in recs], n, 1000), n_records=n, n_entries=n)


def shapes():
    rng = np.random.default_rng(7)
    bundles = []
    for k in SHAPE_COUNTS:
        ids = rand_ids(rng, k)
        bundles.append([(c, int(s)) for c, s in zip(ids, rng.integers(1, 70000, k))])
    ids = [c for b in bundles for c, _ in b]
    return case("bundle_shapes", bundles, entries_for(rng, ids, 700, 1000), shape_counts=SHAPE_COUNTS)


def collisions():
    """COLLIDE_N ids with one slot hash that starts COLLIDE_START of a
    2^COLLIDE_BITS table, and FOREIGN_N ids of other hashes whose slots lie in
    the run the group takes: every probe run of the group's tail wraps the
    table's end and passes over foreign owners."""
    rng = np.random.default_rng(11)
    mask = (1 << COLLIDE_BITS) - 1
    fold = next(f for f in (int(x) for x in rng.integers(0, 1 << 63, 100000))
                if slot_hash(f.to_bytes(8, "little") + bytes(16), mask) == COLLIDE_START)
    group = ids_with_fold(rng, COLLIDE_N, fold)
    run = {(COLLIDE_START + k) & mask for k in range(COLLIDE_N)}
    foreign = []
    while len(foreign) < FOREIGN_N:
        c = rand_ids(rng, 1)[0]
        if slot_hash(c, mask) in run and id_fold(c) != fold:
            foreign.append(c)
    ids = group + foreign
    order = rng.permutation(len(ids))
    recs = [(ids[int(j)], 10 + int(j)) for j in order]
    bundles = split(rng, recs, 9)
    strangers = ids_with_fold(rng, 5, fold)  # the same hash, not in the index: the walk ends at a free slot
    entries = [("chunk", c) for c in ids + strangers] + [("bytes", 0, 9)]
    return case("collisions", bundles, entries, bits=COLLIDE_BITS, group=group, foreign=foreign, strangers=strangers,
                min_probe=COLLIDE_N)


def owners():
    rng = np.random.default_rng(13)
    x, y, p, q, r = rand_ids(rng, 5)
    bundles = [[(p, 11)], [(q, 3), (x, 100)], [(y, 200), (r, 1)], [(x, 100)], [(y, 200)], [(y, 200), (p, 11)],
               [(y, 200)], [(q, 3), (y, 200)]]
    return case("owners_2_and_5", bundles, [("chunk", c) for c in (y, x, p, q, r, y)], in_two=x, in_five=y,
                owner_of_two=1, owner_of_five=2)


def dup_unused():
    rng = np.random.default_rng(17)
    a, b, c = rand_ids(rng, 3)
    bundles = [[(a, 5), (b, 6)], [(c, 7), (c, 7)]]
    return case("dup_unused_bundle", bundles, [("chunk", a), ("chunk", b)], flagged=[1], n_dup_used=0)


def dup_used():
    """Bundle 2 holds x twice and is used through y, while bundle 0 owns x."""
    rng = np.random.default_rng(19)
    x, y, z = rand_ids(rng, 3)
    bundles = [[(x, 9)], [(z, 4)], [(x, 9), (y, 8), (x, 9)], [(x, 9), (z, 4)]]
    return case("dup_used_bundle", bundles, [("chunk", x), ("chunk", z), ("chunk", y), ("chunk", y)], flagged=[2],
                n_dup_used=2, first_dup=2)


def big_sizes():
    rng = np.random.default_rng(23)
    a, b, c, d = rand_ids(rng, 4)
    big = 0xFFFFFFFF
    bundles = [[(d, 1)], [(a, big), (b, big), (c, big), (d, 1)]]
    return case("three_records_of_2^32-1", bundles, [("chunk", c), ("chunk", b), ("chunk", a), ("chunk", c)],
                far_offset=2 * big)


def zero_sizes():
    rng = np.random.default_rng(29)
    ids = rand_ids(rng, 6)
    bundles = [[(ids[0], 0), (ids[1], 5), (ids[2], 0)], [(ids[3], 0)], [(ids[4], 0), (ids[5], 0)]]
    return case("size_0_records", bundles, [("chunk", c) for c in ids] + [("bytes", 10, 0)])


def bytes_only():
    rng = np.random.default_rng(31)
    ids = rand_ids(rng, 5)
    return case("bytes_only", [[(c, 9) for c in ids]], [("bytes", 3 * k, k % 7) for k in range(300)])


def one_chunk_1000():
    rng = np.random.default_rng(37)
    ids = rand_ids(rng, 50)
    bundles = [[(c, 100 + k) for k, c in enumerate(ids[:25])], [(c, 7) for c in ids[25:]]]
    return case("one_chunk_1000_times", bundles, [("chunk", ids[30])] * 1000)


def missing():
    rng = np.random.default_rng(41)
    ids = rand_ids(rng, 40)
    gone = rand_ids(rng, 3)
    entries = [("chunk", c) for c in ids]
    entries[0] = ("chunk", gone[0])
    entries[17] = ("chunk", gone[1])
    entries[-1] = ("chunk", gone[2])
    return case("missing_first_middle_last", split(rng, [(c, 33) for c in ids], 7), entries, n_missing=3,
                first_missing=0)


def missing_late():
    rng = np.random.default_rng(43)
    ids = rand_ids(rng, 300)
    gone = rand_ids(rng, 2)
    entries = [("chunk", c) for c in ids]
    entries[257] = ("chunk", gone[0])
    entries[-1] = ("chunk", gone[1])
    return case("missing_middle_and_last", split(rng, [(c, 33) for c in ids], 7), entries, n_missing=2,
                first_missing=257)


def empty():
    return case("empty", [], [], data_len=0)


def empty_index_with_entries():
    rng = np.random.default_rng(47)
    ids = rand_ids(rng, 3)
    return case("empty_index", [], [("chunk", ids[0]), ("bytes", 0, 4), ("chunk", ids[1])], n_missing=2,
                first_missing=0)


def bundles_without_records():
    return case("bundles_without_records", [[], [], []], [("bytes", 1, 2)])


SMALL = [empty, empty_index_with_entries, bundles_without_records, collisions, owners, dup_unused, dup_used, big_sizes,
         zero_sizes, bytes_only, one_chunk_1000, missing, missing_late, shapes]


def arrays(bundles):
    """zc_gc_input's layout: ids (n x 24 uint8), sizes (uint32), bundle_first (uint64)."""
    recs = [r for b in bundles for r in b]
    ids = (np.frombuffer(b"".join(bytes(c) for c, _ in recs), dtype=np.uint8).reshape(-1, 24).copy() if recs
           else np.zeros((0, 24), dtype=np.uint8))
    sizes = np.array([s for _, s in recs], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(b) for b in bundles])]).astype(np.uint64)
    return ids, sizes, first


INSTR = np.dtype([("kind", "<u4"), ("id", "u1", (24,)), ("reserved", "<u4"), ("data_off", "<u8"), ("size", "<u8")])


def instructions(entries):
    """The zc_instruction array zc_parse_instructions would give for entries."""
    out = np.zeros(len(entries), dtype=INSTR)
    if entries:
        chunk = np.array([e[0] == "chunk" for e in entries])
        out["kind"] = np.where(chunk, 0, 1)
        out["id"] = np.frombuffer(b"".join(e[1] if e[0] == "chunk" else bytes(24) for e in entries),
                                  dtype=np.uint8).reshape(-1, 24)
        out["data_off"] = np.array([0 if e[0] == "chunk" else e[1] for e in entries], dtype=np.uint64)
        out["size"] = np.array([0 if e[0] == "chunk" else e[2] for e in entries], dtype=np.uint64)
    return out


# every ZC_ERR_ARG the two entry points find before any device work: (name,
# which call, keyword changes to a well-formed call, a fragment of the message)
ERRORS = [
    ("null_idx_out", "create", dict(out=False), "null index pointer"),
    ("null_ids", "create", dict(ids=False), "null input array"),
    ("null_bundle_first", "create", dict(bundle_first=None), "null input array"),
    ("too_many_records", "create", dict(N=(1 << 32) - 1, ids=False), "must stay below 2^32 - 1"),
    ("too_many_bundles", "create", dict(B=(1 << 32) - 1, ids=False), "must stay below 2^32 - 1"),
    ("first_not_0", "create", dict(bundle_first=[1, 1, 3]), "bundle_first[0] = 1, not 0"),
    ("first_decreases", "create", dict(bundle_first=[0, 2, 1]), "bundle_first[2] = 1 is below bundle_first[1] = 2"),
    ("first_ends_short", "create", dict(bundle_first=[0, 1, 2]), "bundle_first ends at 2, there are 3 records"),
    ("first_ends_long", "create", dict(bundle_first=[0, 1, 4]), "bundle_first ends at 4, there are 3 records"),
    ("null_index", "resolve", dict(idx=False), "null index"),
    ("null_plan_out", "resolve", dict(out=False), "null plan pointer"),
    ("null_ins", "resolve", dict(ins=False), "null instruction array"),
    ("too_many_entries", "resolve", dict(n=(1 << 32) - 1, ins=False), "must stay below 2^32 - 1"),
    ("bad_kind", "resolve", dict(kind=2), "entry 1 has kind 2"),
    ("bytes_past_end", "resolve", dict(data_off=90, size=11), "run past the stream's 100 bytes"),
    ("bytes_off_past_end", "resolve", dict(data_off=101, size=0), "run past the stream's 100 bytes"),
    ("length_wraps", "resolve", dict(wrap=True), "length passes 2^64 at entry 2"),
]
