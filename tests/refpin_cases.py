"""The streams the reference-built chunker (oracle/_ref/zbc_ref_cli: the
reference's own BackupCreator and ChunkIndex) is run on: the fuzz streams, the
directed cases, and the readers/writers of what it said about them.

Shared by tests/golden/make_golden.py (which records the verdicts as fixtures),
tests/test_oracle_ref.py (CPU: restated oracle against the reference-built
chunker, fixtures against a fresh run) and tests/test_gpu_refpin.py (GPU:
the fixtures only).  Nothing here needs the reference sources.
"""
import glob
import os

import numpy as np

from oracle import oracle

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refbc_corpus")

# --- fuzz streams ------------------------------------------------------------

FUZZ_N = 300
FUZZ_W = [1, 7, 64, 127, 128, 129, 257, 1000, 4096, 4097, 65536]


def random_spec(rng, W):
    segs, n = [], 0
    for _ in range(int(rng.integers(1, 10))):
        t = int(rng.integers(0, 6))
        ln = int(rng.integers(1, 6 * W + 2))
        if t <= 1 or n == 0:
            segs.append(f"R{int(rng.integers(1, 1 << 30))}:{ln}")
        elif t == 2:
            segs.append(f"Z:{ln}")
        elif t == 3:
            segs.append(f"B{int(rng.integers(0, 256))}:{ln}")
        else:
            segs.append(f"C{int(rng.integers(0, n))}:{ln}")
        n += ln
    return ",".join(segs)


def window_id(data, off, W):
    """The true id of the W-byte window at `off`: (sha1_16, rolling, W)."""
    win = data[off:off + W]
    return (bytes(oracle.sha1(win)[:16]), oracle.digest(win), W)


def fuzz_case(i, offsets=False):
    """Fuzz stream i: (spec, W, seeds, feed_max).  rng seed 5000 + i; every third
    run is seeded with four of the stream's own windows, every fourth run is fed
    in capped pieces.  offsets=True: the seeds' window offsets instead of the seeds."""
    rng = np.random.default_rng(5000 + i)
    W = int(rng.choice(FUZZ_W + [int(rng.integers(2, 70000))]))
    spec = random_spec(rng, W)
    seeds, feed_max = [], 0
    if i % 3 == 0:
        data = oracle.gen(spec)
        if data.size >= W:
            offs = [int(off) for off in rng.integers(0, data.size - W + 1, 4)]
            seeds = offs if offsets else [window_id(data, off, W) for off in offs]
    if i % 4 == 0:
        feed_max = int(rng.integers(1, 3 * W + 2))
    return spec, W, seeds, feed_max


def refused_by_ids(recs, seeds):
    """Indices of the NEW records whose id an earlier NEW record or a seed
    carries: the adds ChunkIndex::addChunk refuses (chunk_index.cc:163-202: an id
    is its rolling hash and its 16 SHA-1 bytes; the size takes no part)."""
    seen = {(h, bytes(sha).hex()) for sha, h, _ in seeds}
    out = []
    for i, (k, _, _, h, sha) in enumerate(recs):
        if k == "N":
            if (h, sha) in seen:
                out.append(i)
            seen.add((h, sha))
    return out


# --- directed cases ------------------------------------------------------------
# A seed is described, not stored, so that both generators and tests derive it
# from the stream: ("win", off) the true id of the window at off; ("flip", off)
# the same rolling hash with the first SHA-1 byte flipped (another id under the
# same key); ("sized", off, length, size) the true id of data[off:off+length]
# registered with `size`.

def build_seeds(data, W, desc):
    out = []
    for d in desc:
        if d[0] == "win":
            out.append(window_id(data, d[1], W))
        elif d[0] == "flip":
            sha, h, s = window_id(data, d[1], W)
            out.append((bytes([sha[0] ^ 0x80]) + sha[1:], h, s))
        else:
            _, off, length, size = d
            part = data[off:off + length]
            out.append((bytes(oracle.sha1(part)[:16]), oracle.digest(part), size))
    return out


def _directed():
    cases = []  # (name, spec, W, seed description, feed_max)
    # stream lengths around the window, at the chunk sizes around the 128-byte
    # bytes_to_emit rule and the 256-byte boundary
    for W in (1, 127, 128, 129, 255, 256, 257):
        for tag, n in (("wm1", W - 1), ("w", W), ("wp1", W + 1), ("2wm1", 2 * W - 1), ("2w", 2 * W)):
            if n and not (W == 1 and tag in ("2wm1", "2w")):  # at W = 1 these repeat w and wp1
                cases.append((f"rp_w{W}_len_{tag}", f"R{100 + W}:{n}", W, (), 0))
    for W in (129, 256, 4097):
        # A x A: the second A matches with its window ending on the stream's last
        # byte; the k bytes of x are pending: BYTES below 128, a chunk from 128
        for k in (50, 127, 128):
            cases.append((f"rp_w{W}_match_at_end_frag{k}", f"R1:{W},R2:{k},C0:{W}", W, (), 0))
        # finish with chunkToSaveFill + ringBufferFill > W: r rotated bytes pending
        # and a full ring; the split leaves r bytes for the last record
        for r in (127, 128):
            cases.append((f"rp_w{W}_finish_split{r}", f"R3:{W + r}", W, (), 0))
        # A T A T with 128 <= |T| < W: T is saved before the match and again at
        # finish; the second add is refused
        cases.append((f"rp_w{W}_tail_twice", f"R4:{W},R5:128,C0:{W + 128}", W, (), 0))
    cases.append(("rp_w65536_tail_twice", "R4:65536,R5:200,C0:65736", 65536, (), 0))
    # the tail chunk's id is in the index already (with its size): refused, not matched
    cases.append(("rp_w256_tail_seeded", "R6:256,R7:130", 256, (("sized", 256, 130, 130),), 0))
    # capped feeds over matches and misses.  The ring holds W + 4096 bytes.  At W = 257 a stream
    # of at most 6 W never reaches its end, so the caps only cut the fill and rotate phases into
    # pieces (wpage does not bind at all there).  At W = 4097 the 20,572-byte stream goes round
    # the 8,193-byte ring twice: the caps that divide neither the ring nor W (1000, 4095) put
    # head at a different phase of the extra page on every lap; wpage binds on the first read only
    for W in (257, 4097):
        spec = f"R8:{2 * W + 30},C100:{W + 7},R9:50,C0:{W},C{W}:{W}"
        caps = [("1", 1), ("w", W), ("wpage", W + 4096 - 1)] + ([("1000", 1000), ("4095", 4095)] if W == 4097 else [])
        for tag, cap in caps:
            cases.append((f"rp_w{W}_feedcap_{tag}", spec, W, (), cap))
    # two ids under one rolling key (the key of the stream's first window), in
    # both insertion orders; the wrong id alone; the true id twice; a size that is not W
    for W in (256, 4097):
        spec = f"R10:{W},R11:100,C0:{W},R12:{W + 5}"
        cases.append((f"rp_w{W}_samekey_true_first", spec, W, (("win", 0), ("flip", 0)), 0))
        cases.append((f"rp_w{W}_samekey_flip_first", spec, W, (("flip", 0), ("win", 0)), 0))
        cases.append((f"rp_w{W}_samekey_flip_only", spec, W, (("flip", 0),), 0))
        cases.append((f"rp_w{W}_seed_twice", spec, W, (("win", 0), ("win", 0)), 0))
        cases.append((f"rp_w{W}_seed_size_not_w", spec, W, (("sized", 0, W, W - 1),), 0))
    return cases


DIRECTED = _directed()
DIRECTED_NAMES = [c[0] for c in DIRECTED]
# The cases whose reference verdict the engine knowingly does not reproduce (it registers W-byte
# ids only: include/zchunk.h at zc_seed_index).  The CPU pin holds them like the others; their
# fixtures lie in tests/golden/refpin_divergent/, outside the set every GPU parity test runs, and
# tests/test_gpu_refpin.py asserts what the engine gives for them instead.
DIVERGENT_NAMES = [n for n in DIRECTED_NAMES if n.endswith("_seed_size_not_w")]
DIVERGENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_divergent")


def fixture_path(name):
    from tests import golden_io
    return os.path.join(DIVERGENT if name in DIVERGENT_NAMES else golden_io.GOLDEN, name + ".txt")

# --- fixture text ------------------------------------------------------------
GENERATOR = "oracle/_ref/zbc_ref_cli (the reference's own BackupCreator and ChunkIndex)"


def case_text(name, spec, W, n, seeds, recs, refused=(), seed_spec=None, feed_max=None):
    """One case in the golden format (tests/golden/make_golden.py)."""
    lines = [f"# case: {name}", f"# spec: {spec}", f"# W: {W}", f"# n: {n}", f"# seed_spec: {seed_spec or '-'}"]
    if feed_max is not None:
        lines.append(f"# feed_max: {feed_max}")
    lines.append(f"# generator: {GENERATOR}")
    lines += [f"S {sha.hex()} {h:016x} {s}" for sha, h, s in seeds]
    lines += oracle.format_records(recs)
    lines += [f"X {i}" for i in refused]
    return "\n".join(lines) + "\n"


def parse_cases(text):
    """Every case of a fixture text: [(meta, seeds, recs)]; meta carries W, n, spec,
    feed_max (0: uncapped) and refused (the X lines)."""
    cases = []
    for line in text.splitlines():
        if line.startswith("# case:"):
            cases.append(({"refused": []}, [], []))
        if not cases:
            continue
        meta, seeds, recs = cases[-1]
        if line.startswith("# ") and ":" in line:
            k, v = line[2:].split(":", 1)
            meta[k.strip()] = v.strip()
        elif line.startswith("S "):
            _, sha, h, size = line.split()
            seeds.append((bytes.fromhex(sha), int(h, 16), int(size)))
        elif line.startswith("X "):
            meta["refused"].append(int(line[2:]))
        elif line and line[0] in "NDB":
            k, off, size, h, sha = line.split()
            recs.append((k, int(off), int(size), int(h, 16), sha))
    for meta, _, _ in cases:
        meta["W"], meta["n"] = int(meta["W"]), int(meta["n"])
        meta["feed_max"] = int(meta.get("feed_max", 0))
        meta.setdefault("spec", "")
    return cases


def corpus_paths():
    return sorted(glob.glob(os.path.join(CORPUS, "*.txt")))


def load_corpus():
    """[(meta, seeds, recs)] of tests/golden/refbc_corpus, in file order."""
    out = []
    for p in corpus_paths():
        with open(p) as f:
            out += parse_cases(f.read())
    return out
