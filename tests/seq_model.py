"""The Python-side model of one long-lived context, for the sequence tests
(tests/test_gpu_sequences.py on the GPU, tests/test_sequence_plans.py without).

A context keeps its index between streams: with ZC_FLAG_SHA1 every W-byte chunk
a stream saved (an N record of size W: Writer::add -> ChunkIndex::addChunk)
joins it, zc_seed_index appends ids, zc_forget_stream_chunks drops what the
streams added.  ContextModel keeps that index on the host and predicts each
stream's records with the oracle run against it, and restates from the code
when the first epoch's index insert takes the fused form.  make_plan() draws the
seeded sequence plans of the fuzz; plan_records() runs the model over one."""
import functools

import numpy as np

from oracle import oracle

STILE = 2 << 20  # ZC_STILE: the scan's tile
PATHS = ("device", "host", "window", "feed0")
FUSED, SCAN_KEYS, REALLOC, CLEARED = 1, 2, 4, 8  # ZC_PATH_* (include/zchunk.h)
SEED0 = np.zeros(0, dtype=oracle.SEED_DTYPE)


def strip_sha(recs):
    """What a context without ZC_FLAG_SHA1 reports: chunk ids by rolling hash only."""
    return [(k, o, s, h, "0" * 32 if k != "B" else sha) for (k, o, s, h, sha) in recs]


def tuples(recs):
    """A record array (oracle.RECORD_DTYPE) in record_tuples() format."""
    hexes = recs["sha1"].tobytes().hex()
    return [("NDB"[k], o, s, h, hexes[32 * i:32 * i + 32]) for i, (k, o, s, h) in enumerate(
        zip(recs["kind"].tolist(), recs["offset"].tolist(), recs["size"].tolist(), recs["rolling"].tolist()))]


def ids_of(recs, W):
    """The ids (a SEED_DTYPE array) of the W-byte chunks `recs` saves."""
    sel = recs[(recs["kind"] == oracle.KIND_NEW) & (recs["size"] == W)]
    out = np.zeros(len(sel), dtype=oracle.SEED_DTYPE)
    out["sha1"], out["rolling"], out["size"] = sel["sha1"], sel["rolling"], W
    return out


def chunk_id(chunk):
    """The id of one chunk's bytes, as a seed tuple."""
    return (bytes(oracle.sha1(chunk)[:16]), oracle.digest(chunk), int(chunk.size))


def in_scan_key_set(W):
    """scan_key_lshift_or_none (zc_device.h): the scan writes the grid keys when W
    is a multiple of the 4 KiB lane span and divides the 256 KiB wave-tile."""
    return W >= 4096 and W % 4096 == 0 and (64 * 4096) % W == 0


def table_bits(n, W):
    """Resolver::epoch: the first epoch's tables have 2^bits slots, four per ref."""
    nsref = n // W - 1 if n >= 2 * W and W >= 128 else 0
    bits = 10
    while (1 << bits) < 4 * nsref:
        bits += 1
    return bits if nsref else 0


class ContextModel:
    def __init__(self, W, sha1, seeds=()):
        self.W, self.sha1 = W, sha1
        self.seeded = [oracle.seed_array(seeds)]
        self.added = []       # id arrays of the streams so far
        self.tables = False   # an earlier stream made the epoch tables (and its end cleared them)
        self.bits = 0         # the largest tables so far, log2 slots: at most this
        self.bits_sure = 0    # ... and at least this (a window's epochs are sized by its segments)

    def index(self, carried=True):
        return np.concatenate(self.seeded + (self.added if carried else []))

    def count_added(self):
        return sum(len(a) for a in self.added)

    def predict(self, data, carried=True):
        """The oracle's records of `data` against the index (a record array)."""
        return oracle.chunk_array(data, self.W, seeds=self.index(carried))

    def expect(self, recs):
        want = tuples(recs)
        return want if self.sha1 else strip_sha(want)

    def fused(self, n, path):
        """launch_epoch_index's `fused`, from what the model knows -- all but a
        reallocation of the tables, which the caller reads from the path bits:
        tables_clean (a later stream of the context: Resolver::clear_tables at a
        stream's end needs tables, which an epoch with refs makes), and
        key_from == nsref (begin: scan_keys_ -- W in the scan-key set, the whole
        stream resident -- and every grid chunk inside the scanned full tiles)."""
        W = self.W
        nsref = n // W - 1
        return (self.tables and path != "window" and in_scan_key_set(W) and nsref >= 1
                and nsref <= n // STILE * STILE // W)

    def commit(self, recs, n, path):
        if self.sha1:
            self.added.append(ids_of(recs, self.W))
        b = table_bits(n, self.W)
        if b:
            self.tables = True
            self.bits = max(self.bits, b)
            if path != "window":
                self.bits_sure = max(self.bits_sure, b)

    def forget(self):
        self.added = []

    def seed(self, extra):
        self.seeded.append(oracle.seed_array(extra))


# ---- the seeded sequence plans -------------------------------------------

def _lz_copy(buf, off, ln):
    """buf[off:off+ln] with LZ semantics (a copy may run into itself), as the
    oracle generator's C segments."""
    src = buf[off:]
    return np.resize(src, ln) if src.size < ln else src[:ln].copy()


def _content(rng, W, n, earlier, live=()):
    """n bytes drawn the way the fuzz's _spec draws segments -- random, zeros, a
    repeated byte, copies of this stream's own ranges, short pieces -- plus
    copies of ranges of the context's earlier streams; long streams also get
    long segments, so that a stream is tens of segments, not thousands."""
    out = np.empty(n, dtype=np.uint8)
    pos, nseg, segs = 0, 0, []
    earlier = [e for e in earlier if e.size]
    while pos < n:
        t = int(rng.integers(0, 8))
        u = rng.random()
        ln = int(rng.integers(1, 300)) if u < 0.25 else int(rng.integers(1, (12 if u > 0.9 else 4) * W + 2))
        if rng.random() < 0.5 or nseg >= 40:
            ln = max(ln, int(rng.integers(1, max(n // 4, 2))))
        if nseg >= 60:
            ln = n
        ln = min(ln, n - pos)
        big = [e for e in live if e.size >= 3 * W]
        if nseg in (1, 3) and big and n - pos >= 3 * W:
            # always two ranges of the last stream whose chunks the index still
            # holds (`live`: none forgotten since), long enough to hold a whole chunk
            # of its grid wherever it starts: a match only the carried index gives
            e, t = big[-1], 6
            ln = min(int(rng.integers(3 * W, 6 * W + 1)), e.size, n - pos)
            off = int(rng.integers(0, e.size - ln + 1))
            out[pos:pos + ln] = e[off:off + ln]
            segs.append(f"X{off}:{ln}")
        elif t >= 6 and earlier:
            e = earlier[int(rng.integers(0, len(earlier)))]
            off = int(rng.integers(0, e.size))
            ln = min(ln, e.size - off)
            out[pos:pos + ln] = e[off:off + ln]
            segs.append(f"X{off}:{ln}")
        elif t == 0 or t == 5 or pos == 0:
            s = int(rng.integers(1, 1 << 30))
            out[pos:pos + ln] = oracle.splitmix64(ln, s)
            segs.append(f"R{s}:{ln}")
        elif t == 1:
            out[pos:pos + ln] = 0
            segs.append(f"Z:{ln}")
        elif t == 2:
            b = int(rng.integers(0, 256))
            out[pos:pos + ln] = b
            segs.append(f"B{b}:{ln}")
        else:
            off = int(rng.integers(0, pos))
            if off + ln > pos:  # runs into itself: periodic from here on, kept as short as the fuzz's
                ln = min(ln, 12 * W + 2)
            out[pos:pos + ln] = _lz_copy(out[:pos], off, ln)
            segs.append(f"C{off}:{ln}")
        pos += ln
        nseg += 1
    return out, ",".join(segs)


def _length(rng, W):
    u = int(rng.integers(0, 10))
    if u == 0:
        return int(rng.choice([0, 1]))
    if u == 1:
        return int(rng.choice([W - 1, W + 1]))
    if u <= 5:
        return int(rng.integers(1, 4)) * STILE + int(rng.choice([0, W - 1]))
    return int(rng.integers(1, (6 << 20) + 1))


WS = (128, 256, 1000, 4096, 4100, 12288, 65536)
WS_DRAW = WS + (4096, 65536, 65536)  # (more of the chunk sizes whose grid keys the scan writes)


def make_plan(seed):
    """Plan `seed` of the sequence fuzz: one context (W, sha1, initial seeds; every
    third seeded from another stream's chunks) and 6-10 steps, each {path,
    data, spec, forget, extra}: forget_stream_chunks() and seed_index(extra)
    come after reset() and before the step's stream."""
    rng = np.random.default_rng(91200 + seed)
    W = int(WS[seed % len(WS)] if seed < 2 * len(WS) else rng.choice(WS_DRAW))
    sha1 = bool(seed % 4 != 3)
    steps, datas, live = [], [], []
    for i in range(int(rng.integers(6, 11))):
        forget = bool(i and rng.random() < 0.25)
        if forget:
            live = []
        data, spec = _content(rng, W, _length(rng, W), datas, live)
        datas.append(data)
        live.append(data)
        steps.append({"path": PATHS[int(rng.integers(0, 4))], "data": data, "spec": spec,
                      "forget": forget, "extra": []})
    seeds = []
    if seed % 3 == 0:
        other, _ = _content(np.random.default_rng(92000 + seed), W, 40 * W + 77, [])
        pick = next(d for d in datas if d.size >= 2 * W) if any(d.size >= 2 * W for d in datas) else other
        arr = ids_of(oracle.chunk_array(np.concatenate([other, pick[:2 * W]]), W), W)
        seeds = [(bytes(a["sha1"]), int(a["rolling"]), int(a["size"])) for a in arr]
    for i, st in enumerate(steps):
        if i and rng.random() < 0.25:  # a few ids: half real chunks of a future stream, half fake
            for k in range(int(rng.integers(2, 7))):
                fut = [d for d in datas[i:] if d.size >= W]
                if k % 2 == 0 and fut:
                    d = fut[int(rng.integers(0, len(fut)))]
                    off = int(rng.integers(0, d.size - W + 1))
                    st["extra"].append(chunk_id(d[off:off + W]))
                else:
                    st["extra"].append((bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
                                        int(rng.integers(1, 1 << 62)), W))
    return {"seed": seed, "W": W, "sha1": sha1, "seeds": seeds, "steps": steps}


def describe(plan):
    """The whole plan as text (printed when a sequence fails)."""
    lines = [f"plan seed={plan['seed']} W={plan['W']} sha1={plan['sha1']} seeds={len(plan['seeds'])}"]
    for i, st in enumerate(plan["steps"]):
        lines.append(f"  step {i}: forget={st['forget']} seed_index={len(st['extra'])} path={st['path']} "
                     f"n={st['data'].size} spec={st['spec']}")
    return "\n".join(lines)


@functools.lru_cache(maxsize=None)
def plan_records(seed):
    """The model run over plan `seed`, once per process (the records only: a
    plan's streams are drawn again by make_plan): per step the oracle's
    record array, the prediction of the fused form (but for a reallocation),
    the model's count of stream-added ids after the step, and whether one of
    the step's D records matches a chunk only an earlier stream added.
    fused and fits: the step is predicted to take the fused form."""
    plan = make_plan(seed)
    m = ContextModel(plan["W"], plan["sha1"], plan["seeds"])
    out = []
    for st in plan["steps"]:
        if st["forget"]:
            m.forget()
        if st["extra"]:
            m.seed(st["extra"])
        recs = m.predict(st["data"])
        carried = False
        if m.sha1 and m.count_added():
            # a D record whose id only the carried index holds (not the seeds,
            # not a chunk this stream saved itself): without the carried index
            # the window is no match, and the oracle run without it says so
            mine = set(map(bytes, ids_of(recs, m.W)["sha1"])) | set(map(bytes, m.index(False)["sha1"]))
            dup = recs[recs["kind"] == oracle.KIND_DUP]
            cand = [bytes(s) for s in dup["sha1"] if bytes(s) not in mine]
            if cand:
                alone = m.predict(st["data"], carried=False)
                alone_d = set(map(bytes, alone[alone["kind"] == oracle.KIND_DUP]["sha1"]))
                carried = any(c not in alone_d for c in cand)
        fused = m.fused(st["data"].size, st["path"])
        need = table_bits(st["data"].size, m.W)
        grows, fits = need > m.bits, need <= m.bits_sure  # larger tables than any so far / surely not
        m.commit(recs, st["data"].size, st["path"])
        out.append({"recs": recs, "fused": fused, "grows": grows, "fits": fits, "added": m.count_added(),
                    "carried": carried})
    return out
