#!/usr/bin/env python3
"""Regenerate the golden fixtures in tests/golden/ (run where the reference
sources exist).

Generator: oracle/_ref/zbc_ref_cli = the reference's OWN BackupCreator and
ChunkIndex (backup_creator.cc, chunk_index.cc, chunk_id.cc, rolling_hash.cc and
their helpers, compiled unmodified by `make -C oracle ref` over the stand-in
headers of oracle/refpin/), driven as zutils.cc drives them.  So the boundary
rules, the index probe and every hash in these files come from the reference's
code: the sequence of instructions and of Writer::add calls with their answers.
What does not: Message::serialize and the wire encoding of the instruction
stream (a stand-in of ours; the records are read off the calls, not off bytes),
and the stream generator (oracle/zc_gen.cpp).

`make_golden.py [OUTDIR]` writes into OUTDIR (default: this directory);
tests/test_oracle_ref.py regenerates into a temporary directory and diffs the
result against the committed files.

Each case is a synthetic stream spec (grammar: oracle/zc_oracle.h), so a machine
without the reference regenerates the exact bytes.  Fixture format:
  # key: value        header (case, spec, W, n, seed_spec, feed_max, generator)
  S <sha1_16> <rolling> <size>            index entry registered before the stream
                                          (ChunkIndex::addChunk, in this order)
  N|D|B <offset> <size> <rolling> <sha1_16>
  X <record index>    a NEW record whose Writer::add returned false: the id was
                      in the index already (an earlier NEW record or a seed).
                      Written for the rp_* cases and the corpus; the files of
                      CASES keep their record lines only (some do hold such
                      records, e.g. the periodic ones; tests/refpin_cases.py
                      refused_by_ids names them from the ids)

Three sets are written:
  *.txt                 CASES below, and the directed cases of
                        tests/refpin_cases.py (rp_*: one named edge each, fed
                        with the recorded feed_max)
  refpin_divergent/*.txt  the directed cases whose verdict the engine knowingly does not
                        reproduce (tests/refpin_cases.py DIVERGENT_NAMES): held by the CPU
                        pin, kept out of the set the GPU parity tests run
  refbc_corpus/*.txt    100 of the fuzz streams of tests/refpin_cases.py (W <=
                        4097, at most 40 records; those with refused adds and
                        seeds first), several cases per file
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from oracle import oracle  # noqa: E402
from tests import refpin_cases  # noqa: E402

W64 = 65536

# (name, spec, W, seed_spec)
CASES = [
    # BASELINE.json configs[0]: 16 MiB random stream, W = 64 KiB
    ("c1_rand16m", "R1:16777216", W64, None),
    ("zero16m", "Z:16777216", W64, None),
    ("dup16m", "R2:8388608,C0:8388608", W64, None),
    ("shiftdup", "R3:300000,R4:1000,C0:300000", W64, None),
    ("frag50", "R5:196608,R6:50,C0:196608", W64, None),
    ("finish_big", "R7:360448", W64, None),
    ("small_tail", "R8:131172", W64, None),
    ("empty", "", W64, None),
    ("tiny100", "R9:100", W64, None),
    ("tiny1000", "R9:1000", W64, None),
    ("exact_w", "R10:65536", W64, None),
    ("w_minus_1", "R10:65535", W64, None),
    ("w_plus_1", "R10:65537", W64, None),
    ("two_w_minus_1", "R10:131071", W64, None),
    ("periodic1000", "R11:1000,C0:400000", W64, None),
    ("const255", "B255:300000", W64, None),
    ("mixed", "R12:100000,Z:200000,C50000:150000,B7:70000,C0:90000,R13:5000,C100000:140000", W64, None),
    ("seeded", "R15:12345,R14:400000,R16:70000,R14:200000", W64, "R14:400000"),
    ("w257_rand", "R20:100000", 257, None),
    ("w257_periodic", "R21:3000,C0:60000", 257, None),
    ("w1000_mixed", "R22:50000,C10000:30000,Z:5000,C0:40000", 1000, None),
    ("w4096_periodic3000", "R23:3000,C0:200000", 4096, None),
    ("w4096_shift", "R24:20000,R25:77,C0:20000,R26:300,C5:20000", 4096, None),
    ("w4096_zero_rand", "Z:40000,R31:30000,Z:50000,C0:90000", 4096, None),
    ("w1", "R27:300", 1, None),
    ("w127", "R28:5000", 127, None),
    ("w128", "R29:5000,C0:5000", 128, None),
    ("w65537", "R30:300000,C1:300000", 65537, None),
]

KAT_SPECS = [("empty", ""), ("zero65536", "Z:65536"), ("zero4464", "Z:4464"),
             ("zero3392", "Z:3392"), ("one_byte_ff", "B255:1"), ("rand100", "R99:100"),
             ("rand65536", "R1:65536"), ("rand1000003", "R98:1000003")]


def seeds_from(spec, W):
    recs, _ = oracle.chunk_refbc(oracle.gen(spec), W)
    return [(bytes.fromhex(sha), h, s) for (k, o, s, h, sha) in recs if k == "N"]


CORPUS_N = 100
CORPUS_PER_FILE = 10


def corpus_cases():
    """The recorded fuzz streams: [(index, spec, W, n, seeds, feed_max, recs, refused)]."""
    cand = []
    for i in range(refpin_cases.FUZZ_N):
        spec, W, seeds, feed_max = refpin_cases.fuzz_case(i)
        if W > 4097:
            continue
        data = oracle.gen(spec)
        recs, refused = oracle.chunk_refbc(data, W, seeds, feed_max)
        if len(recs) <= 40:
            cand.append((i, spec, W, data.size, seeds, feed_max, recs, refused))
    # those that say most first: refused adds, then seeded runs, then the rest
    cand.sort(key=lambda c: (not c[7], not c[4], c[0]))
    return sorted(cand[:CORPUS_N])


def write_case(out_dir, name, spec, W, seeds, seed_spec=None, feed_max=None, x_lines=True):
    data = oracle.gen(spec)
    recs, refused = oracle.chunk_refbc(data, W, seeds, feed_max or 0)
    # the answers follow from the ids of the records and seeds; where they are not
    # written down (CASES) they are still checked here
    assert refused == refpin_cases.refused_by_ids(recs, seeds), name
    if not x_lines:
        refused = []
    with open(os.path.join(out_dir, f"{name}.txt"), "w") as f:
        f.write(refpin_cases.case_text(name, spec, W, data.size, seeds, recs, refused, seed_spec, feed_max))
    kinds = {c: sum(1 for r in recs if r[0] == c) for c in "NDB"}
    print(f"{name:30s} n={data.size:9d} W={W:6d} records={len(recs):6d} {kinds} refused={len(refused)}")


def main(out_dir=HERE):
    oracle.build(ref=True)
    for name, spec, W, seed_spec in CASES:
        write_case(out_dir, name, spec, W, seeds_from(seed_spec, W) if seed_spec else [], seed_spec, x_lines=False)
    div_dir = os.path.join(out_dir, "refpin_divergent")
    os.makedirs(div_dir, exist_ok=True)
    for name, spec, W, seed_desc, feed_max in refpin_cases.DIRECTED:
        write_case(div_dir if name in refpin_cases.DIVERGENT_NAMES else out_dir, name, spec, W,
                   refpin_cases.build_seeds(oracle.gen(spec), W, seed_desc), feed_max=feed_max)
    corpus_dir = os.path.join(out_dir, "refbc_corpus")
    os.makedirs(corpus_dir, exist_ok=True)
    corpus = corpus_cases()
    for k in range(0, len(corpus), CORPUS_PER_FILE):
        with open(os.path.join(corpus_dir, f"part{k // CORPUS_PER_FILE:02d}.txt"), "w") as f:
            for i, spec, W, n, seeds, feed_max, recs, refused in corpus[k:k + CORPUS_PER_FILE]:
                f.write(refpin_cases.case_text(f"fuzz{5000 + i}", spec, W, n, seeds, recs, refused,
                                               feed_max=feed_max))
    print(f"refbc_corpus: {len(corpus)} streams")
    L = oracle.lib(ref=True)
    with open(os.path.join(out_dir, "kat_digest.txt"), "w") as f:
        f.write("# RollingHash::digest(buf, size) known answers, computed by the reference's\n")
        f.write("# rolling_hash.cc (oracle/_ref/liboracle_ref.so).  <name> <spec> <digest>\n")
        for name, spec in KAT_SPECS:
            d = oracle.gen(spec, ref=True)
            f.write(f"{name} {spec or '-'} {L.zco_digest(d.ctypes.data, d.size):016x}\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
