"""CPU tests of the resident chunk index:

* zc_resolve_core.h -- the position maps, the (id, bundle) table, the owner
  lookup and the per-entry step the kernels of zc_resolve.hip run -- compiled
  for the host (under ASan + UBSan where that links) with a main of its own and
  compared with std::map / std::set (tests/resolve/resolve_core_check.cpp);
* tests/resolve_ref.py against Restorer.plan / chunk_map on inputs without
  cross-bundle duplicates: the same per-entry (bundle, off, size), the same
  length, the same replayed bytes;
* the case generator of the GPU tests (tests/resolve_cases.py): every case is
  what it claims to be."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import resolve_cases as C
from tests import resolve_ref as R
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_check(tmp_path):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path / "resolve_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "resolve", "resolve_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


def test_core_matches_std_containers(tmp_path):
    exe, sanitized = _build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) >= 30000


def _stream(entries, data_len):
    """A BackupInstruction stream with a chunk_to_emit per chunk entry and
    e[2] random bytes_to_emit per bytes entry (the parse says where they lie)."""
    from zbackup_amd import serialize_instruction
    rng = np.random.default_rng(5)
    parts = []
    for e in entries:
        if e[0] == "chunk":
            parts.append(serialize_instruction(chunk_blob=e[1]))
        else:
            parts.append(serialize_instruction(raw=rng.integers(0, 256, e[2], dtype=np.uint8).tobytes()))
    return b"".join(parts)


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_ref_agrees_with_plan_and_chunk_map(lib):
    """Without cross-bundle duplicates the first-use plan and the reference
    restatement describe the same restore, up to the order of the slots."""
    from zbackup_amd import parse_backup_data
    from zbackup_amd.restore import Restorer, chunk_map
    rng = np.random.default_rng(3)
    for n, max_records in ((0, 3), (1, 3), (40, 5), (700, 60)):
        ids = C.rand_ids(rng, n)
        recs = [(c, int(s)) for c, s in zip(ids, rng.integers(0, 300, n))]
        bundles = C.split(rng, recs, max_records)
        ix = R.build(bundles)
        cmap = chunk_map(bundles)
        assert len(cmap) == len(ix["owner"]) == n
        for c in ids:
            assert R.lookup(ix, c) == cmap[c]
        want = C.entries_for(rng, ids, 2 * n + 3, 0, bytes_share=0.3)
        want = [e if e[0] == "chunk" else ("bytes", 0, int(rng.integers(0, 30))) for e in want]
        data = _stream(want, 0)
        ins = parse_backup_data(data)
        entries = [("chunk", e["id"].tobytes()) if e["kind"] == _lib.ZC_INSTR_CHUNK
                   else ("bytes", int(e["data_off"]), int(e["size"])) for e in ins]
        ref = R.resolve(ix, entries)
        plan = Restorer.plan(data, bundles)
        assert plan.length == ref["length"] and sorted(plan.used) == ref["used"]
        assert plan.sizes.tolist() == ref["size"] and plan.dst_off.tolist() == ref["dst"]
        for k, e in enumerate(entries):  # per entry: the same bundle and offset behind the two slot orders
            if e[0] == "chunk":
                b = ref["used"][ref["slot"][k]]
                assert int(plan.src_off[k]) == plan.pay_off[plan.used.index(b)] + ref["off"][k]
            else:
                assert int(plan.src_off[k]) == plan.instr_off + ref["off"][k]
        # the replayed bytes, via numpy over the plan's image
        payloads = [rng.integers(0, 256, s, dtype=np.uint8).tobytes() for s in ix["bundle_size"]]
        img = plan.host_image([payloads[b] for b in plan.used])
        got = b"".join(img[int(s):int(s) + int(z)].tobytes() for s, z in zip(plan.src_off, plan.sizes))
        assert got == R.restore_bytes(ix, entries, payloads, data)


def test_ref_self_check():
    R._self_check()
    header = open(os.path.join(ROOT, "include", "zchunk.h")).read()
    assert int(re.search(r"#define ZC_NO_BUNDLE (0x[0-9A-Fa-f]+)u", header).group(1), 16) == R.NO_BUNDLE
    assert R.NO_BUNDLE == _lib.ZC_NO_BUNDLE and (R.CHUNK, R.BYTES) == (_lib.ZC_INSTR_CHUNK, _lib.ZC_INSTR_BYTES)


def test_scan_edge_cases_have_their_counts():
    for n in C.SCAN_EDGES:
        c = C.scan_edge(n)
        assert sum(len(b) for b in c["bundles"]) == n == len(c["entries"])
        if n >= 64:
            ix = R.build(c["bundles"])
            assert R.counts(ix)["ids"] == n - n // 10  # a tenth of the records repeat an id
            kinds = {e[0] for e in c["entries"]}
            assert kinds == {"chunk", "bytes"}
    assert max(C.SCAN_EDGES) > 256 * 256  # more tiles than one round of the tile scan's first level takes


def test_named_cases_are_what_they_claim():
    cases = {c["name"]: c for c in (f() for f in C.SMALL)}
    assert len(cases) == len(C.SMALL)
    c = cases["bundle_shapes"]
    assert [len(b) for b in c["bundles"]] == [0, 1, 64, 65, 5000, 0, 3]
    # the colliding ids: one slot hash, a run that wraps the table's end over foreign owners
    c = cases["collisions"]
    mask = (1 << c["bits"]) - 1
    assert {C.slot_hash(x, mask) for x in c["group"] + c["strangers"]} == {C.COLLIDE_START}
    assert len({C.id_fold(x) for x in c["group"] + c["strangers"]}) == 1
    assert len(c["group"]) == 40 and C.COLLIDE_START + len(c["group"]) > mask + 1  # the run wraps
    run = {(C.COLLIDE_START + k) & mask for k in range(len(c["group"]))}
    assert len(c["foreign"]) >= 3 and all(C.slot_hash(x, mask) in run for x in c["foreign"])
    assert all(C.id_fold(x) != C.id_fold(c["group"][0]) for x in c["foreign"])
    n = sum(len(b) for b in c["bundles"])
    assert n == len(c["group"]) + len(c["foreign"]) < mask + 1  # the forced table leaves a free slot
    assert not set(c["strangers"]) & set(c["group"])
    # owners
    c = cases["owners_2_and_5"]
    holds = lambda x: [b for b, recs in enumerate(c["bundles"]) if any(r[0] == x for r in recs)]  # noqa: E731
    assert len(holds(c["in_two"])) == 2 and len(holds(c["in_five"])) == 5
    ix = R.build(c["bundles"])
    assert R.lookup(ix, c["in_two"])[0] == holds(c["in_two"])[0] == c["owner_of_two"]
    assert R.lookup(ix, c["in_five"])[0] == holds(c["in_five"])[0] == c["owner_of_five"]
    assert not any(ix["dup"])
    # duplicates inside a bundle
    for name in ("dup_unused_bundle", "dup_used_bundle"):
        c = cases[name]
        ix = R.build(c["bundles"])
        r = R.resolve(ix, c["entries"])
        assert [b for b, d in enumerate(ix["dup"]) if d] == c["flagged"]
        assert r["n_dup_used"] == c["n_dup_used"] and r["n_missing"] == 0
        assert (c["flagged"][0] in r["used"]) == (name == "dup_used_bundle")
    c = cases["dup_used_bundle"]
    ix = R.build(c["bundles"])
    x = c["entries"][0][1]
    assert R.lookup(ix, x)[0] == 0 and sum(1 for r in c["bundles"][2] if r[0] == x) == 2
    assert R.resolve(ix, c["entries"])["first_dup"] == c["first_dup"]
    # 64-bit offsets
    c = cases["three_records_of_2^32-1"]
    r = R.resolve(R.build(c["bundles"]), c["entries"])
    assert max(r["off"]) == c["far_offset"] > 1 << 32 and r["length"] == 4 * 0xFFFFFFFF
    assert [s for _, s in c["bundles"][1]].count(0xFFFFFFFF) == 3
    # sizes of 0, bytes only, one chunk 1,000 times
    c = cases["size_0_records"]
    assert sum(1 for b in c["bundles"] for _, s in b if s == 0) == 5
    c = cases["bytes_only"]
    assert {e[0] for e in c["entries"]} == {"bytes"} and R.resolve(R.build(c["bundles"]), c["entries"])["n_used"] == 0
    c = cases["one_chunk_1000_times"]
    assert len(c["entries"]) == 1000 and len({e[1] for e in c["entries"]}) == 1
    # missing ids
    c = cases["missing_first_middle_last"]
    r = R.resolve(R.build(c["bundles"]), c["entries"])
    miss = [k for k, s in enumerate(r["slot"]) if s == R.NO_BUNDLE]
    assert miss[0] == 0 and miss[-1] == len(c["entries"]) - 1 and len(miss) == 3 == r["n_missing"]
    assert r["first_missing"] == 0
    c = cases["missing_middle_and_last"]
    r = R.resolve(R.build(c["bundles"]), c["entries"])
    assert (r["n_missing"], r["first_missing"]) == (2, 257)
    for name in ("empty", "empty_index", "bundles_without_records"):
        assert sum(len(b) for b in cases[name]["bundles"]) == 0
    # every bytes run of every case lies inside its stream
    for c in cases.values():
        assert all(e[1] + e[2] <= c["data_len"] for e in c["entries"] if e[0] == "bytes"), c["name"]


def test_every_error_kind_has_a_case():
    kinds = " ".join(text for _, _, _, text in C.ERRORS)
    for needle in ("null index pointer", "null input array", "null plan pointer", "null instruction array",
                   "must stay below 2^32 - 1", "not 0", "is below", "ends at", "has kind", "run past", "passes 2^64"):
        assert needle in kinds
    assert {call for _, call, _, _ in C.ERRORS} == {"create", "resolve"}
    assert len({name for name, _, _, _ in C.ERRORS}) == len(C.ERRORS)
