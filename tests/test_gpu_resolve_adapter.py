"""GPU test of the zbackup-side binding's GpuResidentChunkIndex (integration/
gpu_backup_creator.hh): tests/adapter/resolve_main.cpp, compiled against the
stand-in zbackup types, loads index files written by write_index (with a key),
answers a batch findChunk and plans a backup; every printed line equals what
tests/resolve_ref.py says, and a missing chunk and a used bundle that holds an
id twice come back under the reference's exception names."""
import os
import subprocess

import numpy as np
import pytest

from tests import resolve_cases as C
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")
KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d7781")


@pytest.fixture(scope="module")
def resolve_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("resolve") / "resolve_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    # the flags of tests/adapter/build.py
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "resolve_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,$ORIGIN/../../zbackup_amd", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def run(exe, tmp_path, key, index_files, entries, ids):
    from zbackup_amd import serialize_instruction
    stream = b"".join(serialize_instruction(chunk_blob=e[1]) if e[0] == "chunk" else serialize_instruction(raw=e[1])
                      for e in entries)
    (tmp_path / "backup").write_bytes(stream)
    (tmp_path / "ids").write_bytes(b"".join(ids))
    names = []
    for k, f in enumerate(index_files):
        (tmp_path / f"index{k}").write_bytes(f)
        names.append(str(tmp_path / f"index{k}"))
    out = subprocess.run([exe, key.hex() if key else "none", str(tmp_path / "backup"), str(tmp_path / "ids")] + names,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return stream, out.stdout.split("\n")


def test_adapter_finds_and_plans_as_the_reference(resolve_main, tmp_path):
    from zbackup_amd import parse_backup_data, write_index
    from zbackup_amd.bundle import BundleCompressor
    rng = np.random.default_rng(67)
    case = C.scan_edge(257)
    dup = C.dup_used()
    bundles = case["bundles"] + dup["bundles"]
    bundle_ids = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in bundles]
    cut = len(bundles) // 3
    with BundleCompressor() as comp:
        files = [write_index(list(zip(bundle_ids[a:b], bundles[a:b])), key=KEY,
                             r=bytes(rng.integers(0, 256, 16, dtype=np.uint8)), comp=comp)
                 for a, b in ((0, cut), (cut, len(bundles)))]
    files.insert(1, files[0][:-16])  # a file that lost its last cipher block: bad padding or worse, nothing from it
    ix = R.build(bundles)
    known = [c for b in case["bundles"][::3] for c, _ in b]
    gone = [bytes([7]) * 24, bytes(24)]
    x, z, y = (dup["entries"][k][1] for k in (0, 1, 2))

    # a clean backup: chunks of the first case, bytes runs, x (owned by a clean bundle although another holds it twice)
    entries = [("chunk", c) for c in known[:150]] + [("bytes", b"raw bytes")] + [("chunk", x), ("chunk", z)]
    stream, lines = run(resolve_main, tmp_path, KEY, files, entries, known + gone + [x, y])
    c = R.counts(ix)
    assert lines[0] == f"index bundles {c['bundles']} records {c['records']} ids {c['ids']} flagged {c['flagged']}"
    status = lines[1].split()
    assert status[0] == "status" and status[1] == "0" and status[2] != "0" and status[3] == "0"
    finds = [ln for ln in lines if ln.startswith("find ")]
    want = []
    for cid in known + gone + [x, y]:
        b, off, size = R.lookup(ix, cid)
        want.append(f"find {cid.hex()} {'none' if b == R.NO_BUNDLE else bundle_ids[b].hex()} {off} {size}")
    assert finds == want
    parsed = parse_backup_data(stream)
    ref = R.resolve(ix, [("chunk", e["id"].tobytes()) if e["kind"] == 0 else
                         ("bytes", int(e["data_off"]), int(e["size"])) for e in parsed])
    assert f"plan length {ref['length']} used {ref['n_used']} entries {ref['n_entries']}" in lines
    assert [ln for ln in lines if ln.startswith("used ")] == [f"used {bundle_ids[b].hex()} {s}"
                                                              for b, s in zip(ref["used"], ref["used_size"])]
    assert [ln for ln in lines if ln.startswith("entry ")] == [
        f"entry {s} {o} {n} {d}" for s, o, n, d in zip(ref["slot"], ref["off"], ref["size"], ref["dst"])]

    # a chunk no bundle holds; a used bundle that holds an id twice
    _, lines = run(resolve_main, tmp_path, KEY, files, [("chunk", known[0]), ("chunk", gone[0]), ("chunk", gone[1])], [])
    assert [ln for ln in lines if ln.startswith("plan ")] == [
        f"plan exNoSuchChunk chunk {gone[0].hex()} is in no bundle of the index"]
    _, lines = run(resolve_main, tmp_path, KEY, files, [("chunk", known[0]), ("chunk", y)], [])
    flagged = bundle_ids[len(case["bundles"]) + dup["flagged"][0]]
    assert [ln for ln in lines if ln.startswith("plan ")] == [
        f"plan exDuplicateChunks bundle {flagged.hex()} holds a chunk id twice"]
