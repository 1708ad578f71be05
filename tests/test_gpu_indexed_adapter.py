"""GPU test of the zbackup-side binding's GpuIndexedRestorer (integration/
gpu_backup_creator.hh): tests/adapter/indexed_main.cpp, compiled against the
stand-in zbackup types, serves random ranges of the end-to-end stream's backup
from its bundles' payloads with room for three of them, so payloads are evicted
and fetched again; every range's SHA-256 equals hashlib's over the slice."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")


@pytest.fixture(scope="module")
def indexed_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("indexed") / "indexed_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    # the flags of tests/adapter/build.py
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "indexed_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,$ORIGIN/../../zbackup_amd", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def test_indexed_restorer_serves_ranges_under_a_budget(indexed_main, tmp_path):
    import torch

    from tests.range_stream import chunk_and_bundle, mixed_stream, random_reads
    data = mixed_stream()
    d = torch.from_numpy(data).cuda()
    backup_data, ids, offs, sizes, bundle_of, nb = chunk_and_bundle(d, len(data))
    order = np.random.default_rng(6).permutation(nb)  # the bundles in shuffled order
    blob = struct.pack("<I", nb)
    largest = 0
    for b, k in enumerate(order):
        chunks = np.nonzero(bundle_of == k)[0]
        pay = b"".join(data[offs[i]:offs[i] + sizes[i]].tobytes() for i in chunks)
        largest = max(largest, len(pay))
        blob += bytes([b + 1]) * 24 + struct.pack("<I", len(chunks))
        blob += b"".join(ids[i] + struct.pack("<I", sizes[i]) for i in chunks)
        blob += struct.pack("<Q", len(pay)) + pay
    (tmp_path / "bundles").write_bytes(blob)
    (tmp_path / "backup").write_bytes(backup_data)
    rng = np.random.default_rng(26)
    # short reads all over the stream, a few long ones (one past saveData's step), its two ends
    reads = random_reads(rng, len(data), 60, 200000) + random_reads(rng, len(data), 3, 6 << 20)
    reads += [(0, 1), (len(data) - 1, 1), (len(data), 0), (0, 0)]
    (tmp_path / "reads").write_text("".join(f"{o} {n}\n" for o, n in reads))
    budget = 3 * largest  # room for three payloads
    out = subprocess.run([indexed_main, str(tmp_path / "bundles"), str(tmp_path / "backup"), str(tmp_path / "reads"),
                          str(budget)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == f"size {len(data)}"
    want = [f"read {o} {n} {hashlib.sha256(data[o:o + n].tobytes()).hexdigest()}" for o, n in reads]
    assert [ln for ln in lines if ln.startswith("read ")] == want
    assert "out of range: threw" in lines
    fetched, evicted, resident = (int(v) for v in lines[-2].split()[1::2])
    assert evicted > 0 and fetched > nb and fetched - evicted <= nb  # payloads left and came back
    assert resident <= budget  # the last reads are short: the budget holds again
