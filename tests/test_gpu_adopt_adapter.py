"""GPU test of the zbackup-side binding's GpuRepositoryAdopter (integration/
gpu_backup_creator.hh): tests/adapter/adopt_main.cpp, compiled against the
stand-in zbackup types, adopts the bundles of a small backup -- one chunk
damaged -- and writes a chunk-metadata file; the binding's own reader accepts
it, and its records and mismatches equal those of the Python Adopter.adopt."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")
W = 4096


@pytest.fixture(scope="module")
def adopt_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    oracle.build()
    exe = str(tmp_path_factory.mktemp("adopt") / "adopt_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "adopt_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def test_adopter_writes_the_sidecar_python_writes(adopt_main, tmp_path):
    import torch

    from tests.adapter import build as adapter_build
    from zbackup_amd import Adopter, BackupCreator, chunk_id_blob, read_sidecar
    from zbackup_amd.adopt import sidecar_bytes
    from zbackup_amd.bundle import plan_bundles
    data = oracle.gen("R3:700000,Z:50000,R4:300001")
    t = torch.from_numpy(np.ascontiguousarray(data)).to("cuda")
    with BackupCreator(W, sha1=True) as bc:
        bc.chunk_device(t.data_ptr(), data.size)
        recs = bc.records()
        exported = bc.export_chunk_meta()
    new = recs[recs["kind"] == 0]
    bundle_of, nb = plan_bundles(new["size"], max_payload=300000)
    assert nb >= 3
    bundles, payloads = [[] for _ in range(nb)], [bytearray() for _ in range(nb)]
    for r, b in zip(new, bundle_of):
        bundles[b].append((chunk_id_blob(bytes(r["sha1"]), int(r["rolling"])), int(r["size"])))
        payloads[b] += data[int(r["offset"]):int(r["offset"]) + int(r["size"])].tobytes()
    payloads[1][len(payloads[1]) // 2] ^= 0x04  # one damaged chunk
    payloads = [bytes(p) for p in payloads]
    ids = [bytes([b + 1]) * 24 for b in range(nb)]
    blob = struct.pack("<I", nb)
    for b in range(nb):
        blob += ids[b] + struct.pack("<I", len(bundles[b]))
        blob += b"".join(cid + struct.pack("<I", size) for cid, size in bundles[b])
        blob += struct.pack("<Q", len(payloads[b])) + payloads[b]
    (tmp_path / "bundles").write_bytes(blob)
    meta_dir = tmp_path / "zchunk"
    out = subprocess.run([adopt_main, str(W), str(tmp_path / "bundles"), str(meta_dir)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    with Adopter(W) as a:
        rep = a.adopt(bundles, payloads)
    assert len(rep.bad) == 1 and rep.bad[0][0] == 1 and rep.bad[0][2] == 3
    assert len(rep.meta) == len(exported) - 1
    lines = out.stdout.split("\n")
    assert "refused: adopt: a bundle's payload is not the sum of its chunk sizes" in lines
    assert f"chunks {rep.chunks} bytes {rep.bytes}" in lines
    assert [ln for ln in lines if ln.startswith("bad ")] == [f"bad {ids[b].hex()} {i} {s}" for b, i, s in rep.bad]
    path = [ln for ln in lines if ln.startswith("path ")][0][5:]
    assert os.listdir(meta_dir) == [os.path.basename(path)]
    # the same bytes Python writes for the same records, and both readers take them
    assert open(path, "rb").read() == sidecar_bytes(rep.meta)
    assert read_sidecar(path).tobytes() == rep.meta.tobytes()
    reader = adapter_build.build_sidecar_reader(out=str(tmp_path / "sidecar_read"))
    got = subprocess.run([reader, str(meta_dir)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert got[0] == str(len(rep.meta))
    assert got[1:1 + len(rep.meta)] == ["%016x %d" % (int(r["rolling"]), int(r["anchor"])) for r in rep.meta]
