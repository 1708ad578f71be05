"""GPU test of the zbackup-side binding's GpuXzBundleDecoder (integration/
gpu_backup_creator.hh) and of the two entry points that take its device
payloads, GpuRepositoryAdopter::addBundlesDevice and
GpuIndexedRestorer::setPayloads: tests/adapter/xz_main.cpp, compiled against
the stand-in zbackup types, decodes the LZMA bodies of a small repository to
the host and to the device.  The host payloads are liblzma's; what
Bundle::Reader refuses throws; the adopter over the device payloads writes
the sidecar and reports the mismatch the adopter over host payloads does (and
Python's Adopter.adopt); the restorer serves every read from the device
payloads with the bytes of the backup, its host source never asked."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import xz_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason=R.why_not())]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")
W = 4096


@pytest.fixture(scope="module")
def xz_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("xz_adapter") / "xz_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "xz_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def test_decoder_and_the_device_payload_paths(xz_main, tmp_path):
    from tests.test_gpu_xz_paths import make_repo, true_ids
    from zbackup_amd import Adopter, serialize_instruction
    from zbackup_amd.adopt import sidecar_bytes
    fake, payloads, _, _, _ = make_repo()
    with Adopter(W) as a:
        bundles = true_ids(a, fake, payloads)
        damaged = bytearray(payloads[1])
        damaged[5000] ^= 1  # one damaged chunk: the bundle still claims the old id
        payloads = [payloads[0], bytes(damaged), payloads[2]]
        rep = a.adopt(bundles, payloads)
    assert len(rep.bad) == 1 and rep.bad[0][0] == 1
    bodies = [R.compress(p) for p in payloads]
    assert len({len(p) for p in payloads}) == 3
    # the backup: most chunks in shuffled order, one twice, bytes_to_emit runs between them
    rng = np.random.default_rng(8)
    chunks = [(blob, payloads[b][sum(s for _, s in recs[:i]):][:size])
              for b, recs in enumerate(bundles) for i, (blob, size) in enumerate(recs)]
    order = list(rng.permutation(len(chunks)))[:len(chunks) - 2] + [3]
    stream, want = b"", b""
    for j, c in enumerate(order):
        raw = bytes(rng.integers(0, 256, 1 + j % 7, dtype=np.uint8)) if j % 5 == 0 else None
        stream += serialize_instruction(chunk_blob=chunks[c][0], raw=raw)
        want += chunks[c][1] + (raw or b"")
    ids = [bytes([b + 1]) * 24 for b in range(len(bundles))]
    blob = struct.pack("<I", len(bundles))
    for b, recs in enumerate(bundles):
        blob += ids[b] + struct.pack("<I", len(recs)) + b"".join(cid + struct.pack("<I", size) for cid, size in recs)
        blob += struct.pack("<Q", len(payloads[b])) + payloads[b] + struct.pack("<Q", len(bodies[b])) + bodies[b]
    (tmp_path / "bundles").write_bytes(blob)
    (tmp_path / "backup").write_bytes(stream)
    reads = [(0, len(want)), (0, 1), (4095, 9000), (len(want) - 17, 17), (12345, 70000)]
    (tmp_path / "reads").write_text("".join(f"{o} {n}\n" for o, n in reads))
    out = subprocess.run([xz_main, str(W), str(tmp_path / "bundles"), str(tmp_path / "backup"), str(tmp_path / "reads"),
                          str(tmp_path / "meta_host"), str(tmp_path / "meta_device")], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert f"decodeAll ok {len(bundles)}" in lines and "decode ok" in lines and "in use: threw" in lines
    threw = [ln[7:] for ln in lines if ln.startswith("threw: ")]
    n1 = len(payloads[1])
    assert threw[0].startswith("bundle 0: xz status 5 ")  # ZC_XZ_E_INPUT
    assert threw[1] == f"bundle 0: the stream ends after {len(bodies[1])} of the body's {len(bodies[1]) + 4} bytes"
    assert threw[2] == f"bundle 0: {n1} bytes decoded, its payload has {n1 + 1}"
    assert threw[3].startswith("bundle 0: xz status 6 ")  # ZC_XZ_E_OUTPUT
    assert threw[4].startswith("bundle 1: xz status 5 ")
    assert threw[5] == "adopt: a bundle's payload is not the sum of its chunk sizes"
    assert threw[6] == "a host payload was asked for" and len(threw) == 7
    # the adopter over the device payloads = the adopter over host payloads = Python's
    for which in ("host", "device"):
        assert f"{which} chunks {rep.chunks} bytes {rep.bytes}" in lines
        assert [ln for ln in lines if ln.startswith(which + " bad ")] == \
            [f"{which} bad {ids[b].hex()} {i} {s}" for b, i, s in rep.bad]
        path = [ln for ln in lines if ln.startswith(which + " path ")][0][len(which) + 6:]
        assert open(path, "rb").read() == sidecar_bytes(rep.meta)
    # every read from the device payloads
    assert f"size {len(want)}" in lines and "fetched 0" in lines
    assert [ln for ln in lines if ln.startswith("read ")] == \
        [f"read {o} {n} {hashlib.sha256(want[o:o + n]).hexdigest()}" for o, n in reads]
