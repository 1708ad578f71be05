"""GPU test of the zbackup-side binding's GpuXzBundleCompressor (integration/
gpu_backup_creator.hh): tests/adapter/xzenc_main.cpp, compiled against the
stand-in zbackup types, compresses a batch of payloads, decodes the bodies
with GpuXzBundleDecoder::decodeAll and compares; here the bodies are also held
to Python's lzma and to BundleCompressor.compress_xz_host."""
import lzma
import os
import struct
import subprocess

import pytest

from tests import xz_inputs as XI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")


@pytest.fixture(scope="module")
def xzenc_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("xzenc_adapter") / "xzenc_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "xzenc_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


def test_compressor_round_trips_through_the_decoder(xzenc_main, tmp_path):
    from zbackup_amd.bundle import BundleCompressor
    payloads = [XI.payload(kind, n, 60 + j).tobytes() for j, (kind, n) in enumerate(
        (("text", 70001), ("halfdup", 33000), ("random", 9000), ("zeros", 0), ("period65", 1), ("random", 65537),
         ("alphabet4", 200000)))]
    (tmp_path / "payloads").write_bytes(struct.pack("<I", len(payloads)) +
                                        b"".join(struct.pack("<Q", len(p)) + p for p in payloads))
    out = subprocess.run([xzenc_main, str(tmp_path / "payloads"), str(tmp_path / "bodies")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert f"compressAll ok {len(payloads)}" in lines and "compress ok" in lines
    assert f"decodeAll ok {len(payloads)}" in lines
    blob = (tmp_path / "bodies").read_bytes()
    assert struct.unpack_from("<I", blob)[0] == len(payloads)
    pos, bodies = 4, []
    for _ in payloads:
        n = struct.unpack_from("<Q", blob, pos)[0]
        bodies.append(blob[pos + 8:pos + 8 + n])
        pos += 8 + n
    assert pos == len(blob)
    for p, b in zip(payloads, bodies):
        assert lzma.decompress(b) == p and b[7] == 4
    with BundleCompressor() as bc:
        assert bc.compress_xz_host(payloads) == bodies
