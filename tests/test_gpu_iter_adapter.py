"""GPU test of the zbackup-side binding's GpuBackupRestorer::restoreIterations
(integration/gpu_backup_creator.hh): tests/adapter/iter_main.cpp, compiled
against the stand-in zbackup types, restores the three-iteration repository of
tests/test_gpu_restore_device.py from its index files and payload files, and a
chunk no bundle holds comes back under the reference's exception name."""
import os
import subprocess

import numpy as np
import pytest

from tests.instr_cases import ser
from tests.test_gpu_restore_device import USER_BYTES, Repo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")
KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d7781")


@pytest.fixture(scope="module")
def iter_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("iter") / "iter_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    # the flags of tests/adapter/build.py
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "iter_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,$ORIGIN/../../zbackup_amd", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def test_adapter_restores_three_iterations(iter_main, tmp_path):
    from zbackup_amd import write_index
    from zbackup_amd.bundle import BundleCompressor
    repo = Repo(3)
    rng = np.random.default_rng(71)
    bundle_ids = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in repo.bundles]
    cut = len(repo.bundles) // 2
    with BundleCompressor() as comp:
        files = [write_index(list(zip(bundle_ids[a:b], repo.bundles[a:b])), key=KEY,
                             r=bytes(rng.integers(0, 256, 16, dtype=np.uint8)), comp=comp)
                 for a, b in ((0, cut), (cut, len(repo.bundles)))]
    names = []
    for k, f in enumerate(files):
        (tmp_path / f"index{k}").write_bytes(f)
        names.append(str(tmp_path / f"index{k}"))
    pay = tmp_path / "payloads"
    pay.mkdir()
    for bid, p in zip(bundle_ids, repo.payloads):
        (pay / bid.hex()).write_bytes(p)

    def run(stream, iterations):
        (tmp_path / "backup").write_bytes(stream)
        out = subprocess.run([iter_main, KEY.hex(), str(tmp_path / "backup"), str(iterations), str(pay),
                              str(tmp_path / "out")] + names, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")

    lines = run(repo.streams[3], 3)
    assert f"restored {USER_BYTES}" in lines
    assert (tmp_path / "out").read_bytes() == repo.user
    want = [len(repo.streams[2]), len(repo.streams[1]), len(repo.streams[0]), USER_BYTES]
    assert [ln for ln in lines if ln.startswith("round ")] == [f"round {k} {n}" for k, n in enumerate(want)]
    fetched = [ln.split()[1] for ln in lines if ln.startswith("fetched ")]
    assert len(fetched) == len(set(fetched))  # the shared bundle crossed once although two rounds use it
    assert bundle_ids[repo.shared].hex() in fetched
    # iteration 1's stream with a chunk no bundle holds
    gone = bytes(range(200, 224))
    lines = run(repo.streams[1] + ser(chunk_blob=gone), 1)
    assert lines[0] == f"exNoSuchChunk chunk {gone.hex()} is in no bundle of the index"
