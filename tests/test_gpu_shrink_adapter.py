"""GPU test of the zbackup-side binding's GpuDeviceBackup::backup (integration/
gpu_backup_creator.hh): tests/adapter/shrink_main.cpp, compiled against the
stand-in zbackup types, backs up data that lies in HBM with its shrink passes on
the device.  The backup data, the iterations and every Writer::add -- the id and
the bytes -- equal those of the same loops over the oracle."""
import hashlib
import os
import subprocess

import pytest

from oracle import oracle
from tests.test_gpu_adapter import _expected
from tests.test_gpu_backup_device import CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "adapter")


@pytest.fixture(scope="module")
def shrink_main(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    exe = str(tmp_path_factory.mktemp("shrink") / "shrink_main")
    lib = os.path.join(ROOT, "zbackup_amd")
    # the flags of tests/adapter/build.py
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(HERE, "mock"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                    os.path.join(HERE, "shrink_main.cpp"), "-o", exe, "-L" + lib, "-lzchunk", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,$ORIGIN/../../zbackup_amd", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=["W256", "W4096"])
def test_adapter_device_backup_vs_oracle_loops(shrink_main, tmp_path, case):
    W, spec, size, _, iterations, final, _ = case
    data = oracle.gen(spec)
    inp = tmp_path / "in.bin"
    data.tofile(inp)
    out = str(tmp_path / "out")
    r = subprocess.run([shrink_main, str(W), str(inp), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want_data, want_it, want_adds, index = _expected(data, W, [])
    assert (want_it, len(want_data)) == (iterations, final)
    it, nadds, info_size = map(int, open(out + ".meta").read().split())
    assert it == want_it and info_size == size
    assert open(out + ".data", "rb").read() == want_data
    assert nadds == len(want_adds) and open(out + ".adds", "rb").read() == b"".join(want_adds)
    # the bytes of every add: the index lists the adds' sizes in order; a chunk's SHA-1 begins its id
    chunks = open(out + ".chunks", "rb").read()
    assert len(chunks) == sum(s for _, _, s in index)
    at = 0
    for blob, (_, _, s) in zip(want_adds, index):
        assert hashlib.sha1(chunks[at:at + s]).digest()[:16] == blob[:16]
        at += s
