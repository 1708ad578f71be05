"""GPU: the scan's waves claim their wave-tiles after the first from one device
counter that is never cleared between launches.  Whichever wave takes a
wave-tile, every output word must equal tests/scan_ref.py's: with the grid
capped (ZC_TEST_SCAN_WGS) so that a wave walks 2 .. 10 wave-tiles and the
wave-tile count is no multiple of the wave count; over several streams on one
context (the claim base carries from launch to launch, through streams with one
tile and with no scan launch at all); and over a windowed feed, which makes
several scan launches per stream."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import scan_cases as sc
from tests import scan_ref as sr
from tests.test_gpu_scan_outputs import (_wgs_stream, check_outputs, run_stream, scan_key_count,  # noqa: F401
                                         torch_cuda)
from tests.test_gpu_window import _feed, _same

pytestmark = pytest.mark.gpu

MIB = 1 << 20
W = 65536


@functools.lru_cache(maxsize=None)
def random_10mib():
    """(tests/scan_cases.py's random bytes end at 8 MiB + 300 KiB)"""
    oracle.build()
    buf = oracle.splitmix64(10 * MIB + 5, 12)
    buf.setflags(write=False)
    return buf


def random_input(n):
    return sc.random_input(n) if n <= sc.RANDOM_BYTES else random_10mib()[:n]


# ---------------------------------------------------------------- grid cap
@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("n", [6 * MIB, 10 * MIB + 5])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_claimed_wave_tiles_under_a_grid_cap(torch_cuda, monkeypatch, k, n, kind):  # noqa: F811
    data = random_input(n) if kind == "random" else sc.wgs_planted_input(n, W)[0]
    assert data.size == n
    res = _wgs_stream(torch_cuda, monkeypatch, k, data, W)
    # (a planted stream's zero chunks match each other: more epochs, keys not reported)
    regimes = check_outputs(res, data, W, expect_keys=scan_key_count(n, W) if kind == "random" else None)
    nwt = n // sr.STILE * 8  # the scan kernel's wave-tiles: 24 and 40, on 4 k waves
    assert res[0]["max_tiles_per_wave"] == -(-nwt // (4 * k)) >= 2
    if kind == "planted":
        assert regimes[:nwt] == [["fast", "fast", "fast", "rescan"][t % 4] for t in range(nwt)]


# ---------------------------------------------------------------- one context, several streams
def test_five_streams_on_one_context(torch_cuda):  # noqa: F811
    """6 MiB (24 wave-tiles claimed), 2 MiB + 1 (one tile), 300 KiB (no scan
    launch), 10 MiB, and 6 MiB through the host path: each compared after its
    own call."""
    from zbackup_amd import BackupCreator
    rnd = sc.random_bytes()
    streams = [(rnd[:6 * MIB], "device"), (rnd[6 * MIB:8 * MIB + 1], "device"), (rnd[MIB:MIB + 300 * 1024], "device"),
               (random_input(10 * MIB), "device"), (rnd[2 * MIB:8 * MIB], "host")]
    with BackupCreator(W, sha1=False) as bc:
        for data, via in streams:
            res = run_stream(torch_cuda, bc, data, via)
            check_outputs(res, data, W, expect_keys=scan_key_count(data.size, W))
            bc.reset()


# ---------------------------------------------------------------- windowed feed
def test_windowed_feed_then_a_device_stream(torch_cuda):  # noqa: F811
    """The feed window scans as the stream arrives, several launches per
    stream; the device stream behind it starts from the base those left."""
    from zbackup_amd import BackupCreator
    oracle.build()
    data = oracle.gen("R61:30000000,C777:5000000,Z:1000000,R62:6000000")
    want = oracle.chunk_array(data, W)
    want["sha1"][:] = 0
    rng = np.random.default_rng(61)
    with BackupCreator(W, sha1=False, window=1) as bc:  # the smallest window: 8 W + 16 MiB
        got, _ = _feed(bc, data, rng, 3 << 20)
        assert bc.stats()["segments"] >= 2
        _same(got, want)
        bc.reset()
        dev = sc.random_input(6 * MIB)
        t = torch_cuda.from_numpy(np.array(dev, dtype=np.uint8)).to("cuda")
        bc.chunk_device(t.data_ptr(), dev.size)
        got_dev = bc.records()
    want_dev = oracle.chunk_array(dev, W)
    want_dev["sha1"][:] = 0
    _same(got_dev, want_dev)
