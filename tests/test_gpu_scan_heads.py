"""GPU: anchors in the first 32 positions of a half lane span (the two "head"
pieces), whose anchor state depends on bytes of the neighbouring lane, of the
lane's own other half or of the previous wave-tile -- wherever the scan takes
those bytes from, every output word must equal tests/scan_ref.py's.

The plants sit at offsets 0 .. 32 behind every kind of half boundary, in the
smallest stream in which the scan kernel's own tile end runs (two full 2 MiB
tiles and a tail).  What the inputs reach is asserted on the CPU model first, so
no case can pass through the exact rescan: all 16 full wave-tiles are "fast"."""
import functools

import numpy as np
import pytest

from tests import scan_cases as sc
from tests import scan_ref as sr
from tests.test_gpu_scan_outputs import check_outputs, one_stream, scan_key_count, torch_cuda  # noqa: F401

MIB = 1 << 20
HEAD_BYTES = 4 * MIB + 256 * 1024
HEAD_LANES = [0, 1, 2, 31, 32, 62, 63]
HEAD_WS = [65536, 32768]


@functools.lru_cache(maxsize=None)
def heads_input(j, W):
    """(data, the planted positions that are anchors).  In wave-tile t the
    plants lie d bytes behind the start of both halves of the lanes above; for
    d < 14 the plant's bytes lie before the boundary."""
    buf = np.zeros(HEAD_BYTES, dtype=np.uint8)
    qs = []
    for t in range(17):
        d = 16 * j + t if 16 * j + t <= 32 else (2 * t) % 33
        for lane in HEAD_LANES:
            for off in (0, sr.HALF):
                q = t * sr.WT + lane * sr.LSPAN + off + d
                if q < 14:
                    continue
                sr.plant(buf, q, W)
                qs.append(q)
    buf.setflags(write=False)
    return buf, np.array(sorted(q for q in qs if q >= sr.MIN_OFF), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def heads_ref(j, W):
    data, _ = heads_input(j, W)
    return sr.analyse(data, W)


@pytest.mark.parametrize("W", HEAD_WS)
@pytest.mark.parametrize("j", range(3))
def test_planted_heads_model(j, W):
    """What the planted streams reach, on the CPU model."""
    data, qs = heads_input(j, W)
    ref = heads_ref(j, W)
    assert qs.size == 237 and np.array_equal(ref.pos, qs)  # all lone
    assert ref.regime == ["fast"] * 16 + ["tail"] and not any(ref.side_pool)
    # every offset 0 .. 32 is used by some stream (checked once)
    if j == 0:
        ds = set()
        for jj in range(3):
            ds |= {int(q) % sr.HALF for q in heads_input(jj, W)[1] if int(q) % sr.HALF <= 32}
        assert ds == set(range(33))


@pytest.mark.gpu
@pytest.mark.parametrize("W", HEAD_WS)
@pytest.mark.parametrize("j", range(3))
def test_planted_heads(torch_cuda, j, W):  # noqa: F811
    data, qs = heads_input(j, W)
    ref = heads_ref(j, W)
    assert ref.regime == ["fast"] * 16 + ["tail"] and np.array_equal(ref.pos, qs) and qs.size == 237
    res = one_stream(torch_cuda, data, W)
    regimes = check_outputs(res, data, W)
    assert regimes == ["fast"] * 16 + ["tail"]
    assert np.array_equal(res[0]["anchor_pos"], qs)
    assert not res[0]["wt_side"].any()


# --- capacity with heads: head pieces count into the list's 144 ---------------------
CAP_HEAD_WT = 3
# (head pieces, ordinary pieces) -> (regime, anchors)
CAP_HEAD_CASES = {(127, 17): ("fast", 144), (128, 16): ("fast", 144), (128, 17): ("rescan", None),
                  (128, 0): ("fast", 128)}


@functools.lru_cache(maxsize=None)
def cap_heads_input(heads, ordinary):
    buf = np.zeros(sc.CAP_BYTES, dtype=np.uint8)
    t0 = CAP_HEAD_WT * sr.WT
    pairs = [(lane, off) for lane in range(64) for off in (0, sr.HALF)]
    qs = [t0 + lane * sr.LSPAN + off + (15 if lane & 1 else 31) for lane, off in pairs[:heads]]
    qs += [t0 + i * sr.LSPAN + 1024 + 15 for i in range(ordinary)]
    for q in qs:
        sr.plant(buf, q, sc.CAP_W)
    buf.setflags(write=False)
    return buf, np.array(sorted(qs), dtype=np.uint64)


@pytest.mark.parametrize("case", list(CAP_HEAD_CASES))
def test_capacity_with_heads_model(case):
    data, qs = cap_heads_input(*case)
    ref = sr.analyse(data, sc.CAP_W)
    regime, count = CAP_HEAD_CASES[case]
    assert np.array_equal(ref.pos, qs) and qs.size == sum(case)
    assert ref.regime[CAP_HEAD_WT] == regime and ref.side_pool[CAP_HEAD_WT] == (regime == "rescan")
    assert count is None or count == qs.size
    # (CAP_BYTES ends 100 bytes into an 18th wave-tile)
    assert [r for t, r in enumerate(ref.regime) if t != CAP_HEAD_WT] == ["fast"] * 15 + ["tail"] * 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CAP_HEAD_CASES))
def test_capacity_with_heads(torch_cuda, case):  # noqa: F811
    data, qs = cap_heads_input(*case)
    regime, _ = CAP_HEAD_CASES[case]
    res = one_stream(torch_cuda, data, sc.CAP_W)
    regimes = check_outputs(res, data, sc.CAP_W)  # (the side-pool flag of every wave-tile included)
    assert regimes[CAP_HEAD_WT] == regime
    assert bool(res[0]["wt_side"][CAP_HEAD_WT]) == (regime == "rescan")
    assert int(res[0]["wt_side"].sum()) == int(regime == "rescan")
    assert np.array_equal(res[0]["anchor_pos"], qs)


# --- random bytes ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("via", ["device", "host"])
@pytest.mark.parametrize("W", HEAD_WS)
def test_random_bytes(torch_cuda, W, via):  # noqa: F811
    data = sc.random_input(6 * MIB)
    res = one_stream(torch_cuda, data, W, via)
    check_outputs(res, data, W, expect_keys=scan_key_count(data.size, W))
