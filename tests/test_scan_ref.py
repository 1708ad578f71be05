"""CPU: the scan's reference (tests/scan_ref.py) against the oracle's digest and
its own definition, and a check that the inputs of
tests/test_gpu_scan_outputs.py (tests/scan_cases.py) cannot pass vacuously:
every planted input holds exactly the anchors it planted, each wave-tile takes
the path its case claims, and the random input's anchors straddle the
boundaries of the scan's staging."""
import numpy as np
import pytest

from oracle import oracle
from tests import scan_cases as sc
from tests import scan_ref as sr

M64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


def test_geometry_and_rates_restate_the_header():
    src = open(sr.__file__.replace("tests/scan_ref.py", "zbackup_amd/csrc/zc_device.h")).read()
    assert "#define ZC_WLIST_CFG 144" in src and "#define ZC_LSPAN_CFG 4096" in src
    assert "#define ZC_SCAN_TPB_CFG 512" in src and "constexpr uint32_t ZC_ANCHOR_MIN_OFF = 63;" in src
    assert [sr.anchor_rate_inv(W) for W in (128, 256, 4096, 12288, 32768, 65536, 262144, 1 << 20)] == \
        [16, 16, 256, 512, 2048, 4096, 4096, 4096]
    assert sr.anchor_lo(65536) == 0x7FF0 and sr.anchor_lo(4096) == 0x7F00 and sr.anchor_lo(256) == 0x7000
    assert sr.wave_tile_cap(65536) == 192 and sr.wave_tile_cap(4096) == 2112 and sr.wave_tile_cap(12288) == 1088


def test_states_against_python_ints():
    data = sc.random_input(4096)
    st = sr.states(data)
    b = data.tolist()
    for q in list(range(0, 70)) + [1000, 4095]:
        want = sum(b[q - 2 * j] << j for j in range(16) if q - 2 * j >= 0) & 0xFFFF
        assert int(st[q]) == want, q
    pos, gear = sr.anchors(sc.random_input(1 << 20), 4096)
    st = sr.states(sc.random_input(1 << 20))
    assert pos.size > 3000 and pos.min() >= 63 and np.array_equal(pos, np.flatnonzero(sr.model_anchors(
        sc.random_input(1 << 20), 4096)))
    for q, g in list(zip(pos.tolist(), gear.tolist()))[:50]:
        assert g == int(st[q - 1]) | int(st[q]) << 16 and int(st[q]) >= 0x7F00 and int(st[q]) < 0x8000


def test_span_digests_and_grid_keys_against_the_oracle():
    data = sc.random_input(2 * sc.MIB + 1000)
    blk = sr.span_digests(data)
    assert blk.size == 2049
    for i in (0, 1, 777, 2047):
        span = data[i * 1024:(i + 1) * 1024]
        assert int(blk[i]) == (oracle.digest(span) - pow(257, 1024, 1 << 64)) & M64
    assert int(blk[2048]) == (oracle.digest(data[2048 * 1024:]) - pow(257, 1000, 1 << 64)) & M64
    assert sr.span_digests(data[:1024]).size == 1 and sr.span_digests(data[:0]).size == 0
    for W in (4096, 65536, 262144, 12288):
        keys = sr.grid_keys(data, W)
        assert keys.size == 2 * sc.MIB // W
        for i in (0, keys.size // 2, keys.size - 1):
            assert int(keys[i]) == oracle.digest(data[i * W:(i + 1) * W]), (W, i)
    assert sr.grid_keys(data[:2 * sc.MIB - 1], 65536).size == 0
    assert [W for W in sc.W_CASES if sr.scan_writes_keys(W)] == [4096, 32768, 65536, 262144]


BOUNDARIES = [16, 128, 1024, 2048, 4096, sr.WT, sr.STILE]


@pytest.mark.parametrize("W", [65536, 4096, 256])
def test_a_lone_plant_is_one_anchor_wherever_its_window_lies(W):
    for b in BOUNDARIES:
        base = 8192 + 3 * b if b < 4096 else b
        assert base % b == 0 and (b >= 4096 or base % (2 * b))
        for d in sc.EDGE_D:  # the 31-byte window [q - 30, q] lies before, across and after the boundary
            buf = np.zeros(base + 4096, dtype=np.uint8)
            g = sr.plant(buf, base + d, W)
            pos, gear = sr.anchors(buf, W)
            assert pos.tolist() == [base + d] and gear.tolist() == [g], (b, d)
    buf = np.zeros(4096, dtype=np.uint8)
    sr.plant(buf, 62, W)
    assert sr.anchors(buf, W)[0].size == 0 and sr.regime(np.concatenate([buf] * 512), W)[0] == "fast"
    buf = np.zeros(4096, dtype=np.uint8)
    sr.plant(buf, 63, W)
    assert sr.anchors(buf, W)[0].tolist() == [63]


@pytest.mark.parametrize("W", [65536, 4096, 256])
def test_plants_do_not_interfere(W):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    qs = [1000 + 64 * k for k in range(100)] + [20000 + 32 * k for k in range(100)]
    for q in qs:
        sr.plant(buf, q, W)
    assert sr.anchors(buf, W)[0].tolist() == qs
    # q and q + 1 are separate streams: two anchors in one piece
    for npairs in (96, 97):
        buf, qs, _ = sc._planted(2 * sr.STILE, {q: "" for q in sc.pairs(1, npairs)}, W)
        pos, gear = sr.anchors(buf, W)
        assert np.array_equal(pos, qs) and pos.size == 2 * npairs
        assert len({int(p) // 16 for p in pos}) == npairs
        if W == 65536:
            assert sr.regime(buf, W)[1] == ("fast" if npairs == 96 else "rescan")


@pytest.mark.parametrize("W", sc.EDGE_WS)
def test_the_edge_inputs_hold_exactly_their_plants(W):
    seen = {kind: set() for kind in list(sc.EDGE_BASES) + list(sc.EDGE_SINGLE)}
    for j in range(11):
        data, qs, plants = sc.edge_input(j, W)
        ref = sr.analyse(data, W)
        assert data.size == sc.EDGE_BYTES and np.array_equal(ref.pos, qs)
        assert qs.size == len(plants) - (j % 2)  # position 62 is planted and is no anchor
        assert np.all(np.diff(np.array(sorted(plants))) >= 64)
        assert int(qs[-1]) == data.size - 1 and (63 in plants) == (j % 2 == 0)
        for q, what in plants.items():
            kind, _, d = what.partition(" + ")
            if kind in seen:
                seen[kind].add(int(d))
        # every wave-tile of a full tile is the scan kernel's, the last one the tail's
        assert ref.regime == ["fast"] * 16 + ["tail"] and not any(ref.side_pool)
    assert all(ds == set(sc.EDGE_D) for ds in seen.values()), seen
    # the bases are what their names say, in lanes of the parity named
    for kind, bases in sc.EDGE_BASES.items():
        for b in bases:
            lane, off = b % sr.WT // sr.LSPAN, b % sr.LSPAN
            if "lane" in kind.split(",")[-1]:
                assert lane % 2 == ("odd" in kind), kind
            assert {"lane span start": off == 0, "half span start": off == sr.HALF,
                    "1 KiB boundary": off % 1024 == 0 and off % sr.HALF != 0,
                    "128 B boundary": off % 128 == 0 and off % 1024 != 0,
                    "16 B boundary": off % 16 == 0 and off % 128 != 0,
                    "wave-tile start": b % sr.WT == 0 and b % sr.STILE != 0}[kind.split(",")[0]], (kind, b)


def test_the_capacity_inputs_take_the_paths_they_claim():
    W = sc.CAP_W
    for name, (_, count, regime, side) in sc.CAP_CASES.items():
        data, qs, _ = sc.cap_input(name, False)
        ref = sr.analyse(data, W)
        assert np.array_equal(ref.pos, qs), name
        t = sc.CAP_FULL
        mine = qs[(qs >= t * sr.WT) & (qs < (t + 1) * sr.WT)]
        pieces = len({int(q) // 16 for q in mine})
        assert (pieces, mine.size) == ((count, 2 * count) if "pairs" in name else (count, count)), name
        assert ref.regime == ["fast"] * t + [regime] + ["fast"] * (15 - t) + ["tail"] * 2, name
        assert ref.side_pool == [i == t and side for i in range(18)], name
        # the neighbours hold a few plants
        assert all(((qs >= i * sr.WT) & (qs < (i + 1) * sr.WT)).sum() == 3 for i in (t - 1, t + 1))
        lanes = np.bincount((mine % sr.WT // sr.LSPAN).astype(np.int64), minlength=64)
        if "one" in name:
            assert lanes.max() == count and np.any(mine % sr.LSPAN < sr.HALF) and np.any(mine % sr.LSPAN >= sr.HALF)
        if name == "144 spread":
            assert set(lanes.tolist()) == {2, 3}
    for name, (_, count, side) in sc.CAP_TAIL_CASES.items():
        data, qs, _ = sc.cap_input(name, True)
        ref = sr.analyse(data, W)
        assert np.array_equal(ref.pos, qs), name
        assert ref.regime == ["fast"] * 16 + ["tail"] * 2
        assert ref.side_pool == [i == sc.CAP_TAIL and side for i in range(18)], name
        assert ((qs >= 16 * sr.WT) & (qs < 17 * sr.WT)).sum() == (2 * count if "pairs" in name else count)
    data, qs, _ = sc.two_overflows_input()
    assert np.array_equal(sr.anchors(data, W)[0], qs)
    assert {t for t, s in enumerate(sr.side_pool(data, W)) if s} == sc.TWO_OVERFLOWS_SIDE
    assert [sr.regime(data, W)[t] for t in (3, 4, 9, 16)] == ["rescan", "fast", "rescan", "tail"]


def test_the_grid_cap_inputs_alternate_between_fast_and_rescanned_wave_tiles():
    for n in (6 * sc.MIB, 4 * sc.MIB):
        for W in (65536, 12288):
            data, qs, _ = sc.wgs_planted_input(n, W)
            ref = sr.analyse(data, W)
            assert np.array_equal(ref.pos, qs)
            counts = np.bincount((qs // np.uint64(sr.WT)).astype(np.int64), minlength=n // sr.WT)
            assert counts.tolist() == [sc.WGS_PATTERN[t % 4] for t in range(n // sr.WT)]
            assert ref.regime == [["fast", "fast", "fast", "rescan"][t % 4] for t in range(n // sr.WT)]


def test_the_random_input_reaches_each_regime_and_each_boundary():
    data = sc.random_input(sc.W_CASE_BYTES)
    for W, want in sc.W_CASES.items():
        r = sr.regime(data, W)
        assert set(r[:24]) == want and r[24:] == ["tail"], W
    r = sr.regime(data, 32768)
    assert r.count("fast") >= 2 and r.count("rescan") >= 2  # a real mix
    # anchors whose window straddles (or starts at) a lane span, a half span, a
    # wave-tile that is not a wave's first under a capped grid; at the sparsest rate
    for n in (sc.W_CASE_BYTES, 6 * sc.MIB, 4 * sc.MIB):
        pos = sr.anchors(data[:n], 65536)[0].astype(np.int64)
        lane = pos[(pos % sr.LSPAN <= 30) & (pos % sr.WT > 30)]
        half = pos[(pos % sr.LSPAN >= sr.HALF) & (pos % sr.LSPAN <= sr.HALF + 30)]
        wt = pos[(pos % sr.WT <= 30) & (pos >= 12 * sr.WT)]
        assert lane.size >= 2 and half.size >= 1 and wt.size >= 1, (n, lane.size, half.size, wt.size)
        assert {int(p) % sr.WT // sr.LSPAN % 2 for p in lane} == {0, 1}  # in even and odd lanes
    # the lengths' inputs: an anchor in the tail of 4 MiB + 300 KiB + 17, none below 64 KiB
    pos = sr.anchors(sc.random_input(sc.LENGTHS[-1]), 65536)[0]
    assert (pos >= 4 * sc.MIB).sum() >= 20 and (pos >= 4 * sc.MIB + sr.WT).sum() >= 1
    assert sc.LENGTHS[-1] == 4 * sc.MIB + 300 * 1024 + 17
