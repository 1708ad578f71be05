"""GPU: every word the scan leaves behind, read out with zc_debug_scan_outputs
(BackupCreator.scan_outputs) and compared with tests/scan_ref.py: all span
digests, every wave-tile's anchor positions and gear words in order, which pool
its directory entry points into, the scan-written grid keys, and the anchor
count of zc_stats.  Nothing is sampled.

The inputs (tests/scan_cases.py; tests/test_scan_ref.py pins on the CPU what
they reach) are a few MiB each: lengths around every boundary of the geometry,
chunk sizes that send the wave-tiles down each path (the scan kernel's own tile
end stores anchors only from W = 32 KiB up on random bytes; below, every full
wave-tile overflows its list and is rescanned), planted anchors at every kind of
boundary of the staging, the list's and the pool share's capacity edges, and --
with ZC_TEST_SCAN_WGS, which caps the scan's grid -- waves that walk several
wave-tiles, which otherwise takes a stream of more than 512 MiB."""
import ctypes

import numpy as np
import pytest

from tests import scan_cases as sc
from tests import scan_ref as sr
from zbackup_amd import _lib

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


def run_stream(torch, bc, data, via="device"):
    """One stream through `bc`; returns (scan outputs, stats, path bits)."""
    data = np.array(data, dtype=np.uint8)  # a writable, contiguous copy
    if via == "device":
        t = torch.from_numpy(data).to("cuda")
        bc.chunk_device(t.data_ptr(), data.size)
    else:
        bc.chunk_host(data.ctypes.data, data.size)
    return bc.scan_outputs(), bc.stats(), bc.last_paths()


def one_stream(torch, data, W, via="device"):
    from zbackup_amd import BackupCreator
    with BackupCreator(W, sha1=False) as bc:
        return run_stream(torch, bc, data, via)


def _first_diff(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(a[:m] != b[:m])
    return int(d[0]) if d.size else m


def check_outputs(res, data, W, expect_keys=None):
    """Every word of `res` against the reference.  expect_keys: the key count
    the case demands (None: whatever the hook reports is compared)."""
    out, stats, _ = res
    data = np.asarray(data, dtype=np.uint8)
    n = data.size
    assert out["n"] == n
    # span digests
    want_blk = sr.span_digests(data)
    assert out["blk"].size == want_blk.size == -(-n // sr.SPAN)
    if not np.array_equal(out["blk"], want_blk):
        i = _first_diff(out["blk"], want_blk)
        pytest.fail(f"span digest {i} is {int(out['blk'][i]):#x}, the reference gives {int(want_blk[i]):#x}; "
                    f"the span starts at {sr.where(i * sr.SPAN)}")
    # anchors, wave-tile by wave-tile
    ref = sr.analyse(data, W)
    pos, gear, side, regimes = ref.pos, ref.gear, ref.side_pool, ref.regime
    nwt = -(-n // sr.WT)
    assert out["wt_count"].size == out["wt_side"].size == nwt
    edges = np.searchsorted(pos, np.arange(nwt + 1, dtype=np.uint64) * np.uint64(sr.WT))
    got_edges = np.concatenate([[0], np.cumsum(out["wt_count"].astype(np.int64))])
    assert out["anchor_pos"].size == out["anchor_gear"].size == got_edges[-1]
    for t in range(nwt):
        gp = out["anchor_pos"][got_edges[t]:got_edges[t + 1]]
        gg = out["anchor_gear"][got_edges[t]:got_edges[t + 1]]
        wp, wg = pos[edges[t]:edges[t + 1]], gear[edges[t]:edges[t + 1]]
        if not np.array_equal(gp, wp):
            i = _first_diff(gp, wp)
            got = sr.where(gp[i]) if i < gp.size else "nothing"
            want = sr.where(wp[i]) if i < wp.size else "nothing"
            pytest.fail(f"wave-tile {t} ({regimes[t]}): {gp.size} anchors, the reference has {wp.size}; entry {i} "
                        f"is {got}, the reference has {want}")
        if not np.array_equal(gg, wg):
            i = _first_diff(gg, wg)
            pytest.fail(f"wave-tile {t} ({regimes[t]}): gear word {int(gg[i]):#010x} at entry {i}, the reference "
                        f"gives {int(wg[i]):#010x}; {sr.where(wp[i])}")
        assert bool(out["wt_side"][t]) == side[t], \
            f"wave-tile {t} ({regimes[t]}, {wp.size} anchors): side-pool flag {out['wt_side'][t]}"
    assert stats["anchors"] == pos.size == int(out["wt_count"].sum())
    # grid keys
    if expect_keys is not None:
        assert out["keys"].size == expect_keys, (out["keys"].size, expect_keys, stats["epochs"])
    if out["keys"].size:
        assert sr.scan_writes_keys(W) and stats["epochs"] == 1
        want = sr.grid_keys(data, W)
        assert out["keys"].size == want.size == n // sr.STILE * sr.STILE // W
        if not np.array_equal(out["keys"], want):
            i = _first_diff(out["keys"], want)
            pytest.fail(f"grid key {i} is {int(out['keys'][i]):#x}, the reference gives {int(want[i]):#x}; "
                        f"the chunk starts at {sr.where(i * W)}")
    return regimes


def scan_key_count(n, W):
    return n // sr.STILE * sr.STILE // W if sr.scan_writes_keys(W) and n >= W else 0


# ---------------------------------------------------------------- lengths
@pytest.mark.parametrize("via", ["device", "host"])
@pytest.mark.parametrize("n", sc.LENGTHS)
def test_lengths(torch_cuda, n, via):
    data = sc.random_input(n)
    res = one_stream(torch_cuda, data, 65536, via)
    # random bytes match nothing: one epoch, so the scan's keys are all there
    check_outputs(res, data, 65536, expect_keys=scan_key_count(n, 65536))
    assert res[0]["max_tiles_per_wave"] == (1 if n >= sr.STILE else 0)


@pytest.mark.parametrize("via", ["device", "host"])
def test_empty_stream(torch_cuda, via):
    out, stats, _ = one_stream(torch_cuda, np.zeros(0, dtype=np.uint8), 65536, via)
    assert out["n"] == 0 and stats["anchors"] == 0 and out["max_tiles_per_wave"] == 0
    assert all(out[k].size == 0 for k in ("blk", "wt_count", "wt_side", "anchor_pos", "anchor_gear", "keys"))


def test_host_stream_scanned_in_two_launches(torch_cuda):
    """zc_chunk_host scans each 64 MiB segment as it lands: the second launch
    starts at tile 32 (wave-tile 256).  The first segment is zeros (no anchors,
    every digest 0, whatever its length), so the reference is computed over the
    rest, with the 64 bytes before it for the anchors' windows."""
    seg, n = 64 * MIB, 64 * MIB + 2 * MIB + 300 * 1024 + 5
    data = np.zeros(n, dtype=np.uint8)
    data[seg:] = sc.random_input(n - seg)
    out, stats, _ = one_stream(torch_cuda, data, 65536, "host")
    assert out["n"] == n and not out["blk"][:seg // sr.SPAN].any() and not out["wt_count"][:seg // sr.WT].any()
    pos, gear = sr.anchors(data[seg - 64:], 65536)
    pos += np.uint64(seg - 64)
    assert np.array_equal(out["anchor_pos"], pos), sr.where(pos[_first_diff(out["anchor_pos"], pos)])
    assert np.array_equal(out["anchor_gear"], gear)
    assert np.array_equal(out["blk"][seg // sr.SPAN:], sr.span_digests(data[seg:]))
    assert not out["wt_side"].any() and stats["anchors"] == pos.size
    # 256 wave-tiles on the grid of the first launch: still one per wave
    assert out["max_tiles_per_wave"] == 1


# ---------------------------------------------------------------- chunk sizes
@pytest.mark.parametrize("W", list(sc.W_CASES))
def test_chunk_sizes(torch_cuda, W):
    data = sc.random_input(sc.W_CASE_BYTES)
    res = one_stream(torch_cuda, data, W)
    nk = scan_key_count(data.size, W)
    regimes = check_outputs(res, data, W, expect_keys=nk)
    assert set(regimes[:data.size // sr.STILE * 8]) == sc.W_CASES[W]
    if 4096 <= W <= 262144 and sr.WT % W == 0:
        assert nk == data.size // sr.STILE * sr.STILE // W and res[2] & _lib.ZC_PATH_SCAN_KEYS
    else:
        assert nk == 0 and not res[2] & _lib.ZC_PATH_SCAN_KEYS


# ---------------------------------------------------------------- planted edges
@pytest.mark.parametrize("W", sc.EDGE_WS)
@pytest.mark.parametrize("j", range(11))
def test_planted_edges(torch_cuda, j, W):
    data, qs, plants = sc.edge_input(j, W)
    out = one_stream(torch_cuda, data, W)
    try:
        check_outputs(out, data, W)
    except BaseException:
        got = set(out[0]["anchor_pos"].tolist())
        for q in qs.tolist():
            if q not in got:
                print(f"missing plant: {plants[q]}; {sr.where(q)}")
        raise
    assert np.array_equal(out[0]["anchor_pos"], qs)


# ---------------------------------------------------------------- capacity edges
@pytest.mark.parametrize("name", list(sc.CAP_CASES))
def test_capacity_in_a_full_tile(torch_cuda, name):
    data, qs, _ = sc.cap_input(name, False)
    res = one_stream(torch_cuda, data, sc.CAP_W)
    regimes = check_outputs(res, data, sc.CAP_W)
    _, _, regime, side = sc.CAP_CASES[name]
    assert regimes[sc.CAP_FULL] == regime and bool(res[0]["wt_side"][sc.CAP_FULL]) == side
    assert int(res[0]["wt_side"].sum()) == int(side)


@pytest.mark.parametrize("name", list(sc.CAP_TAIL_CASES))
def test_capacity_in_the_tail(torch_cuda, name):
    data, qs, _ = sc.cap_input(name, True)
    res = one_stream(torch_cuda, data, sc.CAP_W)
    check_outputs(res, data, sc.CAP_W)
    side = sc.CAP_TAIL_CASES[name][2]
    assert bool(res[0]["wt_side"][sc.CAP_TAIL]) == side and int(res[0]["wt_side"].sum()) == int(side)


def test_two_overflowed_wave_tiles_share_the_side_pool(torch_cuda):
    data, qs, _ = sc.two_overflows_input()
    res = one_stream(torch_cuda, data, sc.CAP_W)
    check_outputs(res, data, sc.CAP_W)
    assert set(np.flatnonzero(res[0]["wt_side"]).tolist()) == sc.TWO_OVERFLOWS_SIDE


# ---------------------------------------------------------------- several wave-tiles per wave
def _wgs_stream(torch, monkeypatch, knob, data, W):
    from zbackup_amd import BackupCreator
    if knob is None:
        monkeypatch.delenv("ZC_TEST_SCAN_WGS", raising=False)
    else:
        monkeypatch.setenv("ZC_TEST_SCAN_WGS", str(knob))
    with BackupCreator(W, sha1=False) as bc:  # zc_create reads the knob
        monkeypatch.delenv("ZC_TEST_SCAN_WGS", raising=False)
        return run_stream(torch, bc, data)


@pytest.mark.parametrize("W", [65536, 12288])
@pytest.mark.parametrize("n", [6 * MIB, 4 * MIB])
@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("k", [1, 3])
def test_waves_walk_several_wave_tiles(torch_cuda, monkeypatch, k, kind, n, W):
    data = sc.random_input(n) if kind == "random" else sc.wgs_planted_input(n, W)[0]
    res = _wgs_stream(torch_cuda, monkeypatch, k, data, W)
    # (a planted stream's zero chunks match each other: more epochs, keys not reported)
    regimes = check_outputs(res, data, W, expect_keys=scan_key_count(n, W) if kind == "random" else None)
    # wave-tiles of 4 waves per workgroup: the most one wave walks
    assert res[0]["max_tiles_per_wave"] == -(-(n // sr.WT) // (4 * k)) >= 2
    if (k, n) == (1, 6 * MIB):
        assert res[0]["max_tiles_per_wave"] == 6
    if kind == "planted":
        assert regimes == [["fast", "fast", "fast", "rescan"][t % 4] for t in range(n // sr.WT)]
    # the knob is the cause
    assert _wgs_stream(torch_cuda, monkeypatch, None, data, W)[0]["max_tiles_per_wave"] == 1


@pytest.mark.parametrize("value", ["0", "-1", "zz", "3x", "", "100000"])
def test_an_invalid_grid_cap_is_ignored(torch_cuda, monkeypatch, value):
    data = sc.random_input(4 * MIB)
    res = _wgs_stream(torch_cuda, monkeypatch, value, data, 65536)
    assert res[0]["max_tiles_per_wave"] == 1
    assert np.array_equal(res[0]["anchor_pos"], sr.anchors(data, 65536)[0])


# ---------------------------------------------------------------- one context, several streams
@pytest.mark.parametrize("W", [65536, 32768])
def test_three_streams_on_one_context(torch_cuda, W):
    """6 MiB, 2 MiB + 1, 6 MiB on one context, each compared after its own call:
    the shorter stream reuses the longer one's pool, side pool and directory (at
    W = 32 KiB some wave-tiles are rescanned into the side pool)."""
    from zbackup_amd import BackupCreator
    rnd = sc.random_bytes()
    streams = [rnd[:6 * MIB], rnd[6 * MIB:8 * MIB + 1], rnd[2 * MIB:8 * MIB]]
    with BackupCreator(W, sha1=False) as bc:
        for data in streams:
            res = run_stream(torch_cuda, bc, data)
            check_outputs(res, data, W, expect_keys=scan_key_count(data.size, W))
            bc.reset()


# ---------------------------------------------------------------- the hook's refusals
def test_hook_refusals(torch_cuda):
    from zbackup_amd import BackupCreator
    data = sc.random_input(2 * MIB + 1)
    with BackupCreator(65536, sha1=False) as bc:
        L, ctx = bc._L, bc._ctx
        o = _lib.ZcScanOutputs()
        # before any stream
        assert L.zc_debug_scan_outputs(ctx, ctypes.byref(o)) == _lib.ZC_ERR_STATE
        assert b"no stream" in L.zc_last_error(ctx)
        with pytest.raises(_lib.ZcError):
            bc.scan_outputs()
        # null pointers
        assert L.zc_debug_scan_outputs(ctx, None) == _lib.ZC_ERR_ARG
        assert L.zc_debug_scan_outputs(None, ctypes.byref(o)) == _lib.ZC_ERR_ARG
        out, stats, _ = run_stream(torch_cuda, bc, data)
        assert L.zc_debug_scan_outputs(ctx, None) == _lib.ZC_ERR_ARG
        # too little room: the counts needed come back
        o = _lib.ZcScanOutputs()
        assert L.zc_debug_scan_outputs(ctx, ctypes.byref(o)) == _lib.ZC_ERR_ARG
        assert b"too small" in L.zc_last_error(ctx)
        assert (o.n, o.n_blk, o.n_wt, o.n_anchors, o.n_keys) == (data.size, 2049, 9, stats["anchors"], 32)
        blk = np.zeros(o.n_blk - 1, dtype=np.uint64)
        o.blk, o.blk_cap = blk.ctypes.data, blk.size
        assert L.zc_debug_scan_outputs(ctx, ctypes.byref(o)) == _lib.ZC_ERR_ARG
        assert not blk.any() and o.n_blk == 2049  # nothing written
        # room without an array
        o = _lib.ZcScanOutputs()
        o.blk_cap = o.wt_cap = o.anchor_cap = o.key_cap = 1 << 20
        assert L.zc_debug_scan_outputs(ctx, ctypes.byref(o)) == _lib.ZC_ERR_ARG
        # kept across zc_reset
        bc.reset()
        again = bc.scan_outputs()
        assert all(np.array_equal(again[k], out[k]) for k in out)


def test_hook_refuses_a_windowed_stream(torch_cuda):
    from zbackup_amd import BackupCreator
    data = sc.random_input(2 * MIB + 1)
    with BackupCreator(65536, sha1=False, window=32 * MIB) as bc:
        bc.feed(data)
        bc.finish()
        o = _lib.ZcScanOutputs()
        assert bc._L.zc_debug_scan_outputs(bc._ctx, ctypes.byref(o)) == _lib.ZC_ERR_STATE
        assert b"feed window" in bc._L.zc_last_error(bc._ctx)
    # the whole stream kept in HBM (window 0) is resolved as zc_chunk_device resolves it
    with BackupCreator(65536, sha1=False, window=0) as bc:
        bc.feed(data)
        bc.finish()
        check_outputs((bc.scan_outputs(), bc.stats(), bc.last_paths()), data, 65536, expect_keys=32)
