"""GPU tests of the device instruction parse (zc_parse_instructions_device):
every stream of tests/instr_cases.py is compared with zc_parse_instructions, the
host parser.  A valid stream matches record for record, 48 bytes each; an
invalid one gives the same text after the function's name."""
import ctypes
import os

import numpy as np
import pytest

from tests import instr_cases as C

pytestmark = pytest.mark.gpu

NAME = "zc_parse_instructions_device: "


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


@pytest.fixture(scope="module")
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


def set_tile(tile):
    if tile is None:
        os.environ.pop("ZC_TEST_INSTR_TILE", None)
    else:
        os.environ["ZC_TEST_INSTR_TILE"] = str(tile)


@pytest.fixture(autouse=True)
def restore_tile():
    old = os.environ.get("ZC_TEST_INSTR_TILE")
    yield
    set_tile(old)


def device_parse(torch, comp, data, tile):
    """("ok", records as bytes, n_messages, bytes_total) or ("error", text)."""
    L, ctx = comp._L, comp._ctx
    set_tile(tile)
    t = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).to("cuda:0")
    handle = ctypes.c_void_p(1)
    rc = L.zc_parse_instructions_device(ctx, t.data_ptr() if data else None, len(data), ctypes.byref(handle))
    if rc != 0:
        assert rc == -1 and not handle.value  # ZC_ERR_ARG, *out NULL
        msg = L.zc_last_error(ctx).decode()
        assert msg.startswith(NAME), msg
        return "error", msg[len(NAME):]
    try:
        c = [ctypes.c_uint64() for _ in range(3)]
        assert L.zc_instr_set_counts(handle, *[ctypes.byref(x) for x in c]) == 0
        n = c[0].value
        out = np.zeros(48 * n + 1, dtype=np.uint8)
        assert L.zc_instr_set_fetch(handle, 0, n, out.ctypes.data if n else None) == 0
        return "ok", out[:48 * n].tobytes(), c[1].value, c[2].value
    finally:
        L.zc_instr_set_destroy(handle)


def check(torch, comp, name, data, tile):
    want = C.host_parse(comp._L, data)
    got = device_parse(torch, comp, data, tile)
    assert got[0] == want[0], (name, got[:2] if got[0] == "error" else got[0], want[1][:200])
    if want[0] == "error":
        assert got[1] == want[1], name
        return got
    if got[1] != want[1]:
        g, w = (np.frombuffer(x, dtype=np.uint8) for x in (got[1], want[1]))
        assert len(g) == len(w), f"{name}: {len(g) // 48} entries, expected {len(w) // 48}"
        at = int(np.nonzero(g != w)[0][0])
        raise AssertionError(f"{name}: entry {at // 48} differs at its byte {at % 48}")
    return got


@pytest.mark.parametrize("group", [C.basic, C.malformed_placed, C.geometry, C.phantoms],
                         ids=lambda f: f.__name__)
def test_named_streams(torch_cuda, comp, group):
    for name, data, tile in group():
        got = check(torch_cuda, comp, name, data, tile)
        if name.startswith("phantom cut"):
            assert got[0] == "error" and "instruction length past the end" in got[1]
        elif name.startswith("phantom"):
            assert got[0] == "ok"


def test_phantom_payloads_add_no_entries(torch_cuda, comp):
    """The entries of a stream with a message-like payload are those of the
    stream with a payload of as many plain bytes."""
    for name, payload in C.phantom_payloads():
        a = device_parse(torch_cuda, comp, C.good(3) + C.ser(raw=payload) + C.good(20, seed=2), C.T)
        b = device_parse(torch_cuda, comp, C.good(3) + C.ser(raw=b"." * len(payload)) + C.good(20, seed=2), C.T)
        assert a == b and a[0] == "ok", name


@pytest.mark.parametrize("name,data,tile", C.zeros(), ids=[c[0] for c in C.zeros()])
def test_all_zero_streams(torch_cuda, comp, name, data, tile):
    """Every position is an empty message: no entries, the longest chain a tile can hold."""
    got = check(torch_cuda, comp, name, data, tile)
    assert got == ("ok", b"", len(data), 0)
    from zbackup_amd import Restorer
    with Restorer(ctx=comp._ctx) as r:
        st = r.parse_last_stats()
    assert st["tiles"] == 3 and st["chain_hops"] == 3


def test_counts_and_stats(torch_cuda, comp):
    data = C.good(3000, seed=5)
    got = check(torch_cuda, comp, "good 3000", data, C.T)
    assert got[2] == 3000 and len(got[1]) == 48 * 3000  # r = 3 gives two entries, r = 4 none
    from zbackup_amd import Restorer
    with Restorer(ctx=comp._ctx) as r:
        st = r.parse_last_stats()
    tiles = (len(data) + C.T - 1) // C.T
    assert st["tiles"] == tiles > 256 and 0 < st["chain_hops"] <= tiles
    assert st["hop_ms"] == 0 and st["exit_ms"] > 0 and st["chain_ms"] > 0 and st["emit_ms"] > 0
    ins = np.frombuffer(got[1], dtype=np.dtype([("kind", "<u4"), ("id", "u1", (24,)), ("r", "<u4"),
                                                ("data_off", "<u8"), ("size", "<u8")]))
    assert got[3] == int(ins["size"][ins["kind"] == 1].sum())


def test_fuzz(torch_cuda, comp):
    streams, mutants = C.fuzz()
    assert len(streams) == 200 and len(mutants) == 2000
    errors = 0
    for name, data, tile in streams + mutants:
        errors += check(torch_cuda, comp, name, data, tile)[0] == "error"
    assert errors >= 1000


def test_a_large_parse_then_a_small_one_then_after_reset(torch_cuda, comp):
    """No tile state of an earlier call carries over: the small stream's tiles
    were a large stream's before, with other entries, counts and exits."""
    large = C.good(3000, seed=8)
    small = C.ser(raw=b"abc") + b"\x00" * 70 + C.ser(chunk_blob=C.blob(5))
    bad = C.pad(100) + b"\x02\x12\x09"
    for tile in (C.T, None):
        check(torch_cuda, comp, "large", large, tile)
        check(torch_cuda, comp, "small", small, tile)
        check(torch_cuda, comp, "large", large, tile)
        assert check(torch_cuda, comp, "bad", bad, tile)[0] == "error"
        check(torch_cuda, comp, "small", small, tile)
        assert comp._L.zc_reset(comp._ctx) == 0
        check(torch_cuda, comp, "small after reset", small, tile)
        check(torch_cuda, comp, "empty", b"", tile)
