"""CPU tests of the random-access restore:

* zc_range_core.h -- the search, the walk and the clip the kernel of
  zc_range.hip runs per piece -- compiled for the host (under ASan + UBSan where
  that links) with a main of its own and compared with a restatement of
  IndexedRestorer::saveData (tests/range/range_core_check.cpp);
* the new symbols, and the argument errors the zc_range_* calls find before
  they look at a context: they need no device;
* zc_range_needs against a numpy restatement (tests/range_ref.py), and
  IndexedRestorer.needs mapping slots back to bundle numbers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import range_ref
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zc_range_index_create", "zc_range_index_total", "zc_range_index_destroy", "zc_range_set_slot",
               "zc_range_slot_upload", "zc_range_slot_drop", "zc_range_needs", "zc_range_read",
               "zc_range_read_host", "zc_range_last_stats"]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _build_check(tmp_path):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path / "range_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "range", "range_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


def test_piece_routine_matches_save_data(tmp_path):
    exe, sanitized = _build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) >= 10000


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert not set(NEW_SYMBOLS) - exported
    assert not set(NEW_SYMBOLS) - set(_lib.EXPORTS)
    assert lib.zc_abi_version() == 5  # detected by symbol, not by version
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    import zbackup_amd
    assert zbackup_amd.IndexedRestorer is not None and zbackup_amd.RangeIndex is not None
    # the build id covers the new sources
    names = {os.path.basename(p) for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_range.hip", "zc_range_core.h", "zc_copy_body.h"} <= names


def _u64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.uint64))


def _create(lib, slot_sizes, slot, off, sizes):
    """A host-only index (no context); returns (rc, message, handle)."""
    slot_sizes, off, sizes = _u64(slot_sizes), _u64(off), _u64(sizes)
    slot = np.ascontiguousarray(np.asarray(slot, dtype=np.uint32))
    idx = ctypes.c_void_p()
    rc = lib.zc_range_index_create(None, slot_sizes.ctypes.data, len(slot_sizes), slot.ctypes.data, off.ctypes.data,
                                   sizes.ctypes.data, len(sizes), ctypes.byref(idx))
    return rc, lib.zc_last_error(None).decode(), idx


def _read(lib, idx, reads, dst=1, host=False, dst_off=True):
    """zc_range_read[_host] with no context; dst is never written (1: a non-null pointer)."""
    offset, size = _u64([r[0] for r in reads]), _u64([r[1] for r in reads])
    doff = _u64([0] * len(reads))
    fn = lib.zc_range_read_host if host else lib.zc_range_read
    rc = fn(None, idx, offset.ctypes.data, size.ctypes.data, len(reads), dst, doff.ctypes.data if dst_off else None)
    return rc, lib.zc_last_error(None).decode()


@pytest.fixture()
def small(lib):
    """Three slots; the stream is 100 + 0 + 50 + 30 = 180 bytes."""
    rc, msg, idx = _create(lib, [100, 80, 30], [0, 2, 1, 2], [0, 5, 30, 0], [100, 0, 50, 30])
    assert rc == _lib.ZC_OK, msg
    yield idx
    assert lib.zc_range_index_destroy(idx) == _lib.ZC_OK


@pytest.mark.parametrize("args, text", [
    (([10], [1], [0], [5]), "entry 0 names slot 1 of 1"),
    (([10, 20], [0, 1], [0, 15], [10, 6]), "entry 1 [15, +6) ends past slot 1's 20 bytes"),
    (([10], [0], [11], [0]), "entry 0 [11, +0) ends past slot 0's 10 bytes"),
    (([2 ** 63] * 2, [0, 1, 0], [0, 0, 0], [2 ** 63, 2 ** 63 - 1, 1]), "entry 2 takes the stream's length past 2^64"),
])
def test_create_refuses_bad_entries(lib, args, text):
    rc, msg, idx = _create(lib, *args)
    assert rc == _lib.ZC_ERR_ARG and not idx.value
    assert msg == "zc_range_index_create: " + text


def test_create_and_total_null_arguments(lib):
    idx = ctypes.c_void_p()
    assert lib.zc_range_index_create(None, None, 1, None, None, None, 0, ctypes.byref(idx)) == _lib.ZC_ERR_ARG
    assert "null slot_sizes, slot, off or sizes" in lib.zc_last_error(None).decode()
    assert lib.zc_range_index_create(None, None, 0, None, None, None, 0, None) == _lib.ZC_ERR_ARG
    total = ctypes.c_uint64(7)
    assert lib.zc_range_index_total(None, ctypes.byref(total)) == _lib.ZC_ERR_ARG and total.value == 7
    assert lib.zc_range_index_destroy(None) == _lib.ZC_ERR_ARG
    for fn in (lib.zc_range_set_slot, lib.zc_range_slot_drop):
        assert fn(None, 0, *([None] if fn is lib.zc_range_set_slot else [])) == _lib.ZC_ERR_ARG
    assert lib.zc_range_last_stats(None, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_range_last_stats" in lib.zc_last_error(None)
    # an empty index is legal: no slots, no entries, 0 bytes
    rc, msg, idx = _create(lib, [], [], [], [])
    assert rc == _lib.ZC_OK
    assert lib.zc_range_index_total(idx, ctypes.byref(total)) == _lib.ZC_OK and total.value == 0
    assert _read(lib, idx, [(0, 0)]) == (_lib.ZC_ERR_ARG, "zc_range_read: null context")
    assert _read(lib, idx, [(0, 1)])[1].startswith("zc_range_read: read 0 [0, +1) is out of range")
    lib.zc_range_index_destroy(idx)


@pytest.mark.parametrize("host", [False, True])
def test_read_errors_come_before_the_context(lib, small, host):
    """With no context at all: the message names the fault, not the context."""
    what = "zc_range_read_host: " if host else "zc_range_read: "
    total = ctypes.c_uint64()
    assert lib.zc_range_index_total(small, ctypes.byref(total)) == _lib.ZC_OK and total.value == 180
    # out of range (exOutOfRange), the sum wrapping included; 0 bytes at the total is a read
    for reads, text in (([(0, 10), (171, 10)], "read 1 [171, +10) is out of range: the stream has 180 bytes"),
                        ([(181, 0)], "read 0 [181, +0) is out of range"),
                        ([(2 ** 64 - 1, 2)], "read 0 [18446744073709551615, +2) is out of range")):
        rc, msg = _read(lib, small, reads, host=host)
        assert rc == _lib.ZC_ERR_ARG and msg.startswith(what + text), msg
    # a touched slot without a pointer: the message names it
    rc, msg = _read(lib, small, [(180, 0), (10, 20)], host=host)
    assert rc == _lib.ZC_ERR_ARG and msg.startswith(what + "slot 0 is not resident"), msg
    assert lib.zc_range_set_slot(small, 0, 0x1000) == _lib.ZC_OK
    rc, msg = _read(lib, small, [(10, 20), (99, 2)], host=host)  # the empty entry's slot 2 is not touched
    assert rc == _lib.ZC_ERR_ARG and msg.startswith(what + "slot 1 is not resident"), msg
    assert lib.zc_range_set_slot(small, 1, 0x2000) == _lib.ZC_OK
    # null arguments with reads > 0
    assert _read(lib, small, [(10, 20)], dst=None, host=host) == (_lib.ZC_ERR_ARG, what + "null destination")
    rc, msg = _read(lib, small, [(10, 20)], dst_off=False, host=host)
    assert rc == _lib.ZC_ERR_ARG and "null offset, size or dst_off" in msg
    assert (lib.zc_range_read_host if host else lib.zc_range_read)(None, None, None, None, 0, None, None) \
        == _lib.ZC_ERR_ARG
    assert lib.zc_last_error(None).decode() == what + "null index"
    # all of it in order: only the context is missing now (0 reads included)
    assert _read(lib, small, [(10, 20), (99, 2)], host=host) == (_lib.ZC_ERR_ARG, what + "null context")
    assert _read(lib, small, [], host=host) == (_lib.ZC_ERR_ARG, what + "null context")
    # clearing a slot takes it away again; a slot that does not exist is refused
    assert lib.zc_range_slot_drop(small, 1) == _lib.ZC_OK
    assert _read(lib, small, [(99, 2)], host=host)[1].startswith(what + "slot 1 is not resident")
    assert lib.zc_range_set_slot(small, 3, 0x1000) == _lib.ZC_ERR_ARG
    assert lib.zc_last_error(None).decode() == "zc_range_set_slot: slot 3 of 3"
    # an upload needs the slot's size, and a device
    buf = np.zeros(100, dtype=np.uint8)
    assert lib.zc_range_slot_upload(small, 0, buf.ctypes.data, 99) == _lib.ZC_ERR_ARG
    assert lib.zc_last_error(None).decode() == "zc_range_slot_upload: slot 0 holds 100 bytes, 99 given"
    assert lib.zc_range_slot_upload(small, 0, buf.ctypes.data, 100) == _lib.ZC_ERR_ARG
    assert "made without a context" in lib.zc_last_error(None).decode()


def _needs(lib, idx, reads, cap):
    offset, size = _u64([r[0] for r in reads]), _u64([r[1] for r in reads])
    out = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    n = ctypes.c_size_t(99)
    rc = lib.zc_range_needs(idx, offset.ctypes.data, size.ctypes.data, len(reads), out.ctypes.data, cap,
                            ctypes.byref(n))
    return rc, n.value, [int(s) for s in out[:min(n.value, cap)]]


def test_needs_matches_the_numpy_restatement(lib, small):
    assert _needs(lib, small, [(0, 180)], 3) == (_lib.ZC_OK, 3, [0, 1, 2])
    assert _needs(lib, small, [(0, 150)], 3) == (_lib.ZC_OK, 2, [0, 1])  # slot 2's entry in there is empty...
    assert _needs(lib, small, [(149, 2)], 3) == (_lib.ZC_OK, 2, [1, 2])  # ... and its other one is not
    assert _needs(lib, small, [], 0) == (_lib.ZC_OK, 0, [])
    assert _needs(lib, small, [(180, 0), (5, 0)], 0) == (_lib.ZC_OK, 0, [])
    rc, n, got = _needs(lib, small, [(0, 180)], 1)  # too little room: the count is still reported
    assert (rc, n, got) == (_lib.ZC_ERR_ARG, 3, [0]) and "room for 1" in lib.zc_last_error(None).decode()
    assert _needs(lib, small, [(100, 81)], 3)[0] == _lib.ZC_ERR_ARG
    assert "out of range" in lib.zc_last_error(None).decode()
    rng = np.random.default_rng(5)
    for n_entries, n_slots in ((1, 1), (40, 7), (3000, 50)):
        sizes = rng.choice([0, 0, 1, 2, 15, 16, 17, 4096, 65537], n_entries)
        slot = rng.integers(0, n_slots, n_entries)
        rc, msg, idx = _create(lib, [70000] * n_slots, slot, rng.integers(0, 4000, n_entries), sizes)
        assert rc == _lib.ZC_OK, msg
        total = int(sizes.sum())
        pos = range_ref.positions(sizes)
        for batch in (1, 3, 40):
            for _ in range(30):
                reads = []
                for _ in range(batch):
                    o = int(rng.choice(pos)) + int(rng.integers(-1, 2)) if rng.random() < 0.5 \
                        else int(rng.integers(0, total + 1))
                    o = min(max(o, 0), total)
                    reads.append((o, min(int(rng.choice([0, 1, 2, 100, 70000, 10 ** 6])), total - o)))
                want = range_ref.needs(slot, sizes, reads)
                assert _needs(lib, idx, reads, n_slots) == (_lib.ZC_OK, len(want), want)
        lib.zc_range_index_destroy(idx)


def test_indexed_restorer_needs_names_bundles(lib):
    """A host-only IndexedRestorer: slots map back to bundle numbers, the
    instruction stream's slot (the bytes_to_emit runs) to none."""
    from zbackup_amd import IndexedRestorer, serialize_instruction
    ids = [bytes([k + 1]) * 24 for k in range(6)]
    # bundle 0 is never referenced; the stream uses bundles 2, 1, 3 in that order
    bundles = [[(ids[0], 10)], [(ids[1], 100), (ids[2], 50)], [(ids[3], 70)], [(ids[4], 30), (ids[5], 1)]]
    stream = [(ids[3], None), (None, b"abcde"), (ids[2], None), (ids[5], None), (ids[3], b"xy"), (ids[1], None)]
    data = b"".join(serialize_instruction(chunk_blob=c, raw=b) for c, b in stream)
    with IndexedRestorer(data, bundles, device=None) as ir:
        assert ir.plan.used == [2, 1, 3]
        sizes = [70, 5, 50, 1, 70, 2, 100]
        assert ir.size == sum(sizes) == 298
        assert ir.needs([(0, 298)]) == [2, 1, 3]
        assert ir.needs([(0, 70)]) == [2] and ir.needs([(70, 5)]) == [] and ir.needs([(69, 7)]) == [2, 1]
        assert ir.needs([(125, 1)]) == [3] and ir.needs([(124, 3)]) == [2, 1, 3]
        assert ir.needs([(196, 2), (10, 1)]) == [2] and ir.needs([(298, 0)]) == []
        with pytest.raises(_lib.ZcError, match="out of range"):
            ir.needs([(298, 1)])
        with pytest.raises(_lib.ZcError, match="bundle 0 is not one the stream references"):
            ir.drop_payload(0)
        ir.set_payload(1, 0x1000)
        with pytest.raises(_lib.ZcError, match=r"zc_range_read failed \(-1\): zc_range_read: slot 0 is not resident"):
            ir.read([(0, 10)], 0x5000, [0])
