"""CPU tests of the index-file entry points: the symbols, the argument errors
found before the context is used, and the host-only writer against
tests/index_ref.py.  No device is needed."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from tests import index_ref as R
from zbackup_amd import _build, _lib, index

NEW_SYMBOLS = ["zc_index_load", "zc_index_load_host", "zc_index_set_counts", "zc_index_set_fetch",
               "zc_index_set_device", "zc_index_set_destroy", "zc_bundle_info_parse", "zc_bundle_info_parse_host",
               "zc_index_serialize", "zc_index_file_size", "zc_index_last_stats"]
EDGE_SIZES = [0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert not set(NEW_SYMBOLS) - exported
    assert not set(NEW_SYMBOLS) - set(_lib.EXPORTS)
    assert lib.zc_abi_version() == 5  # detected by symbol, not by version
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)


def test_status_codes_match_the_header_and_the_reference():
    header = open(_build.HEADERS[-1]).read()
    for code, name in enumerate(R.STATUS_NAMES):
        value = int(re.search(r"\bZC_INDEX_%s = (\d+)" % name, header).group(1))
        assert value == code == getattr(_lib, "ZC_INDEX_" + name)
    assert sorted(_lib.INDEX_STATUS_NAMES) == list(range(9))


def _err(lib):
    return lib.zc_last_error(None).decode()


def test_null_arguments_are_errors_with_a_message_before_the_context_is_used(lib):
    h = ctypes.c_void_p()
    off, size = np.zeros(2, dtype=np.uint64), np.full(2, 32, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint8)
    key = bytes(16)
    for fn, name in ((lib.zc_index_load, "zc_index_load"), (lib.zc_index_load_host, "zc_index_load_host")):
        # a well-formed call and no context: the context's absence is the error
        assert fn(None, None, buf.ctypes.data, off.ctypes.data, size.ctypes.data, 2, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null context"
        assert fn(None, None, None, None, None, 0, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null context"
        assert fn(None, None, None, off.ctypes.data, size.ctypes.data, 2, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null pointer"
        assert fn(None, None, buf.ctypes.data, None, size.ctypes.data, 2, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null pointer"
        assert fn(None, None, buf.ctypes.data, off.ctypes.data, size.ctypes.data, 2, None) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null set pointer"
        # with a key: zc_bundle_unseal's alignment rules
        odd = np.array([0, 40], dtype=np.uint64)
        assert fn(None, key, buf.ctypes.data, odd.ctypes.data, size.ctypes.data, 2, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert "an offset that is not 16-byte aligned (file 1)" in _err(lib)
        assert fn(None, None, buf.ctypes.data, odd.ctypes.data, size.ctypes.data, 2, ctypes.byref(h)) == _lib.ZC_ERR_ARG
        assert _err(lib) == name + ": null context"  # without a key any offset will do
    assert lib.zc_index_load(None, key, buf.ctypes.data + 8, off.ctypes.data, size.ctypes.data, 2,
                             ctypes.byref(h)) == _lib.ZC_ERR_ARG
    assert "a base pointer is not 16-byte aligned" in _err(lib)
    assert not h.value

    n = ctypes.c_uint64(7)
    ids, sizes = np.zeros(24, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    first, st = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    for fn, name in ((lib.zc_bundle_info_parse, "zc_bundle_info_parse"),
                     (lib.zc_bundle_info_parse_host, "zc_bundle_info_parse_host")):
        args = [buf.ctypes.data, off.ctypes.data, size.ctypes.data, 2, ids.ctypes.data, sizes.ctypes.data, 1,
                first.ctypes.data, st.ctypes.data, ctypes.byref(n)]
        assert fn(None, *args) == _lib.ZC_ERR_ARG and _err(lib) == name + ": null context"
        for k in (0, 1, 2, 7, 8):
            bad = list(args)
            bad[k] = None
            assert fn(None, *bad) == _lib.ZC_ERR_ARG and _err(lib) == name + ": null pointer", k
        bad = list(args)
        bad[9] = None
        assert fn(None, *bad) == _lib.ZC_ERR_ARG and _err(lib) == name + ": null n_records"
        big = np.array([32, 1 << 32], dtype=np.uint64)
        bad = list(args)
        bad[2] = big.ctypes.data
        assert fn(None, *bad) == _lib.ZC_ERR_ARG and "a BundleInfo of 2^32 bytes or more (bundle 1)" in _err(lib)
    assert n.value == 7

    assert lib.zc_index_set_counts(None, None, None, None) == _lib.ZC_ERR_ARG and "zc_index_set_counts" in _err(lib)
    assert lib.zc_index_set_fetch(None, None, None, None, None, None, None) == _lib.ZC_ERR_ARG
    assert "zc_index_set_fetch" in _err(lib)
    assert lib.zc_index_set_device(None, None, None) == _lib.ZC_ERR_ARG and "zc_index_set_device" in _err(lib)
    assert lib.zc_index_set_destroy(None) == _lib.ZC_ERR_ARG and "zc_index_set_destroy" in _err(lib)
    d = ctypes.c_double(3.5)
    assert lib.zc_index_last_stats(None, ctypes.byref(d), None, None, None, None) == _lib.ZC_ERR_ARG
    assert "zc_index_last_stats" in _err(lib) and d.value == 3.5


def test_serialize_matches_the_reference_writer(lib):
    rng = random.Random(9)
    for counts in ([], [0], [1], [4, 5], [600], [3, 0, 2, 0, 40]):
        b = R.rand_bundles(rng, counts, EDGE_SIZES)
        body = index.serialize_index(b)
        assert body == R.body(b)
        assert index.write_index(b) == R.write(b)  # without a key nothing runs on the device
        for keyed in (False, True):
            assert index.index_file_size(len(body), keyed) == R.file_size(len(body), keyed)
            assert index.index_file_size(len(body), keyed) == len(R.write(b, bytes(16) if keyed else None, bytes(16)))
    for n in range(0, 70):
        for keyed in (False, True):
            assert index.index_file_size(n, keyed) == R.file_size(n, keyed)


def test_serialize_argument_errors(lib):
    need = ctypes.c_uint64()
    first = np.array([0, 1], dtype=np.uint64)
    bid, cid, size = np.zeros(24, dtype=np.uint8), np.ones(24, dtype=np.uint8), np.array([5], dtype=np.uint32)
    out = np.zeros(64, dtype=np.uint8)
    args = [cid.ctypes.data, size.ctypes.data, first.ctypes.data, bid.ctypes.data, 1]
    assert lib.zc_index_serialize(*args, out.ctypes.data, 64, None) == _lib.ZC_ERR_ARG and "null n_out" in _err(lib)
    assert lib.zc_index_serialize(*args, out.ctypes.data, 10, ctypes.byref(need)) == _lib.ZC_ERR_ARG
    assert need.value == 3 + 27 + 1 + 30 + 1 and "62 bytes, room for 10" in _err(lib)
    assert lib.zc_index_serialize(*args, out.ctypes.data, 64, ctypes.byref(need)) == _lib.ZC_OK
    assert out[:62].tobytes() == R.body([(bytes(24), [(bytes([1]) * 24, 5)])])
    assert lib.zc_index_serialize(None, size.ctypes.data, first.ctypes.data, bid.ctypes.data, 1, out.ctypes.data, 64,
                                  ctypes.byref(need)) == _lib.ZC_ERR_ARG and "null record arrays" in _err(lib)
    down = np.array([0, 2, 1], dtype=np.uint64)
    two = np.zeros(48, dtype=np.uint8)
    assert lib.zc_index_serialize(cid.ctypes.data, size.ctypes.data, down.ctypes.data, two.ctypes.data, 2,
                                  out.ctypes.data, 64, ctypes.byref(need)) == _lib.ZC_ERR_ARG
    assert "bundle_first decreases" in _err(lib)
    with pytest.raises(_lib.ZcError):
        index.serialize_index([(bytes(23), [])])
    with pytest.raises(ValueError):
        index.write_index([], key=bytes(16))  # no R
