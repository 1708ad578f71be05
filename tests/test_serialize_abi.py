"""CPU tests of the device serializer's entry points: the symbols, and every
argument error zc_serialized_size and zc_serialize_records_device find before
they look at their context or at the device.  No device is needed: with no
context at all the message names the fault, the output is untouched, and a
well-formed call -- no records included -- names the missing context."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from zbackup_amd import RECORD_DTYPE, _build, _lib, chunk_id_blob, serialize_instruction

NEW_SYMBOLS = ["zc_serialized_size", "zc_serialize_records_device", "zc_serialize_last_stats"]
NAME = "zc_serialize_records_device: "


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _err(lib):
    return lib.zc_last_error(None).decode()


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert not set(NEW_SYMBOLS) - exported
    assert not set(NEW_SYMBOLS) - set(_lib.EXPORTS)
    assert lib.zc_abi_version() == 5  # detected by symbol, not by version
    header = open(_build.HEADERS[-1]).read()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, header), name
    import zbackup_amd
    for name in ("serialize_device", "free_device", "backup_device", "serialize_stats"):
        assert callable(getattr(zbackup_amd.BackupCreator, name))
    assert callable(zbackup_amd.serialized_size)
    names = {p.rsplit("/", 1)[-1] for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_ser.hip", "zc_ser_core.h", "zc_scan_body.h"} <= names


def _records(kinds_sizes, offsets=None):
    recs = np.zeros(len(kinds_sizes), dtype=RECORD_DTYPE)
    for i, (kind, size) in enumerate(kinds_sizes):
        recs[i]["kind"], recs[i]["size"] = kind, size
        recs[i]["offset"] = offsets[i] if offsets else 0
        recs[i]["rolling"] = 0x0123456789ABCDEF + i
        recs[i]["sha1"] = np.arange(16, dtype=np.uint8) + i
    return recs


def test_serialized_size_on_hand_made_records(lib):
    size = ctypes.c_uint64(77)
    assert lib.zc_serialized_size(None, 0, ctypes.byref(size)) == _lib.ZC_OK and size.value == 0
    recs = _records([(_lib.ZC_CHUNK_NEW, 65536), (_lib.ZC_BYTES, 0), (_lib.ZC_BYTES, 1), (_lib.ZC_CHUNK_DUP, 9),
                     (_lib.ZC_BYTES, 127), (_lib.ZC_BYTES, 128), (7, 3), (_lib.ZC_BYTES, 16384)])
    want = sum(len(serialize_instruction(raw=bytes(int(r["size"])))) if r["kind"] == _lib.ZC_BYTES else
               len(serialize_instruction(chunk_blob=chunk_id_blob(bytes(r["sha1"]), int(r["rolling"])))) for r in recs)
    assert want == 27 + 3 + 4 + 27 + 131 + 133 + 27 + (3 + 1 + 3 + 16384)
    assert lib.zc_serialized_size(recs.ctypes.data, len(recs), ctypes.byref(size)) == _lib.ZC_OK
    assert size.value == want
    # the errors: the message is the thread's, *bytes is left alone
    size.value = 77
    assert lib.zc_serialized_size(recs.ctypes.data, len(recs), None) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_serialized_size: null size pointer"
    assert lib.zc_serialized_size(None, 3, ctypes.byref(size)) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_serialized_size: null record array" and size.value == 77


def _call(lib, recs, stream_len=4096, out_cap=1 << 20, stream=True, out=True, n_out=True, n=None):
    fake_stream = np.zeros(16, dtype=np.uint8)  # stand for device memory: nothing reads or writes them
    fake_out = np.full(64, 0xEE, dtype=np.uint8)  # before the context is looked at
    wrote = ctypes.c_uint64(77)
    rc = lib.zc_serialize_records_device(None, recs.ctypes.data if recs is not None else None,
                                         len(recs) if n is None else n,
                                         fake_stream.ctypes.data if stream else None, stream_len,
                                         fake_out.ctypes.data if out else None, out_cap,
                                         ctypes.byref(wrote) if n_out else None)
    assert (fake_out == 0xEE).all() and not fake_stream.any()
    return rc, _err(lib), wrote.value


def test_serialize_device_argument_errors(lib):
    recs = _records([(_lib.ZC_CHUNK_NEW, 4096), (_lib.ZC_BYTES, 100), (_lib.ZC_BYTES, 300)], offsets=[0, 4096 - 400, 4096 - 300])
    need = 27 + 103 + 305
    # well formed: the missing context is all that is wrong, *n_out is the stream's length
    assert _call(lib, recs) == (_lib.ZC_ERR_ARG, NAME + "null context", need)
    assert _call(lib, recs, out_cap=need) == (_lib.ZC_ERR_ARG, NAME + "null context", need)
    # no records: legal with or without buffers
    empty = _records([])
    assert _call(lib, empty) == (_lib.ZC_ERR_ARG, NAME + "null context", 0)
    assert _call(lib, None, n=0, stream=False, stream_len=0, out=False, out_cap=0) == (
        _lib.ZC_ERR_ARG, NAME + "null context", 0)
    # NULL arguments
    assert _call(lib, recs, n_out=False)[:2] == (_lib.ZC_ERR_ARG, NAME + "null n_out")
    assert _call(lib, None, n=3) == (_lib.ZC_ERR_ARG, NAME + "null record array", 77)
    assert _call(lib, recs, stream=False) == (_lib.ZC_ERR_ARG, NAME + "null stream pointer", 77)
    assert _call(lib, recs, out=False) == (_lib.ZC_ERR_ARG, NAME + "null output pointer", 77)
    # the record count keeps 32-bit positions in the scan
    for n in ((1 << 32) - 1, 1 << 40):
        assert _call(lib, recs, n=n) == (_lib.ZC_ERR_ARG, NAME + f"{n} records: the count must stay below 2^32 - 1", 77)


def test_a_range_past_the_stream_names_its_record(lib):
    recs = _records([(_lib.ZC_CHUNK_NEW, 4096), (_lib.ZC_BYTES, 100), (_lib.ZC_BYTES, 300)], offsets=[0, 3996, 3797])
    assert _call(lib, recs)[1] == NAME + "record 2: bytes [3797, +300) past the end of a stream of 4096 bytes"
    recs["offset"][2] = 3796
    assert _call(lib, recs)[1] == NAME + "null context"
    recs["offset"][1] = 3997
    assert _call(lib, recs) == (_lib.ZC_ERR_ARG,
                                NAME + "record 1: bytes [3997, +100) past the end of a stream of 4096 bytes", 77)
    # an offset that would wrap, an empty range at the very end, and a chunk record, whose range is not read
    recs["offset"][1] = (1 << 64) - 50
    assert "record 1: bytes [18446744073709551566, +100) past" in _call(lib, recs)[1]
    recs["offset"][1], recs["size"][1] = 4096, 0
    assert _call(lib, recs)[1] == NAME + "null context"
    recs["offset"][1] = 4097
    assert "record 1: bytes [4097, +0) past" in _call(lib, recs)[1]
    recs["offset"][1] = 0
    recs["offset"][0], recs["size"][0] = 1 << 50, 4096
    assert _call(lib, recs)[1] == NAME + "null context"
    # an empty stream takes empty ranges only
    assert _call(lib, recs, stream=False, stream_len=0)[1].startswith(NAME + "record 2: bytes [3796, +300) past")


def test_a_short_output_reports_the_bytes_needed(lib):
    recs = _records([(_lib.ZC_CHUNK_DUP, 4096), (_lib.ZC_BYTES, 100), (_lib.ZC_BYTES, 300)], offsets=[0, 0, 100])
    need = 27 + 103 + 305
    for cap in (0, 1, need - 1):
        assert _call(lib, recs, out_cap=cap, out=cap > 0) == (
            _lib.ZC_ERR_ARG, NAME + f"the stream takes {need} bytes, the output has room for {cap}", need)


def test_last_stats_checks_its_context(lib):
    staged = ctypes.c_uint64(7)
    assert lib.zc_serialize_last_stats(None, None, None, None, ctypes.byref(staged), None) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_serialize_last_stats: null context" and staged.value == 7
