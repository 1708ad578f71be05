"""CPU tests of the chunk-index entry points: the symbols, the struct layouts,
and every argument error zc_chunk_index_create_arrays and zc_restore_resolve
find before they look at their context (tests/resolve_cases.py lists them).
No device is needed: with no context at all the message names the fault, and a
well-formed call -- zero-sized everything included -- names the missing
context."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from tests import resolve_cases as C
from zbackup_amd import _build, _lib

NEW_SYMBOLS = ["zc_chunk_index_create", "zc_chunk_index_create_arrays", "zc_chunk_index_counts",
               "zc_chunk_index_bundles", "zc_chunk_index_lookup", "zc_chunk_index_destroy", "zc_restore_resolve",
               "zc_restore_plan_counts", "zc_restore_plan_fetch", "zc_restore_plan_destroy", "zc_resolve_last_stats"]


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
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    import zbackup_amd
    assert zbackup_amd.ChunkIndex is not None and zbackup_amd.Restorer.plan_index is not None
    assert zbackup_amd.IndexedRestorer.from_index is not None and zbackup_amd.IndexLoader.load_resident is not None
    names = {p.rsplit("/", 1)[-1] for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_resolve.hip", "zc_resolve_core.h"} <= names


def test_struct_layouts():
    """zc_instruction is read on the device as twelve 32-bit words: kind at 0,
    the id at 4, data_off at 32, size at 40."""
    f = {name: getattr(_lib.ZcInstruction, name).offset for name, _ in _lib.ZcInstruction._fields_}
    assert f == {"kind": 0, "id": 4, "reserved": 28, "data_off": 32, "size": 40}
    assert ctypes.sizeof(_lib.ZcInstruction) == 48 == C.INSTR.itemsize
    assert [C.INSTR.fields[n][1] for n in ("kind", "id", "reserved", "data_off", "size")] == [0, 4, 28, 32, 40]
    header = open(_build.HEADERS[-1]).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name


def _create(lib, N=3, B=2, bundle_first=(0, 1, 3), ids=True, out=True):
    keep = [np.zeros(max(24 * N, 1) if ids else 1, dtype=np.uint8), np.zeros(max(N, 1) if ids else 1, dtype=np.uint32)]
    first = None if bundle_first is None else np.array(bundle_first, dtype=np.uint64)
    idx = ctypes.c_void_p()
    rc = lib.zc_chunk_index_create_arrays(None, keep[0].ctypes.data if ids else None,
                                          keep[1].ctypes.data if ids else None, N,
                                          None if first is None else first.ctypes.data, B,
                                          ctypes.byref(idx) if out else None)
    assert not idx.value
    return rc, _err(lib)


def _resolve(lib, idx=True, out=True, ins=True, n=None, kind=None, data_off=None, size=None, wrap=False):
    """A well-formed call of three entries over a stream of 100 bytes, then the change asked for."""
    fake = np.zeros(64, dtype=np.uint64)  # stands for an index: nothing reads it before the context is looked at
    a = np.zeros(3, dtype=C.INSTR)
    a[1]["kind"], a[1]["data_off"], a[1]["size"] = 1, 10, 90
    instr_bytes = 100
    if kind is not None:
        a[1]["kind"] = kind
    if data_off is not None:
        a[1]["data_off"], a[1]["size"] = data_off, size
    if wrap:
        instr_bytes = (1 << 64) - 1
        a[0]["kind"], a[0]["size"] = 1, 1 << 63
        a[1]["size"] = 5
        a[2]["kind"], a[2]["size"] = 1, (1 << 63) - 5
    plan = ctypes.c_void_p()
    rc = lib.zc_restore_resolve(None, fake.ctypes.data if idx else None, a.ctypes.data if ins else None,
                                len(a) if n is None else n, instr_bytes, ctypes.byref(plan) if out else None)
    assert not plan.value
    return rc, _err(lib)


def test_well_formed_calls_without_a_context_name_the_context(lib):
    assert _create(lib) == (_lib.ZC_ERR_ARG, "zc_chunk_index_create_arrays: null context")
    # zero records in two bundles, zero bundles, and nothing at all (bundle_first NULL stands for {0})
    assert _create(lib, N=0, B=2, bundle_first=(0, 0, 0), ids=False)[1] == "zc_chunk_index_create_arrays: null context"
    assert _create(lib, N=0, B=0, bundle_first=(0,), ids=False)[1] == "zc_chunk_index_create_arrays: null context"
    assert _create(lib, N=0, B=0, bundle_first=None, ids=False)[1] == "zc_chunk_index_create_arrays: null context"
    assert _resolve(lib) == (_lib.ZC_ERR_ARG, "zc_restore_resolve: null context")
    assert _resolve(lib, n=0, ins=False)[1] == "zc_restore_resolve: null context"
    assert _resolve(lib, data_off=100, size=0)[1] == "zc_restore_resolve: null context"  # 0 bytes at the end
    assert _resolve(lib, data_off=0, size=100)[1] == "zc_restore_resolve: null context"


@pytest.mark.parametrize("name, call, kw, text", C.ERRORS, ids=[e[0] for e in C.ERRORS])
def test_argument_errors_are_found_before_the_context_is_used(lib, name, call, kw, text):
    rc, msg = (_create if call == "create" else _resolve)(lib, **kw)
    assert rc == _lib.ZC_ERR_ARG
    prefix = "zc_chunk_index_create_arrays: " if call == "create" else "zc_restore_resolve: "
    assert msg.startswith(prefix) and text in msg, msg


def test_the_other_entry_points_check_their_pointers(lib):
    idx = ctypes.c_void_p()
    assert lib.zc_chunk_index_create(None, None, ctypes.byref(idx)) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_chunk_index_create: null set" and not idx.value
    fake = np.zeros(64, dtype=np.uint64)
    ids, b, off, sz = (np.zeros(24, dtype=np.uint8), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64),
                       np.zeros(1, dtype=np.uint32))
    args = [ids.ctypes.data, 1, b.ctypes.data, off.ctypes.data, sz.ctypes.data]
    assert lib.zc_chunk_index_lookup(None, None, *args) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_chunk_index_lookup: null index"
    assert lib.zc_chunk_index_lookup(None, fake.ctypes.data, *args) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_chunk_index_lookup: null context"
    for k in (0, 2, 3, 4):
        bad = list(args)
        bad[k] = None
        assert lib.zc_chunk_index_lookup(None, fake.ctypes.data, *bad) == _lib.ZC_ERR_ARG
        assert _err(lib) == "zc_chunk_index_lookup: null pointer"
    assert lib.zc_chunk_index_lookup(None, fake.ctypes.data, None, 0, None, None, None) == _lib.ZC_ERR_ARG
    assert _err(lib) == "zc_chunk_index_lookup: null context"  # no ids: nothing to point at
    for fn, name in ((lib.zc_chunk_index_counts, "zc_chunk_index_counts"),
                     (lib.zc_restore_plan_counts, "zc_restore_plan_counts"),
                     (lib.zc_restore_plan_fetch, "zc_restore_plan_fetch")):
        assert fn(None, *[None] * (len(fn.argtypes) - 1)) == _lib.ZC_ERR_ARG and name in _err(lib)
    assert lib.zc_chunk_index_bundles(None, None, None) == _lib.ZC_ERR_ARG and "zc_chunk_index_bundles" in _err(lib)
    assert lib.zc_chunk_index_destroy(None) == _lib.ZC_ERR_ARG and "zc_chunk_index_destroy" in _err(lib)
    assert lib.zc_restore_plan_destroy(None) == _lib.ZC_ERR_ARG and "zc_restore_plan_destroy" in _err(lib)
    slots = ctypes.c_uint64(7)
    assert lib.zc_resolve_last_stats(None, None, None, ctypes.byref(slots), None) == _lib.ZC_ERR_ARG
    assert "zc_resolve_last_stats" in _err(lib) and slots.value == 7
