"""CPU tests of garbage collection:

* zc_gc_core.h -- the id table's hash, 24-byte compare, insert and lookup the
  kernels of zc_gc.hip run -- compiled for the host (under ASan + UBSan where
  that links) with a main of its own and compared with std::map on random ids
  at every table load, on near-equal ids and on thousands of ids with one slot
  hash (tests/gc/gc_core_check.cpp);
* the reference restatement's own checks (tests/gc_ref.py runs them on import);
* the new symbols, and the argument errors zc_gc_plan finds before it looks at
  its context: they need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gc_ref
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zc_gc_plan", "zc_gc_last_stats", "zc_gc_last_times"]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _build_check(tmp_path):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path / "gc_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "gc", "gc_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


def test_table_core_matches_std_map(tmp_path):
    exe, sanitized = _build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    # the one-hash case alone looks up 4,500 records
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) >= 10000


def test_reference_helper():
    """gc_ref checked itself on import; its flag and action numbers are the header's."""
    gc_ref._self_check()
    header = open(os.path.join(ROOT, "include", "zchunk.h")).read()
    for name, ref in (("ZC_GC_DEEP", gc_ref.DEEP), ("ZC_GC_REPACK", gc_ref.REPACK), ("ZC_GC_CONCAT", gc_ref.CONCAT),
                      ("ZC_GC_ACT_KEEP", gc_ref.KEEP), ("ZC_GC_ACT_REMOVE", gc_ref.REMOVE),
                      ("ZC_GC_ACT_REPACK", gc_ref.REPACK_BUNDLE), ("ZC_GC_ACT_DROP_RECORD", gc_ref.DROP_RECORD),
                      ("ZC_GC_REC_COUNTED", gc_ref.COUNTED), ("ZC_GC_REC_USED", gc_ref.USED),
                      ("ZC_GC_REC_COPIED", gc_ref.COPIED)):
        value = int(re.search(r"\b%s = (\d+)" % name, header).group(1))
        assert value == ref == getattr(_lib, name)
    assert gc_ref.MAX_PAYLOAD_SIZE == 0x200000


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
    assert zbackup_amd.Collector is not None and zbackup_amd.GcPlan is not None
    # the build id covers the new sources
    names = {os.path.basename(p) for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_gc.hip", "zc_gc_core.h"} <= names


def _call(lib, ctx=None, N=0, B=0, I=0, U=0, bundle_first=None, index_first=None, flags=0, ids=True, outs=True,
          copy_cap=0):
    """zc_gc_plan over zeroed arrays of the given counts; returns (rc, message)."""
    keep = []

    def arr(n, dtype, on=True):
        if not on:
            return None
        a = np.zeros(max(n, 1), dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    def ranges(v):
        if v is None:
            return None
        a = np.array(v, dtype=np.uint64)
        keep.append(a)
        return a.ctypes.data

    gin = _lib.ZcGcInput(arr(24 * N, np.uint8, ids), arr(N, np.uint32), N, ranges(bundle_first), arr(24 * B, np.uint8),
                         B, ranges(index_first), I, arr(24 * U, np.uint8), U, flags, 0, 1 << 21)
    out = _lib.ZcGcOutput(arr(N, np.uint8, outs), arr(B, np.uint32), arr(B, np.uint32), arr(B, np.uint8),
                          arr(I, _lib.ZcGcIndex), arr(copy_cap, np.uint32), arr(copy_cap, np.uint32),
                          arr(copy_cap, np.uint64), copy_cap, 0, arr(copy_cap, np.uint32), arr(copy_cap, np.uint64),
                          copy_cap, 0)
    rc = lib.zc_gc_plan(ctx, ctypes.byref(gin), ctypes.byref(out))
    return rc, lib.zc_last_error(ctx).decode()


def test_null_context_is_an_argument_error_with_a_message(lib):
    """A well-formed (empty) input and no context: the context's absence is the error."""
    rc, msg = _call(lib)
    assert rc == _lib.ZC_ERR_ARG and msg == "zc_gc_plan: null context"
    rc, msg = _call(lib, N=3, B=2, I=1, U=1, bundle_first=[0, 1, 3], index_first=[0, 2], copy_cap=3)
    assert rc == _lib.ZC_ERR_ARG and msg == "zc_gc_plan: null context"
    assert lib.zc_gc_plan(None, None, None) == _lib.ZC_ERR_ARG
    assert "null input or output" in lib.zc_last_error(None).decode()
    slots = ctypes.c_uint64(7)
    assert lib.zc_gc_last_stats(None, None, None, ctypes.byref(slots), None) == _lib.ZC_ERR_ARG
    assert b"zc_gc_last_stats" in lib.zc_last_error(None) and slots.value == 7
    assert lib.zc_gc_last_times(None, None, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_gc_last_times" in lib.zc_last_error(None)


@pytest.mark.parametrize("kw, text", [
    (dict(N=3, B=2, I=1, bundle_first=[0, 2, 1], index_first=[0, 2]), "bundle_first[2] = 1 is below bundle_first[1] = 2"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 2], index_first=[0, 2]), "bundle_first ends at 2, there are 3 records"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 4], index_first=[0, 2]), "bundle_first ends at 4, there are 3 records"),
    (dict(N=3, B=2, I=1, bundle_first=[1, 1, 3], index_first=[0, 2]), "bundle_first[0] = 1, not 0"),
    (dict(N=3, B=2, I=2, bundle_first=[0, 1, 3], index_first=[0, 2, 1]), "index_first[2] = 1 is below index_first[1] = 2"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 3], index_first=[0, 1]), "index_first ends at 1, there are 2 bundles"),
    (dict(N=3, B=0, I=0), "bundle_first is empty but there are 3 records"),
    (dict(N=0, B=2, I=0, bundle_first=[0, 0, 0]), "index_first is empty but there are 2 bundles"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 3], index_first=[0, 2], ids=False), "null input array"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 3], index_first=[0, 2], outs=False), "null output array"),
    (dict(N=3, B=2, I=1, bundle_first=[0, 1, 3], index_first=[0, 2], flags=8), "unknown flag"),
    (dict(N=(1 << 32) - 1, ids=False), "must stay below 2^32 - 1"),
    (dict(U=(1 << 32) - 1, ids=False), "must stay below 2^32 - 1"),
])
def test_bad_input_is_found_before_the_context_is_used(lib, kw, text):
    """With no context at all: the message names the fault, not the context."""
    if kw.get("N", 0) > 1 << 20 or kw.get("U", 0) > 1 << 20:
        # counts only: no array of that size is made, none is read
        gin = _lib.ZcGcInput(None, None, kw.get("N", 0), None, None, 0, None, 0, None, kw.get("U", 0), 0, 0, 0)
        out = _lib.ZcGcOutput()
        rc, msg = lib.zc_gc_plan(None, ctypes.byref(gin), ctypes.byref(out)), lib.zc_last_error(None).decode()
    else:
        rc, msg = _call(lib, **kw)
    assert rc == _lib.ZC_ERR_ARG
    assert msg.startswith("zc_gc_plan: ") and text in msg, msg
