"""CPU tests of the restore-iteration entry points: the symbols, and every
argument error zc_parse_instructions_device, zc_restore_resolve_device and
zc_restore_replay find before they look at their context or at the device.  No
device is needed: with no context at all the message names the fault, and a
well-formed call -- a zero-length stream included -- names the missing context."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from zbackup_amd import _build, _lib

NEW_SYMBOLS = ["zc_parse_instructions_device", "zc_instr_set_counts", "zc_instr_set_fetch", "zc_instr_set_destroy",
               "zc_instr_last_stats", "zc_restore_resolve_device", "zc_restore_plan_entry", "zc_restore_plan_used",
               "zc_restore_replay"]


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
    for name in ("parse_device", "plan_device", "replay_device", "restore_iterations"):
        assert callable(getattr(zbackup_amd.Restorer, name))
    assert zbackup_amd.InstructionSet and zbackup_amd.DevicePlan and zbackup_amd.XzBodiesPayloads
    names = {p.rsplit("/", 1)[-1] for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_instr.hip", "zc_instr_core.h"} <= names


def _parse(lib, data=True, n=10, out=True):
    fake = np.zeros(16, dtype=np.uint8)  # stands for device memory: nothing reads it before the context is looked at
    handle = ctypes.c_void_p(1)
    rc = lib.zc_parse_instructions_device(None, fake.ctypes.data if data else None, n,
                                          ctypes.byref(handle) if out else None)
    assert not out or not handle.value  # *out is NULL after a failed call
    return rc, _err(lib)


def test_parse_argument_errors(lib):
    name = "zc_parse_instructions_device: "
    assert _parse(lib) == (_lib.ZC_ERR_ARG, name + "null context")
    # a NULL or zero-length stream is legal
    assert _parse(lib, n=0) == (_lib.ZC_ERR_ARG, name + "null context")
    assert _parse(lib, data=False, n=0) == (_lib.ZC_ERR_ARG, name + "null context")
    assert _parse(lib, out=False) == (_lib.ZC_ERR_ARG, name + "null set pointer")
    assert _parse(lib, data=False) == (_lib.ZC_ERR_ARG, name + "null stream pointer")
    # the size limit: positions fit 32 bits with one value to spare
    assert _parse(lib, n=(1 << 32) - 2) == (_lib.ZC_ERR_ARG, name + "null context")
    for n in ((1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        rc, msg = _parse(lib, n=n)
        assert rc == _lib.ZC_ERR_ARG and msg == name + f"a stream of {n} bytes: the size must stay below 2^32 - 1"


def test_the_sets_calls_check_their_pointers(lib):
    for fn, name in ((lib.zc_instr_set_counts, "zc_instr_set_counts"),
                     (lib.zc_instr_set_fetch, "zc_instr_set_fetch"),
                     (lib.zc_restore_plan_entry, "zc_restore_plan_entry"),
                     (lib.zc_restore_plan_used, "zc_restore_plan_used")):
        args = [0 if t in (ctypes.c_uint64, ctypes.c_size_t) else None for t in fn.argtypes[1:]]
        assert fn(None, *args) == _lib.ZC_ERR_ARG and _err(lib).startswith(name + ": null"), name
    assert lib.zc_instr_set_destroy(None) == _lib.ZC_ERR_ARG and _err(lib) == "zc_instr_set_destroy: null set"
    tiles = ctypes.c_uint64(7)
    assert lib.zc_instr_last_stats(None, None, None, None, None, ctypes.byref(tiles), None) == _lib.ZC_ERR_ARG
    assert "zc_instr_last_stats" in _err(lib) and tiles.value == 7


def test_resolve_device_argument_errors(lib):
    name = "zc_restore_resolve_device: "
    fake = np.zeros(64, dtype=np.uint64)  # stands for an index
    plan = ctypes.c_void_p()
    assert lib.zc_restore_resolve_device(None, None, fake.ctypes.data, ctypes.byref(plan)) == _lib.ZC_ERR_ARG
    assert _err(lib) == name + "null index"
    assert lib.zc_restore_resolve_device(None, fake.ctypes.data, None, ctypes.byref(plan)) == _lib.ZC_ERR_ARG
    assert _err(lib) == name + "null instruction set"
    assert lib.zc_restore_resolve_device(None, fake.ctypes.data, fake.ctypes.data, None) == _lib.ZC_ERR_ARG
    assert _err(lib) == name + "null plan pointer" and not plan.value


def test_replay_argument_errors(lib):
    """n_slots mismatches and the rest, on the plan of an empty stream: zeroed
    memory stands for it (no entries, no used bundles, length 0), as the other
    ABI tests let zeroed memory stand for an index."""
    name = "zc_restore_replay: "
    plan = np.zeros(256, dtype=np.uint64)
    base = (ctypes.c_void_p * 2)(None, None)
    out = np.zeros(16, dtype=np.uint8)
    call = lambda *a: (lib.zc_restore_replay(None, *a), _err(lib))  # noqa: E731
    assert call(None, base, 1, out.ctypes.data, 16) == (_lib.ZC_ERR_ARG, name + "null plan")
    for n_slots in (0, 2, 1 << 40):
        assert call(plan.ctypes.data, base, n_slots, out.ctypes.data, 16) == (
            _lib.ZC_ERR_ARG, name + f"{n_slots} slots, the plan has 0 used bundles and the instruction stream")
    assert call(plan.ctypes.data, None, 1, out.ctypes.data, 16) == (_lib.ZC_ERR_ARG, name + "null slot array")
    # well formed: one slot, NULL because the plan has no bytes_to_emit run, no room needed
    assert call(plan.ctypes.data, base, 1, None, 0) == (_lib.ZC_ERR_ARG, name + "null context")
    assert not out.any()
