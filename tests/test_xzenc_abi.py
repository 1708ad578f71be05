"""The LZMA encoder's entry points: argument errors that need no device (no
context is made, or the error comes before any device work), n == 0, the
result record's layout, and zc_xz_capacity."""
import ctypes
import os
import re

import numpy as np
import pytest

from zbackup_amd import _build, _lib
from zbackup_amd import bundle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_null_context_is_an_argument_error(lib):
    one = (ctypes.c_uint64 * 1)(0)
    cap = (ctypes.c_uint64 * 1)(64)
    res = _lib.ZcXzEncResult()
    buf = ctypes.create_string_buffer(128)
    for fn in (lib.zc_xz_encode, lib.zc_xz_encode_host):
        rc = fn(None, buf, one, one, 1, buf, one, cap, 4, ctypes.byref(res))
        assert rc == _lib.ZC_ERR_ARG
        assert b"null context" in lib.zc_last_error(None)
    assert lib.zc_xz_encode_last_stats(None, None, None, None, None) == _lib.ZC_ERR_ARG
    assert lib.zc_xz_encode_last_schedule(None, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_xz_encode_last_schedule: null context" in lib.zc_last_error(None)


def test_result_layout_matches_the_header():
    assert ctypes.sizeof(_lib.ZcXzEncResult) == 16
    assert [_lib.ZcXzEncResult.status.offset, _lib.ZcXzEncResult.info.offset, _lib.ZcXzEncResult.size.offset] == [0, 4, 8]
    assert B.XZ_ENC_RESULT_DTYPE.itemsize == 16
    with open(os.path.join(ROOT, "include", "zchunk.h")) as f:
        m = re.search(r"typedef struct zc_xz_enc_result \{(.*?)\} zc_xz_enc_result;", f.read(), re.S)
    fields = re.findall(r"^\s*(u?int\d+_t) (\w+);", m.group(1), re.M)
    assert fields == [("int32_t", "status"), ("uint32_t", "info"), ("uint64_t", "size")]


def test_capacity(lib):
    """container + 3 bytes per 64 KiB + payload; the empty stream has no block."""
    assert lib.zc_xz_capacity(0) == 32
    assert lib.zc_xz_capacity(1) == 1 + 3 + 64
    assert lib.zc_xz_capacity(65536) == 65536 + 3 + 64
    assert lib.zc_xz_capacity(65537) == 65537 + 6 + 64


def _u64(*v):
    return np.array(v, dtype=np.uint64)


@pytest.mark.gpu
def test_argument_errors_come_with_a_message_and_before_any_device_work(lib):
    """The errors are found on the host from the arrays alone: the pointers
    below are never dereferenced (they are not device memory)."""
    with B.BundleCompressor() as bc:
        L, ctx = bc._L, bc._ctx
        base = 1 << 40  # an address, never touched
        res = np.zeros(2, dtype=B.XZ_ENC_RESULT_DTYPE)

        def call(pay=base, out=base + (1 << 30), pay_off=_u64(0, 1000), pay_size=_u64(1000, 1000),
                 out_off=_u64(0, 2000), out_cap=_u64(2000, 2000), check=4, n=2, r=res.ctypes.data, host=False):
            fn = L.zc_xz_encode_host if host else L.zc_xz_encode
            rc = fn(ctx, pay, pay_off.ctypes.data if pay_off is not None else None,
                    pay_size.ctypes.data if pay_size is not None else None, n, out,
                    out_off.ctypes.data if out_off is not None else None,
                    out_cap.ctypes.data if out_cap is not None else None, check, r)
            return rc, L.zc_last_error(ctx)

        for host in (False, True):
            for kw in (dict(pay=None), dict(out=None), dict(pay_off=None), dict(pay_size=None), dict(out_off=None),
                       dict(out_cap=None), dict(r=None)):
                rc, msg = call(host=host, **kw)
                assert rc == _lib.ZC_ERR_ARG and b"null pointer" in msg, kw
            for check in (2, 3, 5, 10, 16):
                rc, msg = call(host=host, check=check)
                assert rc == _lib.ZC_ERR_ARG and b"check id" in msg
            rc, msg = call(host=host, out_off=_u64(0, 1999))
            assert rc == _lib.ZC_ERR_ARG and b"overlap" in msg
            rc, msg = call(host=host, out=base, out_off=_u64(5000, 1999))
            assert rc == _lib.ZC_ERR_ARG and b"touches the payload" in msg
            rc, msg = call(host=host, out=base, out_off=_u64(5000, 999), out_cap=_u64(10, 1))
            assert rc == _lib.ZC_ERR_ARG and b"touches the payload" in msg
            rc, msg = call(host=host, pay_size=_u64(1000, (64 << 20) + 1))
            assert rc == _lib.ZC_ERR_ARG and b"64 MiB" in msg
            # an empty call is fine whatever the pointers are, and launches nothing
            rc, msg = call(host=host, n=0, pay=None, out=None, r=None)
            assert rc == _lib.ZC_OK
        assert bc.xz_last_stats() == dict(match_ms=0.0, code_ms=0.0, check_ms=0.0, total_ms=0.0, batches=0,
                                          max_rounds=0, generation=0)
        # every output of the schedule is optional, alone and together
        b, r, g = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7)
        assert L.zc_xz_encode_last_schedule(ctx, None, None, None) == _lib.ZC_OK
        assert L.zc_xz_encode_last_schedule(ctx, ctypes.byref(b), None, None) == _lib.ZC_OK and b.value == 0
        assert L.zc_xz_encode_last_schedule(ctx, None, ctypes.byref(r), None) == _lib.ZC_OK and r.value == 0
        assert L.zc_xz_encode_last_schedule(ctx, None, None, ctypes.byref(g)) == _lib.ZC_OK and g.value == 0
