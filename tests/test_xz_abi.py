"""The LZMA entry points and the three device-memory helpers beside them
(zc_device_alloc, zc_device_free, zc_upload): argument errors that need no
device (no context is made), and the result record's layout."""
import ctypes

import pytest

from zbackup_amd import _build, _lib


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_null_context_is_an_argument_error(lib):
    p = ctypes.c_void_p(0x1234)
    one = (ctypes.c_uint64 * 1)(0)
    res = _lib.ZcXzResult()
    buf = ctypes.create_string_buffer(16)
    for host in (lib.zc_xz_decode, lib.zc_xz_decode_host):
        rc = host(None, buf, one, one, 1, buf, one, one, ctypes.byref(res))
        assert rc == _lib.ZC_ERR_ARG
        assert b"null context" in lib.zc_last_error(None)
    assert lib.zc_xz_last_stats(None, None, None, None, None) == _lib.ZC_ERR_ARG
    assert lib.zc_device_alloc(None, 16, ctypes.byref(p)) == _lib.ZC_ERR_ARG
    assert p.value == 0x1234  # nothing was written through it
    assert b"zc_device_alloc" in lib.zc_last_error(None)
    assert lib.zc_device_free(None, None) == _lib.ZC_ERR_ARG
    assert b"zc_device_free" in lib.zc_last_error(None)
    assert lib.zc_upload(None, buf, buf, 16) == _lib.ZC_ERR_ARG
    assert b"zc_upload" in lib.zc_last_error(None)


def test_result_layout_matches_the_header():
    assert ctypes.sizeof(_lib.ZcXzResult) == 24
    assert [(_lib.ZcXzResult.status.offset), _lib.ZcXzResult.info.offset, _lib.ZcXzResult.decoded.offset,
            _lib.ZcXzResult.consumed.offset] == [0, 4, 8, 16]
    assert sorted(_lib.XZ_STATUS_NAMES) == list(range(9))
