"""CPU tests of the encryption path:

* zc_aes_core.h -- the AES-128 key expansion and block functions the CBC
  kernels run -- compiled for the host (under ASan + UBSan where that links)
  with a main of its own and compared with libcrypto's AES_encrypt /
  AES_decrypt on the FIPS-197 and SP 800-38A vectors, 10,000 random key /
  block pairs and CBC chains of 1, 2, 3 and 4,097 blocks; the plaintext
  parser on random bytes and, with exact fields, on well-formed plaintexts at
  every pair of varint widths;
* the reference helper's own checks (tests/aes_ref.py runs them on import);
* zc_bundle_file_size at every padding residue, and the new symbols."""
import os
import re
import subprocess

import pytest

from tests import aes_ref
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSL_INC = next((d for d in ("/usr/include", "/opt/conda/include") if os.path.exists(os.path.join(d, "openssl", "aes.h"))),
               None)

NEW_SYMBOLS = ["zc_aes128_cbc_encrypt", "zc_aes128_cbc_decrypt", "zc_aes128_cbc_encrypt_host",
               "zc_aes128_cbc_decrypt_host", "zc_bundle_file_size", "zc_bundle_seal", "zc_bundle_seal_host",
               "zc_bundle_unseal", "zc_bundle_unseal_host", "zc_aes_last_form"]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _build_check(tmp_path):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path / "aes_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-Wno-deprecated-declarations", "-std=c++17",
            "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"), "-I" + SSL_INC,
            os.path.join(ROOT, "tests", "aes", "aes_core_check.cpp")]
    if SSL_INC.startswith("/opt/conda"):
        base += ["-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib"]
    base += ["-lcrypto", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


@pytest.mark.skipif(SSL_INC is None, reason="libcrypto's headers are not in this image")
def test_cipher_core_matches_libcrypto(tmp_path):
    exe, sanitized = _build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    # the cipher and Adler-32 checks, 20,000 random plaintexts, 2 x 150 well-formed ones
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) >= 20000 + 218 + 20000 + 300


def test_reference_helper():
    """aes_ref checked itself on import; its format restatement round-trips."""
    key = bytes(range(16))
    for keyed in (key, None):
        for body_len in range(0, 40):
            prefix = (bytes(range(100, 116)) if keyed else b"") + aes_ref.message(b"hdr") + aes_ref.message(b"i" * 200)
            body = bytes((7 * k) & 0xff for k in range(body_len))
            f = aes_ref.seal_ref(keyed, prefix, body)
            st, lay, plain = aes_ref.unseal_ref(keyed, f)
            assert st == aes_ref.OK
            assert plain[lay["body_off"]:lay["body_off"] + lay["body_len"]] == body
            assert plain[lay["header_off"]:lay["header_off"] + lay["header_len"]] == b"hdr"
            assert lay["info_len"] == 200
    assert aes_ref.unseal_ref(key, b"")[0] == aes_ref.BAD_SIZE
    assert aes_ref.unseal_ref(key, bytes(17))[0] == aes_ref.BAD_SIZE
    if aes_ref.have_libcrypto():
        assert aes_ref.byte_budget() is None
    else:
        assert aes_ref.byte_budget() == 64 << 10


def test_bundle_file_size(lib):
    from zbackup_amd.bundle import bundle_file_size
    seen = set()
    for P in (16, 23, 40):
        for B in range(0, 64):
            r = (P + B + 8) % 16
            seen.add(r)
            keyed, plain = bundle_file_size(P, B, True), bundle_file_size(P, B, False)
            assert plain == P + B + 8 == aes_ref.file_size(P, B, False)
            assert keyed == aes_ref.file_size(P, B, True) and keyed % 16 == 0
            assert 1 <= keyed - plain <= 16
            if r == 0:
                assert keyed == plain + 16  # a whole block of padding
            if r == 1:
                assert keyed == plain + 15
            if r == 15:
                assert keyed == plain + 1
    assert {0, 1, 15} <= seen
    assert bundle_file_size(0, 0, False) == 8 and bundle_file_size(0, 0, True) == 16
    assert bundle_file_size(1 << 20, (1 << 32) + 5, True) == ((1 << 20) + (1 << 32) + 13) // 16 * 16 + 16


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert not set(NEW_SYMBOLS) - exported
    assert not set(NEW_SYMBOLS) - set(_lib.EXPORTS)
    assert lib.zc_abi_version() == 5  # detected by symbol, not by version
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes is not None


def test_last_form_without_a_context(lib):
    import ctypes
    form = ctypes.c_uint32(7)
    assert lib.zc_aes_last_form(None, ctypes.byref(form)) == _lib.ZC_ERR_ARG
    assert b"zc_aes_last_form" in lib.zc_last_error(None) and form.value == 7
    assert (_lib.ZC_AES_FORM_DECRYPT, _lib.ZC_AES_FORM_PLAIN_TABLES, _lib.ZC_AES_FORM_LANE, _lib.ZC_AES_FORM_AHEAD_1,
            _lib.ZC_AES_FORM_CPW_SHIFT) == (1, 2, 4, 8, 8)
    header = open(os.path.join(ROOT, "include", "zchunk.h")).read()
    for name in ("DECRYPT", "PLAIN_TABLES", "LANE", "AHEAD_1", "CPW_SHIFT"):
        value = re.search(r"\bZC_AES_FORM_%s = (\d+)" % name, header).group(1)
        assert int(value) == getattr(_lib, "ZC_AES_FORM_" + name)


def test_null_context_is_an_argument_error_with_a_message(lib):
    """No device is touched: the context is checked first."""
    key = bytes(16)
    assert lib.zc_aes128_cbc_encrypt(None, key, None, None, None, 0, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_aes128_cbc_encrypt" in lib.zc_last_error(None)
    assert lib.zc_bundle_seal(None, key, None, None, 0, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_bundle_seal" in lib.zc_last_error(None)
    assert lib.zc_bundle_unseal(None, key, None, None, None, 0, None, None, None) == _lib.ZC_ERR_ARG
    assert b"zc_bundle_unseal" in lib.zc_last_error(None)
    import ctypes
    n = ctypes.c_size_t()
    assert lib.zc_parse_instructions(b"", 0, None, 0, ctypes.byref(n)) == _lib.ZC_OK  # clears the thread's message
    assert lib.zc_last_error(None) == b"null context"
