"""Reference for the AES tests: a pure-Python AES-128 written from FIPS-197
(always available), a ctypes wrapper over the machine's libcrypto (used when
it loads: EVP_aes_128_cbc with padding off), and a Python restatement of the
bundle file format (seal_ref / unseal_ref):

  [R: 16 random bytes, keyed only] header message, info message, A1, body, A2
  [PKCS#7 padding of 1..16 bytes, keyed only]; each message = varint32 length +
  bytes; A1 / A2 = little-endian zlib Adler-32 of everything before them; with
  a key the file is one AES-128-CBC chain from the zero IV.

Importing the module checks the helper against the FIPS-197 C.1 and SP 800-38A
F.2.1 / F.2.2 vectors, and pure Python against libcrypto when both exist."""
import ctypes
import ctypes.util
import struct
import zlib

OK, BAD_SIZE, TRUNCATED, BAD_ADLER1, BAD_ADLER2, BAD_PADDING = 0, 1, 2, 3, 4, 5

# ---- pure Python, from FIPS-197 ----


def _xtime(a):
    return ((a << 1) ^ (0x1b if a & 0x80 else 0)) & 0xff


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _make_sbox():
    sbox = [0] * 256
    for x in range(256):
        inv = 0 if x == 0 else next(y for y in range(1, 256) if _gmul(x, y) == 1)
        s = inv
        for k in range(1, 5):
            s ^= ((inv << k) | (inv >> (8 - k))) & 0xff
        sbox[x] = s ^ 0x63
    return sbox


SBOX = _make_sbox()
INV_SBOX = [0] * 256
for _x, _s in enumerate(SBOX):
    INV_SBOX[_s] = _x
_MUL = {c: [_gmul(x, c) for x in range(256)] for c in (2, 3, 9, 11, 13, 14)}


def expand_key(key):
    """The 11 round keys (16 bytes each) of a 16-byte key (FIPS-197 5.2)."""
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rc = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rc
            rc = _xtime(rc)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


# state = 16 bytes in the input's order: byte 4 c + r is row r of column c
_SHIFT = [4 * ((c + r) % 4) + r for c in range(4) for r in range(4)]
_INV_SHIFT = [4 * ((c - r) % 4) + r for c in range(4) for r in range(4)]


def _mix(s, m):
    out = []
    for c in range(4):
        col = s[4 * c:4 * c + 4]
        for r in range(4):
            v = 0
            for k in range(4):
                f = m[(k - r) % 4]
                v ^= col[k] if f == 1 else _MUL[f][col[k]]
            out.append(v)
    return out


def encrypt_block(rks, block):
    s = [a ^ b for a, b in zip(block, rks[0])]
    for r in range(1, 11):
        s = [SBOX[s[i]] for i in _SHIFT]
        if r < 10:
            s = _mix(s, (2, 3, 1, 1))
        s = [a ^ b for a, b in zip(s, rks[r])]
    return bytes(s)


def decrypt_block(rks, block):
    s = [a ^ b for a, b in zip(block, rks[10])]
    for r in range(9, -1, -1):
        s = [INV_SBOX[s[i]] for i in _INV_SHIFT]
        s = [a ^ b for a, b in zip(s, rks[r])]
        if r > 0:
            s = _mix(s, (14, 11, 13, 9))
    return bytes(s)


def py_cbc_encrypt(key, iv, data):
    rks, prev, out = expand_key(key), bytes(iv), bytearray()
    for i in range(0, len(data), 16):
        prev = encrypt_block(rks, bytes(a ^ b for a, b in zip(data[i:i + 16], prev)))
        out += prev
    return bytes(out)


def py_cbc_decrypt(key, iv, data):
    rks, prev, out = expand_key(key), bytes(iv), bytearray()
    for i in range(0, len(data), 16):
        c = data[i:i + 16]
        out += bytes(a ^ b for a, b in zip(decrypt_block(rks, c), prev))
        prev = c
    return bytes(out)


# ---- libcrypto ----

def _load_libcrypto():
    for name in ("libcrypto.so.3", ctypes.util.find_library("crypto"), "/opt/conda/lib/libcrypto.so.1.1",
                 "libcrypto.so.1.1"):
        if not name:
            continue
        try:
            L = ctypes.CDLL(name)
            L.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
            L.EVP_aes_128_cbc.restype = ctypes.c_void_p
            L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
            L.EVP_CipherInit_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                                            ctypes.c_char_p, ctypes.c_int]
            L.EVP_CIPHER_CTX_set_padding.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.EVP_CipherUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                           ctypes.c_void_p, ctypes.c_int]
            return L
        except (OSError, AttributeError):
            continue
    return None


_CRYPTO = _load_libcrypto()


def have_libcrypto():
    return _CRYPTO is not None


def _evp(key, iv, data, enc):
    L = _CRYPTO
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        if L.EVP_CipherInit_ex(ctx, L.EVP_aes_128_cbc(), None, bytes(key), bytes(iv), enc) != 1:
            raise RuntimeError("EVP_CipherInit_ex failed")
        L.EVP_CIPHER_CTX_set_padding(ctx, 0)
        data = bytes(data)
        out = ctypes.create_string_buffer(len(data) + 16)
        pos = 0
        for i in range(0, len(data), 1 << 30):  # the length argument is an int
            piece = data[i:i + (1 << 30)]
            n = ctypes.c_int()
            if L.EVP_CipherUpdate(ctx, ctypes.byref(out, pos), ctypes.byref(n), piece, len(piece)) != 1:
                raise RuntimeError("EVP_CipherUpdate failed")
            pos += n.value
        assert pos == len(data)
        return out.raw[:pos]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def cbc_encrypt(key, iv, data):
    """AES-128-CBC without padding; len(data) a multiple of 16."""
    assert len(key) == 16 and len(iv) == 16 and len(data) % 16 == 0
    return _evp(key, iv, data, 1) if _CRYPTO else py_cbc_encrypt(key, iv, data)


def cbc_decrypt(key, iv, data):
    assert len(key) == 16 and len(iv) == 16 and len(data) % 16 == 0
    return _evp(key, iv, data, 0) if _CRYPTO else py_cbc_decrypt(key, iv, data)


def byte_budget():
    """Bytes the byte-compare cases may put through the reference in total:
    unbounded with libcrypto, 64 KiB with the pure-Python cipher."""
    return None if _CRYPTO else 64 << 10


# ---- the bundle file ----

def varint(v):
    out = bytearray()
    while True:
        if v < 0x80:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7f) | 0x80)
        v >>= 7


def message(payload):
    return varint(len(payload)) + bytes(payload)


def file_size(prefix_len, body_len, keyed):
    return (prefix_len + 4 + body_len + 4) // 16 * 16 + 16 if keyed else prefix_len + body_len + 8


def plaintext_ref(prefix, body, keyed):
    """The plaintext image: prefix (R + both messages), A1, body, A2, padding."""
    p = bytes(prefix)
    p += struct.pack("<I", zlib.adler32(p))
    p += bytes(body)
    p += struct.pack("<I", zlib.adler32(p))
    if keyed:
        n = 16 - len(p) % 16
        p += bytes([n]) * n
    return p


def encrypt_file(key, plain):
    return cbc_encrypt(key, bytes(16), plain) if key is not None else bytes(plain)


def seal_ref(key, prefix, body):
    out = encrypt_file(key, plaintext_ref(prefix, body, key is not None))
    assert len(out) == file_size(len(prefix), len(body), key is not None)
    return out


def _read_varint(p, pos, end):
    v = 0
    for k in range(5):
        if pos >= end:
            return None, pos
        b = p[pos]
        pos += 1
        v |= (b & 0x7f) << (7 * k)
        if not b & 0x80:
            return (v if v <= 0xffffffff else None), pos
    return None, pos


def unseal_ref(key, data):
    """(status, layout dict, plaintext): what a reader finds in one file."""
    keyed = key is not None
    if len(data) == 0 or (keyed and len(data) % 16):
        return BAD_SIZE, {}, b""
    p = cbc_decrypt(key, bytes(16), data) if keyed else bytes(data)
    end, pos = len(p), 0
    if keyed:
        n = p[-1]
        if not 1 <= n <= 16 or p[-n:] != bytes([n]) * n:
            return BAD_PADDING, {}, p
        end, pos = len(p) - n, 16
    lay = {}
    if pos > end:
        return TRUNCATED, lay, p
    for name in ("header", "info"):
        v, pos = _read_varint(p, pos, end)
        if v is None or v > end - pos:
            return TRUNCATED, lay, p
        lay[name + "_off"], lay[name + "_len"] = pos, v
        pos += v
    if end - pos < 8:
        return TRUNCATED, lay, p
    lay["body_off"], lay["body_len"] = pos + 4, end - 4 - (pos + 4)
    if struct.unpack_from("<I", p, pos)[0] != zlib.adler32(p[:pos]):
        return BAD_ADLER1, lay, p
    if struct.unpack_from("<I", p, end - 4)[0] != zlib.adler32(p[:end - 4]):
        return BAD_ADLER2, lay, p
    return OK, lay, p


# ---- the helper checks itself ----

def _self_check():
    h = bytes.fromhex
    key = h("000102030405060708090a0b0c0d0e0f")
    blk = h("00112233445566778899aabbccddeeff")
    assert encrypt_block(expand_key(key), blk) == h("69c4e0d86a7b0430d8cdb78070b4c55a"), "FIPS-197 C.1"
    assert decrypt_block(expand_key(key), h("69c4e0d86a7b0430d8cdb78070b4c55a")) == blk, "FIPS-197 C.1 inverse"
    for enc, dec in ((py_cbc_encrypt, py_cbc_decrypt), (cbc_encrypt, cbc_decrypt)):
        assert enc(F2_KEY, F2_IV, F2_PLAIN) == F2_CIPHER, "SP 800-38A F.2.1"
        assert dec(F2_KEY, F2_IV, F2_CIPHER) == F2_PLAIN, "SP 800-38A F.2.2"
    if _CRYPTO:
        import random
        r = random.Random(5)
        for n in (16, 48, 1024):
            k, iv, d = (bytes(r.getrandbits(8) for _ in range(m)) for m in (16, 16, n))
            c = py_cbc_encrypt(k, iv, d)
            assert c == cbc_encrypt(k, iv, d) and py_cbc_decrypt(k, iv, c) == d == cbc_decrypt(k, iv, c)


F2_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
F2_IV = bytes.fromhex("000102030405060708090a0b0c0d0e0f")
F2_PLAIN = bytes.fromhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
                         "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
F2_CIPHER = bytes.fromhex("7649abac8119b246cee98e9b12e9197d5086cb9b507219ee95db113a917678b2"
                          "73bed6b8e3c1743b7116e69e222295163ff1caa1681fac09120eca307586e1a7")
C1_KEY = bytes.fromhex("000102030405060708090a0b0c0d0e0f")
C1_PLAIN = bytes.fromhex("00112233445566778899aabbccddeeff")
C1_CIPHER = bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")

_self_check()
