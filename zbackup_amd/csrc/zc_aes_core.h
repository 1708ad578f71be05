// AES-128 (FIPS-197) for host and device alike (ZC_HD, as zc_lzo_core.h): the
// tables, the key expansion for both directions, and the single-block encrypt
// and decrypt the CBC kernels of zc_aes.hip are built on.  The CPU unit check
// (tests/aes/aes_core_check.cpp) runs exactly this code against libcrypto.
//
// What zbackup runs: Encryption::encrypt / decrypt (encryption.cc:17-95) =
// OpenSSL's AES-128-CBC over a whole bundle file, key from EncryptionKey.
//
// Everything is derived from the standard's definitions, nothing is copied:
// the S-box is the multiplicative inverse in GF(2^8) mod x^8+x^4+x^3+x+1
// followed by the affine map (FIPS-197 5.1.1); a round is SubBytes, ShiftRows,
// MixColumns, AddRoundKey (5.1); decryption is the equivalent inverse cipher
// (5.3.5) with InvMixColumns applied to round keys 1..9.
//
// Words are little-endian columns: state column j is the 32-bit word
// a0 | a1 << 8 | a2 << 16 | a3 << 24 (rows 0..3), which is how a 16-byte load
// delivers a block, so no byte swaps.  One 1 KiB table per direction:
//   te0[x] = {2 S(x), S(x), S(x), 3 S(x)}            (MixColumns' first column)
//   td0[x] = {14 Si(x), 9 Si(x), 13 Si(x), 11 Si(x)} (InvMixColumns' first column)
// the tables of the other three rows are rotations of these (one v_alignbit).
// The last round's plain S(x) is byte 1 of te0[x]; the inverse cipher's last
// round needs Si(x) on its own (isb).
//
// Lookups go through a caller-supplied accessor T with te(x), td(x), isb(x)
// (x in 0..255), so the kernels can serve them from LDS in whatever layout
// they measured best, and the host check from plain arrays.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

#if defined(__clang__)
#define ZCAES_UNROLL _Pragma("unroll")
#else
#define ZCAES_UNROLL
#endif

namespace zcaes {

constexpr int kRounds = 10;
constexpr int kRkWords = 4 * (kRounds + 1);  // 44

ZC_HD inline uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
ZC_HD inline uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
ZC_HD inline uint8_t gmul(uint8_t a, uint8_t b) {
  uint8_t r = 0;
  for (int i = 0; i < 8; ++i) {
    if (b & 1) r ^= a;
    a = xtime(a);
    b >>= 1;
  }
  return r;
}

struct Tables {
  uint8_t sb[256];
  uint32_t te0[256];
  uint32_t td0[256];
  uint32_t isb[256];  // the inverse S-box, a word per entry (the kernels' LDS layout)
};

// FIPS-197 5.1.1: b = inverse of x (0 -> 0), then b ^ rotl8(b, 1..4) ^ 0x63
inline void make_tables(Tables* t) {
  uint8_t inv[256];
  inv[0] = 0;
  for (int x = 1; x < 256; ++x)
    for (int y = 1; y < 256; ++y)
      if (gmul((uint8_t)x, (uint8_t)y) == 1) {
        inv[x] = (uint8_t)y;
        break;
      }
  for (int x = 0; x < 256; ++x) {
    const uint8_t b = inv[x];
    uint8_t s = b;
    for (int k = 1; k <= 4; ++k) s ^= (uint8_t)((b << k) | (b >> (8 - k)));
    s ^= 0x63;
    t->sb[x] = s;
    t->isb[s] = (uint32_t)x;
  }
  for (int x = 0; x < 256; ++x) {
    const uint8_t s = t->sb[x], si = (uint8_t)t->isb[x];
    t->te0[x] = (uint32_t)xtime(s) | (uint32_t)s << 8 | (uint32_t)s << 16 | (uint32_t)(xtime(s) ^ s) << 24;
    t->td0[x] = (uint32_t)gmul(si, 14) | (uint32_t)gmul(si, 9) << 8 | (uint32_t)gmul(si, 13) << 16 |
                (uint32_t)gmul(si, 11) << 24;
  }
}

// plain-array accessor (host)
struct HostLookup {
  const Tables* t;
  uint32_t te(uint32_t x) const { return t->te0[x]; }
  uint32_t td(uint32_t x) const { return t->td0[x]; }
  uint32_t isb(uint32_t x) const { return t->isb[x]; }
};

// KeyExpansion (FIPS-197 5.2) for Nk = 4: ek[4 r ..+ 4) is round key r
inline void expand_encrypt_key(const Tables& t, const uint8_t key[16], uint32_t ek[kRkWords]) {
  for (int i = 0; i < 4; ++i)
    ek[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 |
            (uint32_t)key[4 * i + 3] << 24;
  uint8_t rc = 1;
  for (int i = 4; i < kRkWords; ++i) {
    uint32_t w = ek[i - 1];
    if (i % 4 == 0) {
      w = (w >> 8) | (w << 24);  // RotWord: {a1, a2, a3, a0}
      w = (uint32_t)t.sb[w & 0xff] | (uint32_t)t.sb[(w >> 8) & 0xff] << 8 | (uint32_t)t.sb[(w >> 16) & 0xff] << 16 |
          (uint32_t)t.sb[w >> 24] << 24;
      w ^= rc;  // Rcon = {rc, 0, 0, 0}
      rc = xtime(rc);
    }
    ek[i] = ek[i - 4] ^ w;
  }
}

// the equivalent inverse cipher's schedule (5.3.5): dk round r = ek round 10 - r,
// InvMixColumns applied for r = 1..9
inline void expand_decrypt_key(const Tables& t, const uint8_t key[16], uint32_t dk[kRkWords]) {
  uint32_t ek[kRkWords];
  expand_encrypt_key(t, key, ek);
  for (int r = 0; r <= kRounds; ++r)
    for (int j = 0; j < 4; ++j) {
      const uint32_t w = ek[4 * (kRounds - r) + j];
      if (r == 0 || r == kRounds) {
        dk[4 * r + j] = w;
        continue;
      }
      const uint8_t a0 = (uint8_t)w, a1 = (uint8_t)(w >> 8), a2 = (uint8_t)(w >> 16), a3 = (uint8_t)(w >> 24);
      dk[4 * r + j] = (uint32_t)(gmul(a0, 14) ^ gmul(a1, 11) ^ gmul(a2, 13) ^ gmul(a3, 9)) |
                      (uint32_t)(gmul(a0, 9) ^ gmul(a1, 14) ^ gmul(a2, 11) ^ gmul(a3, 13)) << 8 |
                      (uint32_t)(gmul(a0, 13) ^ gmul(a1, 9) ^ gmul(a2, 14) ^ gmul(a3, 11)) << 16 |
                      (uint32_t)(gmul(a0, 11) ^ gmul(a1, 13) ^ gmul(a2, 9) ^ gmul(a3, 14)) << 24;
    }
}

// Cipher (5.1) on the block s[0..4) in place.  rk is read at constant indices
// once the loops are unrolled (kernel arguments stay in scalar registers).
template <class RK, class T>
ZC_HD inline void encrypt_block(const RK& rk, const T& t, uint32_t s[4]) {
  uint32_t a0 = s[0] ^ rk[0], a1 = s[1] ^ rk[1], a2 = s[2] ^ rk[2], a3 = s[3] ^ rk[3];
  ZCAES_UNROLL
  for (int r = 1; r < kRounds; ++r) {
    // column j: row i comes from column j + i (ShiftRows)
    const uint32_t b0 = t.te(a0 & 0xff) ^ rotl(t.te((a1 >> 8) & 0xff), 8) ^ rotl(t.te((a2 >> 16) & 0xff), 16) ^
                        rotl(t.te(a3 >> 24), 24) ^ rk[4 * r];
    const uint32_t b1 = t.te(a1 & 0xff) ^ rotl(t.te((a2 >> 8) & 0xff), 8) ^ rotl(t.te((a3 >> 16) & 0xff), 16) ^
                        rotl(t.te(a0 >> 24), 24) ^ rk[4 * r + 1];
    const uint32_t b2 = t.te(a2 & 0xff) ^ rotl(t.te((a3 >> 8) & 0xff), 8) ^ rotl(t.te((a0 >> 16) & 0xff), 16) ^
                        rotl(t.te(a1 >> 24), 24) ^ rk[4 * r + 2];
    const uint32_t b3 = t.te(a3 & 0xff) ^ rotl(t.te((a0 >> 8) & 0xff), 8) ^ rotl(t.te((a1 >> 16) & 0xff), 16) ^
                        rotl(t.te(a2 >> 24), 24) ^ rk[4 * r + 3];
    a0 = b0, a1 = b1, a2 = b2, a3 = b3;
  }
  // last round: no MixColumns; S(x) is byte 1 of te0[x]
#define ZCAES_S(x) ((t.te(x) >> 8) & 0xff)
  s[0] = (ZCAES_S(a0 & 0xff) | ZCAES_S((a1 >> 8) & 0xff) << 8 | ZCAES_S((a2 >> 16) & 0xff) << 16 |
          ZCAES_S(a3 >> 24) << 24) ^ rk[40];
  s[1] = (ZCAES_S(a1 & 0xff) | ZCAES_S((a2 >> 8) & 0xff) << 8 | ZCAES_S((a3 >> 16) & 0xff) << 16 |
          ZCAES_S(a0 >> 24) << 24) ^ rk[41];
  s[2] = (ZCAES_S(a2 & 0xff) | ZCAES_S((a3 >> 8) & 0xff) << 8 | ZCAES_S((a0 >> 16) & 0xff) << 16 |
          ZCAES_S(a1 >> 24) << 24) ^ rk[42];
  s[3] = (ZCAES_S(a3 & 0xff) | ZCAES_S((a0 >> 8) & 0xff) << 8 | ZCAES_S((a1 >> 16) & 0xff) << 16 |
          ZCAES_S(a2 >> 24) << 24) ^ rk[43];
#undef ZCAES_S
}

// EqInvCipher (5.3.5) on the block s[0..4) in place, dk from expand_decrypt_key
template <class RK, class T>
ZC_HD inline void decrypt_block(const RK& dk, const T& t, uint32_t s[4]) {
  uint32_t a0 = s[0] ^ dk[0], a1 = s[1] ^ dk[1], a2 = s[2] ^ dk[2], a3 = s[3] ^ dk[3];
  ZCAES_UNROLL
  for (int r = 1; r < kRounds; ++r) {
    // column j: row i comes from column j - i (InvShiftRows)
    const uint32_t b0 = t.td(a0 & 0xff) ^ rotl(t.td((a3 >> 8) & 0xff), 8) ^ rotl(t.td((a2 >> 16) & 0xff), 16) ^
                        rotl(t.td(a1 >> 24), 24) ^ dk[4 * r];
    const uint32_t b1 = t.td(a1 & 0xff) ^ rotl(t.td((a0 >> 8) & 0xff), 8) ^ rotl(t.td((a3 >> 16) & 0xff), 16) ^
                        rotl(t.td(a2 >> 24), 24) ^ dk[4 * r + 1];
    const uint32_t b2 = t.td(a2 & 0xff) ^ rotl(t.td((a1 >> 8) & 0xff), 8) ^ rotl(t.td((a0 >> 16) & 0xff), 16) ^
                        rotl(t.td(a3 >> 24), 24) ^ dk[4 * r + 2];
    const uint32_t b3 = t.td(a3 & 0xff) ^ rotl(t.td((a2 >> 8) & 0xff), 8) ^ rotl(t.td((a1 >> 16) & 0xff), 16) ^
                        rotl(t.td(a0 >> 24), 24) ^ dk[4 * r + 3];
    a0 = b0, a1 = b1, a2 = b2, a3 = b3;
  }
  s[0] = (t.isb(a0 & 0xff) | t.isb((a3 >> 8) & 0xff) << 8 | t.isb((a2 >> 16) & 0xff) << 16 | t.isb(a1 >> 24) << 24) ^
         dk[40];
  s[1] = (t.isb(a1 & 0xff) | t.isb((a0 >> 8) & 0xff) << 8 | t.isb((a3 >> 16) & 0xff) << 16 | t.isb(a2 >> 24) << 24) ^
         dk[41];
  s[2] = (t.isb(a2 & 0xff) | t.isb((a1 >> 8) & 0xff) << 8 | t.isb((a0 >> 16) & 0xff) << 16 | t.isb(a3 >> 24) << 24) ^
         dk[42];
  s[3] = (t.isb(a3 & 0xff) | t.isb((a2 >> 8) & 0xff) << 8 | t.isb((a1 >> 16) & 0xff) << 16 | t.isb(a0 >> 24) << 24) ^
         dk[43];
}

// ---- the bundle file's arithmetic (encrypted_file.cc:239-392, bundle.cc:96-155) ----

// bytes of a file whose prefix (R + the two messages) is P bytes and body B
inline uint64_t bundle_file_size(uint64_t P, uint64_t B, bool keyed) {
  return keyed ? (P + 4 + B + 4) / 16 * 16 + 16 : P + B + 8;
}

constexpr uint32_t kAdlerBase = 65521;
// zlib's Adler-32 (from 1, or continuing from `ad`) on the host: the prefixes are short
inline uint32_t adler32_host(const uint8_t* p, uint64_t n, uint32_t ad = 1) {
  uint64_t a = ad & 0xffff, b = ad >> 16;
  while (n) {
    const uint64_t k = n < 5552 ? n : 5552;  // sums stay under 2^32
    for (uint64_t i = 0; i < k; ++i) {
      a += p[i];
      b += a;
    }
    a %= kAdlerBase;
    b %= kAdlerBase;
    p += k;
    n -= k;
  }
  return (uint32_t)(b << 16 | a);
}
// Adler-32 of X || Y from those of X and Y (each from 1) and len(Y): with
// a = 1 + sum, b = len + sum of (len - i) x_i, appending Y adds a2 - 1 to a and
// b2 + len2 * (a1 - 1) to b
ZC_HD inline uint32_t adler32_join(uint32_t ad1, uint32_t ad2, uint64_t len2) {
  const uint64_t a1 = ad1 & 0xffff, b1 = ad1 >> 16, a2 = ad2 & 0xffff, b2 = ad2 >> 16;
  const uint64_t a = (a1 + a2 + kAdlerBase - 1) % kAdlerBase;
  const uint64_t b = (b1 + b2 + (len2 % kAdlerBase) * ((a1 + kAdlerBase - 1) % kAdlerBase)) % kAdlerBase;
  return (uint32_t)(b << 16 | a);
}

// What a reader finds in a bundle file's plaintext (bundle.cc:157-218,
// encrypted_file.cc:20-236): status codes of zc_bundle_unseal
constexpr int kBundleOk = 0, kBundleBadSize = 1, kBundleTruncated = 2, kBundleAdler1 = 3, kBundleAdler2 = 4,
              kBundleBadPadding = 5;
struct Parsed {
  int32_t status;
  uint32_t a1, a2;        // the stored Adler-32 values
  uint32_t pad;
  uint64_t header_off, header_len, info_off, info_len, a1_off, body_off, body_len;
};

// Walks one plaintext of `size` bytes (read through byte(i), i < size only).
// Every loop is bounded by a constant (5 varint bytes, 16 pad bytes).
template <class In>
ZC_HD inline void parse_plain(const In& in, uint64_t size, bool keyed, Parsed* out) {
  Parsed p{};
  p.status = kBundleOk;
  uint64_t end = size, pos = 0;
  if (size == 0 || (keyed && size % 16)) {
    p.status = kBundleBadSize;
    *out = p;
    return;
  }
  if (keyed) {
    const uint32_t pad = in.byte(size - 1);
    bool ok = pad >= 1 && pad <= 16;
    for (uint32_t k = 0; k < 16; ++k)
      if (ok && k < pad && in.byte(size - 1 - k) != pad) ok = false;
    if (!ok) {
      p.status = kBundleBadPadding;
      *out = p;
      return;
    }
    p.pad = pad;
    end = size - pad;
    pos = 16;  // R
  }
  bool good = pos <= end;
  for (int m = 0; m < 2 && good; ++m) {
    uint64_t v = 0;
    bool done = false;
    for (int k = 0; k < 5 && good && !done; ++k) {
      if (pos >= end) {
        good = false;
        break;
      }
      const uint32_t b = in.byte(pos++);
      v |= (uint64_t)(b & 0x7f) << (7 * k);
      done = !(b & 0x80);
    }
    if (!done || v > 0xffffffffull || v > end - pos) good = false;
    if (!good) break;
    if (m == 0) {
      p.header_off = pos;
      p.header_len = v;
    } else {
      p.info_off = pos;
      p.info_len = v;
    }
    pos += v;
  }
  if (good && end - pos < 8) good = false;  // A1 and A2
  if (!good) {
    p.status = kBundleTruncated;
    *out = p;
    return;
  }
  p.a1_off = pos;
  p.body_off = pos + 4;
  p.body_len = end - 4 - p.body_off;
  for (int k = 0; k < 4; ++k) {
    p.a1 |= (uint32_t)in.byte(pos + k) << (8 * k);
    p.a2 |= (uint32_t)in.byte(end - 4 + k) << (8 * k);
  }
  *out = p;
}

}  // namespace zcaes
