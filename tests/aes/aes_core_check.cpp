// CPU unit check of zc_aes_core.h (test infrastructure only): the tables, key
// expansion and both block functions the CBC kernels run, against libcrypto's
// AES_encrypt / AES_decrypt on the FIPS-197 C.1 and SP 800-38A F.2.1 / F.2.2
// vectors and on random key / block pairs; a host CBC loop over the core
// against the library's CBC at 1, 2, 3 and 4,097 blocks; the Adler-32 helpers
// and the plaintext parser: no read past the end on random bytes, and exact
// fields for well-formed plaintexts at every pair of varint widths.  Prints "ok <checks>"; exits non-zero
// on the first difference.
#include <openssl/aes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zc_aes_core.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static void fill(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)rnd();
}
static void unhex(const char* h, uint8_t* out) {
  for (size_t i = 0; h[2 * i]; ++i) {
    unsigned v;
    sscanf(h + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}
static void die(const char* what, long at) {
  printf("MISMATCH %s at %ld\n", what, at);
  exit(1);
}

static zcaes::Tables T;

static void core_encrypt(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  uint32_t rk[zcaes::kRkWords], s[4];
  zcaes::expand_encrypt_key(T, key, rk);
  memcpy(s, in, 16);
  zcaes::encrypt_block(rk, zcaes::HostLookup{&T}, s);
  memcpy(out, s, 16);
}
static void core_decrypt(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  uint32_t rk[zcaes::kRkWords], s[4];
  zcaes::expand_decrypt_key(T, key, rk);
  memcpy(s, in, 16);
  zcaes::decrypt_block(rk, zcaes::HostLookup{&T}, s);
  memcpy(out, s, 16);
}

struct Bytes {
  const uint8_t* p;
  uint32_t byte(uint64_t i) const { return p[i]; }
};

// v as a varint of exactly `width` bytes: above the canonical width the last
// canonical byte gets a continuation bit and 0x80 bytes follow, up to a final 0
static void put_varint(std::vector<uint8_t>& d, uint64_t v, int width) {
  int n = 0;
  do {
    d.push_back((uint8_t)((v & 0x7f) | (v >> 7 || n + 1 < width ? 0x80 : 0)));
    v >>= 7;
    ++n;
  } while (v || n < width);
  if (n != width) die("put_varint width", width);
}
static void put_le32(std::vector<uint8_t>& d, uint32_t v) {
  for (int k = 0; k < 4; ++k) d.push_back((uint8_t)(v >> (8 * k)));
}
// what a reader makes of a plaintext: parse_plain, then both Adler-32s as
// zc_bundle_unseal checks them (the share before A1, joined with the share
// from A1 to A2)
static int reader_status(const std::vector<uint8_t>& d, bool keyed, zcaes::Parsed* p) {
  zcaes::parse_plain(Bytes{d.data()}, d.size(), keyed, p);
  if (p->status != zcaes::kBundleOk) return p->status;
  const uint32_t a1 = zcaes::adler32_host(d.data(), p->a1_off);
  if (a1 != p->a1) return zcaes::kBundleAdler1;
  const uint64_t n2 = 4 + p->body_len;
  if (zcaes::adler32_join(a1, zcaes::adler32_host(d.data() + p->a1_off, n2), n2) != p->a2) return zcaes::kBundleAdler2;
  return zcaes::kBundleOk;
}

int main() {
  zcaes::make_tables(&T);
  long checks = 0;
  // FIPS-197 figure 7: S(0x00) = 0x63, S(0x53) = 0xed
  if (T.sb[0] != 0x63 || T.sb[0x53] != 0xed || T.isb[0x63] != 0) die("sbox", 0);
  uint8_t key[16], in[16], want[16], got[16];
  // FIPS-197 Appendix C.1
  unhex("000102030405060708090a0b0c0d0e0f", key);
  unhex("00112233445566778899aabbccddeeff", in);
  unhex("69c4e0d86a7b0430d8cdb78070b4c55a", want);
  core_encrypt(key, in, got);
  if (memcmp(got, want, 16)) die("FIPS-197 C.1 encrypt", 0);
  core_decrypt(key, want, got);
  if (memcmp(got, in, 16)) die("FIPS-197 C.1 decrypt", 0);
  checks += 2;
  // 10,000 random key / block pairs against the library
  for (int k = 0; k < 10000; ++k) {
    fill(key, 16);
    fill(in, 16);
    AES_KEY ek, dk;
    AES_set_encrypt_key(key, 128, &ek);
    AES_set_decrypt_key(key, 128, &dk);
    AES_encrypt(in, want, &ek);
    core_encrypt(key, in, got);
    if (memcmp(got, want, 16)) die("encrypt_block", k);
    AES_decrypt(in, want, &dk);
    core_decrypt(key, in, got);
    if (memcmp(got, want, 16)) die("decrypt_block", k);
    checks += 2;
  }
  // SP 800-38A F.2.1 / F.2.2 (CBC-AES128), then random chains
  {
    uint8_t iv[16], pt[64], ct[64];
    unhex("2b7e151628aed2a6abf7158809cf4f3c", key);
    unhex("000102030405060708090a0b0c0d0e0f", iv);
    unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
          "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710", pt);
    unhex("7649abac8119b246cee98e9b12e9197d5086cb9b507219ee95db113a917678b2"
          "73bed6b8e3c1743b7116e69e222295163ff1caa1681fac09120eca307586e1a7", ct);
    uint32_t ek[zcaes::kRkWords], dk[zcaes::kRkWords], prev[4], s[4];
    zcaes::expand_encrypt_key(T, key, ek);
    zcaes::expand_decrypt_key(T, key, dk);
    memcpy(prev, iv, 16);
    for (int b = 0; b < 4; ++b) {
      memcpy(s, pt + 16 * b, 16);
      for (int j = 0; j < 4; ++j) s[j] ^= prev[j];
      zcaes::encrypt_block(ek, zcaes::HostLookup{&T}, s);
      if (memcmp(s, ct + 16 * b, 16)) die("SP 800-38A F.2.1", b);
      memcpy(prev, s, 16);
    }
    for (int b = 0; b < 4; ++b) {
      memcpy(s, ct + 16 * b, 16);
      zcaes::decrypt_block(dk, zcaes::HostLookup{&T}, s);
      const uint8_t* pv = b ? ct + 16 * (b - 1) : iv;
      for (int j = 0; j < 16; ++j)
        if ((((uint8_t*)s)[j] ^ pv[j]) != pt[16 * b + j]) die("SP 800-38A F.2.2", b);
    }
    checks += 8;
  }
  for (size_t nblk : {(size_t)1, (size_t)2, (size_t)3, (size_t)4097}) {
    std::vector<uint8_t> pt(16 * nblk), want_ct(16 * nblk), got_ct(16 * nblk), back(16 * nblk);
    uint8_t iv[16], iv2[16];
    fill(key, 16);
    fill(iv, 16);
    fill(pt.data(), pt.size());
    AES_KEY lk;
    AES_set_encrypt_key(key, 128, &lk);
    memcpy(iv2, iv, 16);
    AES_cbc_encrypt(pt.data(), want_ct.data(), pt.size(), &lk, iv2, AES_ENCRYPT);
    uint32_t ek[zcaes::kRkWords], dk[zcaes::kRkWords], prev[4], s[4];
    zcaes::expand_encrypt_key(T, key, ek);
    zcaes::expand_decrypt_key(T, key, dk);
    memcpy(prev, iv, 16);
    for (size_t b = 0; b < nblk; ++b) {
      memcpy(s, pt.data() + 16 * b, 16);
      for (int j = 0; j < 4; ++j) s[j] ^= prev[j];
      zcaes::encrypt_block(ek, zcaes::HostLookup{&T}, s);
      memcpy(got_ct.data() + 16 * b, s, 16);
      memcpy(prev, s, 16);
    }
    if (got_ct != want_ct) die("CBC encrypt", (long)nblk);
    for (size_t b = 0; b < nblk; ++b) {  // any order: every block is independent
      memcpy(s, want_ct.data() + 16 * b, 16);
      zcaes::decrypt_block(dk, zcaes::HostLookup{&T}, s);
      const uint8_t* pv = b ? want_ct.data() + 16 * (b - 1) : iv;
      for (int j = 0; j < 16; ++j) back[16 * b + j] = ((uint8_t*)s)[j] ^ pv[j];
    }
    if (back != pt) die("CBC decrypt", (long)nblk);
    checks += 2;
  }
  // Adler-32: joining two shares equals the Adler-32 of the whole
  for (int k = 0; k < 200; ++k) {
    const size_t n1 = rnd() % 70000, n2 = rnd() % 70000;
    std::vector<uint8_t> d(n1 + n2 + 1);
    fill(d.data(), d.size());
    if (k % 3 == 0) memset(d.data(), 0xff, d.size());
    const uint32_t whole = zcaes::adler32_host(d.data(), n1 + n2);
    const uint32_t a = zcaes::adler32_host(d.data(), n1), b = zcaes::adler32_host(d.data() + n1, n2);
    if (zcaes::adler32_join(a, b, n2) != whole) die("adler32_join", k);
    if (zcaes::adler32_host(d.data() + n1, n2, a) != whole) die("adler32 continue", k);
    ++checks;
  }
  if (zcaes::adler32_host((const uint8_t*)"Wikipedia", 9) != 0x11E60398u) die("adler32 vector", 0);
  // the plaintext parser never reads at or past `size`, whatever the bytes are
  for (int k = 0; k < 20000; ++k) {
    const size_t size = rnd() % 97;
    std::vector<uint8_t> d(size);  // exactly size bytes: a read past the end is a sanitizer error
    fill(d.data(), size);
    if (size && k % 2) d[size - 1] = (uint8_t)(1 + rnd() % 16);
    if (size > 40 && k % 4 == 1) d[16] =(uint8_t)(rnd() % 8), d[17 + d[16]] = (uint8_t)(rnd() % 8);
    zcaes::Parsed p;
    zcaes::parse_plain(Bytes{d.data()}, size, k % 2 != 0, &p);
    if (p.status == zcaes::kBundleOk) {
      if (p.body_off + p.body_len + 4 + p.pad != size) die("parse_plain body end", k);
      if (p.header_off + p.header_len > p.info_off || p.info_off + p.info_len != p.a1_off) die("parse_plain order", k);
    }
    ++checks;
  }
  // well-formed plaintexts, built here: both length varints at every width 1..5
  // (padded with 0x80 continuation bytes above the canonical width) x three
  // (header, info, body) length triples, keyed and plain; every field exact.
  // The same plaintext cut by one keyed block, or by one byte when plain, must
  // not read as a good file.
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int tr = 0; tr < 3; ++tr)
      for (int wh = 1; wh <= 5; ++wh)
        for (int wi = 1; wi <= 5; ++wi) {
          static const uint64_t kTriples[3][3] = {{0, 0, 0}, {2, 5, 1}, {3, 127, 33}};
          const uint64_t H = kTriples[tr][0], I = kTriples[tr][1], B = kTriples[tr][2];
          const long id = ((keyed * 3 + tr) * 5 + (wh - 1)) * 5 + (wi - 1);
          std::vector<uint8_t> d;
          auto put_random = [&](uint64_t n) {
            for (uint64_t k = 0; k < n; ++k) d.push_back((uint8_t)rnd());
          };
          if (keyed) put_random(16);  // R
          const uint64_t start = d.size();
          put_varint(d, H, wh);
          put_random(H);
          put_varint(d, I, wi);
          put_random(I);
          const uint32_t a1 = zcaes::adler32_host(d.data(), d.size());
          put_le32(d, a1);
          put_random(B);
          const uint32_t a2 = zcaes::adler32_host(d.data(), d.size());
          put_le32(d, a2);
          const uint32_t pad = keyed ? 16 - (uint32_t)(d.size() % 16) : 0;
          d.insert(d.end(), pad, (uint8_t)pad);
          if (d.size() != zcaes::bundle_file_size(start + wh + H + wi + I, B, keyed != 0)) die("well-formed size", id);
          zcaes::Parsed p;
          if (reader_status(d, keyed != 0, &p) != zcaes::kBundleOk) die("well-formed status", id);
          if (p.header_off != start + wh || p.header_len != H) die("well-formed header", id);
          if (p.info_off != start + wh + H + wi || p.info_len != I) die("well-formed info", id);
          if (p.a1_off != p.info_off + I || p.body_off != p.a1_off + 4 || p.body_len != B) die("well-formed body", id);
          if (p.pad != pad || p.a1 != a1 || p.a2 != a2) die("well-formed pad / A1 / A2", id);
          if (p.body_off + B + 4 + pad != d.size()) die("well-formed end", id);
          ++checks;
          const std::vector<uint8_t> cut(d.begin(), d.end() - (keyed ? 16 : 1));  // exactly the bytes left
          if (reader_status(cut, keyed != 0, &p) == zcaes::kBundleOk) die("cut file reads as good", id);
          ++checks;
        }
  if (zcaes::bundle_file_size(20, 4, true) != 48 || zcaes::bundle_file_size(20, 3, true) != 32 ||
      zcaes::bundle_file_size(20, 3, false) != 31)
    die("bundle_file_size", 0);
  printf("ok %ld\n", checks);
  return 0;
}
