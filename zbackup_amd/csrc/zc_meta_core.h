// The content-anchor metadata record of one chunk, as a function of its bytes
// alone, for host and device alike (ZC_HD, as zc_gc_core.h and zc_aes_core.h):
// the scalar definition zc_meta.hip's kernels are checked against, the pieces
// of it those kernels run themselves (the gear step, the anchor test, the
// powers of 257, the id comparison), and the record's assembly.  The CPU unit
// check (tests/meta/meta_core_check.cpp) runs exactly this code against a
// plain-Python restatement.
//
// What it restates: the record zc_export_chunk_meta writes for a chunk a
// context cut itself, which there comes out of the scan's anchor
// pool and span digests.  Here the chunk is b[0, size) wherever it lies, under
// a context with chunk.max_size W:
//   rolling      257^size + sum b[i] 257^(size-1-i) mod 2^64 (RollingHash::digest)
//   sha1         the first 16 bytes of SHA-1(b)             (ChunkId::cryptoHash)
//   anchor       the smallest q in [63, W-1] with (int16)st(q) >= anchor_lo_for(W),
//                st(q) = sum_{j<16} b[q-2j] 2^j mod 2^16; only when size == W > 63
//   gear         st(q-1) | st(q) << 16
//   fingerprint  b[q-7 .. q] as a little-endian 64-bit word
// The anchor rate and threshold follow the context's W, never the chunk's size.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcmeta {

constexpr uint32_t kAnchorMinOff = 63;         // ZC_ANCHOR_MIN_OFF
constexpr uint32_t kNoAnchor = 0xFFFFFFFFu;    // ZC_META_NO_ANCHOR
enum { kBadSha1 = 1, kBadRolling = 2, kBadSize = 4 };  // ZC_META_BAD_*

// include/zchunk.h's zc_chunk_meta and zc_seed, field for field (the check
// program includes no other header of the library)
struct Record {
  uint8_t sha1[16];
  uint64_t rolling;
  uint32_t size;
  uint32_t anchor_def;
  uint32_t anchor;
  uint32_t gear;
  uint64_t fingerprint;
};
struct Expect {
  uint8_t sha1[16];
  uint64_t rolling;
  uint32_t size;
  uint32_t reserved;
};
static_assert(sizeof(Record) == 48 && sizeof(Expect) == 32, "record layout");

// the anchor rate for W (a W-byte chunk holds ~16 anchors), its threshold and
// the definition word metadata carries (zc_anchor_def): zc_device.h's
// anchor_rate_inv / anchor_lo_for and the engine's anchor_def_of
ZC_HD inline uint32_t anchor_rate_inv(uint32_t W) {
  uint32_t rate_inv = 16;
  while (rate_inv < 4096 && rate_inv * 2 <= W / 16) rate_inv *= 2;
  return rate_inv;
}
ZC_HD inline int32_t anchor_lo_for(uint32_t W) { return (int32_t)(0x8000u - 0x10000u / anchor_rate_inv(W)); }
ZC_HD inline uint32_t anchor_def(uint32_t W) {
  uint32_t log2 = 0;
  while ((1u << log2) < anchor_rate_inv(W)) ++log2;
  return 0x5A410000u | (2u << 8) | log2;
}

// 257^e mod 2^64, 32 squarings whatever e is
ZC_HD inline uint64_t pow257(uint32_t e) {
  uint64_t r = 1, b = 257;
  for (int i = 0; i < 32; ++i) {
    if ((e >> i) & 1u) r *= b;
    b *= b;
  }
  return r;
}

// One byte of the anchor state {st(q-1), st(q) << 16}: st(q+1) = 2 st(q-1) + b
ZC_HD inline uint32_t gear_step(uint32_t g, uint32_t b) { return (g >> 16) | (((g << 1) + b) << 16); }
ZC_HD inline bool anchor_hit(uint32_t g, int32_t lo) { return (int32_t)g >> 16 >= lo; }

ZC_HD inline uint64_t rolling(const uint8_t* b, uint32_t size) {
  uint64_t acc = 0;
  for (uint32_t i = 0; i < size; ++i) acc = acc * 257u + b[i];
  return pow257(size) + acc;
}

// the first anchor of b[0, size) under W; false: none (fields as the export writes them)
ZC_HD inline bool first_anchor(const uint8_t* b, uint32_t size, uint32_t W, uint32_t* anchor, uint32_t* gear,
                               uint64_t* fingerprint) {
  *anchor = kNoAnchor;
  *gear = 0;
  *fingerprint = 0;
  if (size != W || W <= kAnchorMinOff) return false;
  const int32_t lo = anchor_lo_for(W);
  uint32_t g = 0;
  // the state at q covers b[q-30, q]: from q = 63 on no byte before the chunk is in it
  for (uint32_t q = kAnchorMinOff - 31; q < size; ++q) {
    g = gear_step(g, b[q]);
    if (q >= kAnchorMinOff && anchor_hit(g, lo)) {
      uint64_t f = 0;
      for (int k = 0; k < 8; ++k) f |= (uint64_t)b[q - 7 + k] << (8 * k);
      *anchor = q;
      *gear = g;
      *fingerprint = f;
      return true;
    }
  }
  return false;
}

// SHA-1 (FIPS 180-4) of b[0, size), the scalar way
ZC_HD inline uint32_t rotl32(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
ZC_HD inline void sha1_block(uint32_t* st, const uint8_t* p) {
  uint32_t w[80];
  for (int t = 0; t < 16; ++t)
    w[t] = (uint32_t)p[4 * t] << 24 | (uint32_t)p[4 * t + 1] << 16 | (uint32_t)p[4 * t + 2] << 8 | p[4 * t + 3];
  for (int t = 16; t < 80; ++t) w[t] = rotl32(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1);
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
  for (int t = 0; t < 80; ++t) {
    uint32_t f, k;
    if (t < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
    else if (t < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
    else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
    else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
    const uint32_t tmp = rotl32(a, 5) + f + e + k + w[t];
    e = d; d = c; c = rotl32(b, 30); b = a; a = tmp;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}
ZC_HD inline void sha1(const uint8_t* b, uint64_t size, uint8_t out[20]) {
  uint32_t st[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
  uint64_t i = 0;
  for (; i + 64 <= size; i += 64) sha1_block(st, b + i);
  uint8_t last[128];
  const uint32_t rem = (uint32_t)(size - i), n = rem + 9 <= 64 ? 64u : 128u;
  for (uint32_t k = 0; k < n; ++k) last[k] = k < rem ? b[i + k] : k == rem ? 0x80 : 0;
  const uint64_t bits = size * 8;
  for (int k = 0; k < 8; ++k) last[n - 1 - k] = (uint8_t)(bits >> (8 * k));
  sha1_block(st, last);
  if (n == 128) sha1_block(st, last + 64);
  for (int k = 0; k < 5; ++k) {
    out[4 * k] = (uint8_t)(st[k] >> 24);
    out[4 * k + 1] = (uint8_t)(st[k] >> 16);
    out[4 * k + 2] = (uint8_t)(st[k] >> 8);
    out[4 * k + 3] = (uint8_t)st[k];
  }
}

// The record from its parts (sha: at least 16 bytes), and what differs from an expected id
ZC_HD inline Record make_record(const uint8_t* sha, uint64_t rolling_v, uint32_t size, uint32_t def, uint32_t anchor,
                                uint32_t gear, uint64_t fingerprint) {
  Record r;
  for (int k = 0; k < 16; ++k) r.sha1[k] = sha[k];
  r.rolling = rolling_v;
  r.size = size;
  r.anchor_def = def;
  r.anchor = anchor;
  r.gear = anchor == kNoAnchor ? 0u : gear;
  r.fingerprint = anchor == kNoAnchor ? 0ull : fingerprint;
  return r;
}
ZC_HD inline uint32_t compare(const Record& r, const Expect& e) {
  uint32_t diff = 0;
  for (int k = 0; k < 16; ++k) diff |= (uint32_t)(r.sha1[k] ^ e.sha1[k]);
  return (diff ? (uint32_t)kBadSha1 : 0u) | (r.rolling != e.rolling ? (uint32_t)kBadRolling : 0u) |
         (r.size != e.size ? (uint32_t)kBadSize : 0u);
}

// the whole definition: the record of chunk b[0, size) under chunk.max_size W
ZC_HD inline Record chunk_record(const uint8_t* b, uint32_t size, uint32_t W) {
  uint8_t h[20];
  sha1(b, size, h);
  uint32_t anchor, gear;
  uint64_t fp;
  first_anchor(b, size, W, &anchor, &gear, &fp);
  return make_record(h, rolling(b, size), size, anchor_def(W), anchor, gear, fp);
}

}  // namespace zcmeta
