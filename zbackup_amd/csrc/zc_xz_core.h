// xz / LZMA2 / LZMA decoding for the restore and adoption paths, written for
// host and device alike (ZC_HD, as zc_lzo_dec.h and zc_index_core.h): the GPU
// bundle decoder (zc_xz.hip) runs exactly what the CPU unit check
// (tests/xz/xz_core_check.cpp, test infrastructure only) compares with liblzma.
//
// What zbackup runs: Bundle::Creator compresses a bundle's payload with
// lzma_easy_encoder(6, LZMA_CHECK_CRC64) (compression.cc:78-97) and
// Bundle::Reader decodes it with lzma_stream_decoder(UINT64_MAX, 0) into a
// buffer of the size BundleInfo gives (compression.cc:99-107, bundle.cc:179-216).
// The decoder here is written from the xz file format (1.0.4) and the LZMA2 /
// LZMA descriptions, not from a library.
//
// The container, narrower than liblzma on purpose (as the index reader is
// narrower than libprotobuf): one stream of zero or one block whose only
// filter is LZMA2, check id 0 (none), 1 (CRC32) or 4 (CRC64).  More blocks,
// other filter chains, check id 10 (SHA-256) and a second stream behind stream
// padding are kUnsupported; liblzma reads them, zbackup writes none of them.
// Everything else is checked as the format asks: every CRC32, the block's
// padding, its optional size fields, the index record against the block's real
// sizes, the backward size against the index, the footer's flags against the
// header's.  Bytes after the footer that do not start another stream are not
// looked at: Result::consumed says where the stream ended, and the caller
// compares it with what it handed in.
//
// Statuses and liblzma's classes (lzma_stream_buffer_decode):
//   kFormat       LZMA_FORMAT_ERROR (7)
//   kUnsupported  none: liblzma returns LZMA_OK, or LZMA_OPTIONS_ERROR (8) for
//                 reserved header bits
//   kHeader, kData, kCheck   LZMA_DATA_ERROR (9)
//   kInput        LZMA_BUF_ERROR (10) by the table of the format; the buffer
//                 call itself reports input that ends early as 9
//   kOutput       LZMA_BUF_ERROR (10): the reference's exTooMuchData
//   kBudget       never: the walk's trip count ran out
//
// decode() walks the stream and writes the payload through a sink; it does
// not compute the payload's check, it reports its id and stored value
// (Result::check_id / stored), and the caller compares (check_of on the host,
// zc_xz_check_kernel on the device).
//
//   in.byte(i)                     only for i < in_size
//   probs.ld(i) / .st(i, v)        16-bit probabilities, i < probs.cap()
//   probs.fill(n)                  every one of the first n to 1024
//   out.lit(pos, b)                out[pos] = b
//   out.get(pos)                   out[pos], pos below the write position
//   out.copy(pos, dist, len)       out[pos + k] = out[pos - dist + k % dist], k < len
//   out.stored(src, pos, len)      out[pos + k] = in[src + k]
// Every op the walk hands the sink is validated first: pos + len <= cap, 1 <=
// dist <= pos, src + len <= in_size.  That is the memory-safety argument of the
// device decoder: its sink touches only what the walk proved in range.
//
// Termination: one loop.  A trip reads a chunk header (at least four input
// bytes), decodes one symbol (at least one output byte) or ends the walk, so
// out_cap + in_size + 64 trips, fixed before the walk, bound it whatever the
// bytes are; every other loop has a constant trip count or one taken from a
// validated size field.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif
// Every function of the walk is inlined into its caller on the device: the
// walk's state then lives in scalar registers, not behind a pointer in scratch.
#if defined(__HIP_DEVICE_COMPILE__)
#define ZC_XZ_FN ZC_HD inline __attribute__((always_inline))
#else
#define ZC_XZ_FN ZC_HD inline
#endif

namespace zcxz {

constexpr int kOk = 0, kFormat = 1, kUnsupported = 2, kHeader = 3, kData = 4, kInput = 5, kOutput = 6, kCheck = 7,
              kBudget = 8;
// not a status of the interface: the properties need more probabilities than probs.cap()
constexpr int kNeedWide = 100;

constexpr uint32_t kCheckNone = 0, kCheckCrc32 = 1, kCheckCrc64 = 4, kCheckSha256 = 10;

// the probability array's layout
constexpr uint32_t kStates = 12, kPosStatesMax = 16;
constexpr uint32_t kIsMatch = 0;                                      // [state][pos_state]
constexpr uint32_t kIsRep = kIsMatch + kStates * kPosStatesMax;       // [state]
constexpr uint32_t kIsRep0 = kIsRep + kStates;
constexpr uint32_t kIsRep1 = kIsRep0 + kStates;
constexpr uint32_t kIsRep2 = kIsRep1 + kStates;
constexpr uint32_t kIsRep0Long = kIsRep2 + kStates;                   // [state][pos_state]
constexpr uint32_t kDistSlot = kIsRep0Long + kStates * kPosStatesMax; // [4][64]
constexpr uint32_t kDistSpecial = kDistSlot + 4 * 64;                 // 128 - 14 of them
constexpr uint32_t kDistAlign = kDistSpecial + 114;                   // 16
constexpr uint32_t kLenChoice = 0, kLenChoice2 = 1, kLenLow = 2, kLenMid = kLenLow + 16 * 8,
                   kLenHigh = kLenMid + 16 * 8, kLenSize = kLenHigh + 256;
constexpr uint32_t kMatchLen = kDistAlign + 16;
constexpr uint32_t kRepLen = kMatchLen + kLenSize;
constexpr uint32_t kLiteral = kRepLen + kLenSize;                     // 0x300 << (lc + lp)
static_assert(kLiteral == 1846, "the LZMA probability count");
ZC_HD constexpr uint32_t prob_count(uint32_t lclp) { return kLiteral + (0x300u << lclp); }
constexpr uint32_t kProbsCommon = 1846 + (0x300u << 3);  // lc + lp <= 3: every liblzma preset
constexpr uint32_t kProbsWide = 1846 + (0x300u << 4);    // LZMA2's limit, lc + lp = 4

constexpr uint32_t kMatchLenMax = 273;

struct Result {
  int status;
  uint32_t check_id;  // the stream's (valid once the header was read)
  uint64_t stored;    // the block's stored check value (status kOk, a block present)
  uint64_t decoded;   // bytes written to the sink
  uint64_t consumed;  // bytes of input up to and including the footer (status kOk)
};

// ---- the checks ----

constexpr uint32_t kPoly32 = 0xEDB88320u;
constexpr uint64_t kPoly64 = 0xC96C5795D7870F42ull;

// table entry t of the reflected bytewise CRC
ZC_XZ_FN uint32_t crc32_entry(uint32_t t) {
  uint32_t r = t;
  for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (kPoly32 & (0u - (r & 1)));
  return r;
}
ZC_XZ_FN uint64_t crc64_entry(uint32_t t) {
  uint64_t r = t;
  for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (kPoly64 & (0ull - (r & 1)));
  return r;
}
// one byte into a raw (unconditioned) CRC, without a table
ZC_XZ_FN uint32_t crc32_byte(uint32_t c, uint32_t b) { return crc32_entry((c ^ b) & 0xff) ^ (c >> 8); }
ZC_XZ_FN uint64_t crc64_byte(uint64_t c, uint32_t b) { return crc64_entry((uint32_t)(c ^ b) & 0xff) ^ (c >> 8); }

// Polynomials over GF(2) modulo the CRC's, in the reflected order: the top
// bit is x^0.  T = uint32_t with kPoly32, uint64_t with kPoly64.
template <class T>
ZC_XZ_FN T gf_mul(T a, T b, T poly) {
  const int W = (int)sizeof(T) * 8;
  T p = 0;
  for (int i = 0; i < W; ++i) {
    p ^= b & ((T)0 - ((a >> (W - 1 - i)) & 1));
    b = (b >> 1) ^ (poly & ((T)0 - (b & 1)));
  }
  return p;
}
// x^(8 * bytes)
template <class T>
ZC_XZ_FN T gf_x8n(uint64_t bytes, T poly) {
  const int W = (int)sizeof(T) * 8;
  T r = (T)1 << (W - 1), base = (T)1 << (W - 9);  // x^0, x^8
  for (int i = 0; i < 64; ++i) {
    if ((bytes >> i) & 1) r = gf_mul(r, base, poly);
    base = gf_mul(base, base, poly);
  }
  return r;
}
// the finished CRC of A B from the finished CRCs of A and of B and B's length
ZC_XZ_FN uint32_t crc32_combine(uint32_t a, uint32_t b, uint64_t len_b) {
  return gf_mul(gf_x8n<uint32_t>(len_b, kPoly32), a, kPoly32) ^ b;
}
ZC_XZ_FN uint64_t crc64_combine(uint64_t a, uint64_t b, uint64_t len_b) {
  return gf_mul(gf_x8n<uint64_t>(len_b, kPoly64), a, kPoly64) ^ b;
}
// the finished CRC of n bytes from their raw CRC (start 0, no final inversion):
// the start value ~0 rides through n bytes, then the final inversion
ZC_XZ_FN uint32_t crc32_finish_raw(uint32_t raw, uint64_t n) {
  return raw ^ gf_mul(gf_x8n<uint32_t>(n, kPoly32), 0xffffffffu, kPoly32) ^ 0xffffffffu;
}
ZC_XZ_FN uint64_t crc64_finish_raw(uint64_t raw, uint64_t n) {
  return raw ^ gf_mul(gf_x8n<uint64_t>(n, kPoly64), (uint64_t)~0ull, kPoly64) ^ (uint64_t)~0ull;
}

// finished CRC-32 of in[off, off + n)
template <class In>
ZC_XZ_FN uint32_t crc32_of(const In& in, uint64_t off, uint64_t n) {
  uint32_t c = 0xffffffffu;
  for (uint64_t k = 0; k < n; ++k) c = crc32_byte(c, in.byte(off + k));
  return ~c;
}
template <class In>
ZC_XZ_FN uint64_t crc64_of(const In& in, uint64_t off, uint64_t n) {
  uint64_t c = ~0ull;
  for (uint64_t k = 0; k < n; ++k) c = crc64_byte(c, in.byte(off + k));
  return ~c;
}
// the check of n decoded bytes under a stream's check id (0 for kCheckNone)
template <class In>
ZC_XZ_FN uint64_t check_of(const In& payload, uint64_t n, uint32_t check_id) {
  if (check_id == kCheckCrc32) return crc32_of(payload, 0, n);
  if (check_id == kCheckCrc64) return crc64_of(payload, 0, n);
  return 0;
}
ZC_XZ_FN uint32_t check_size(uint32_t id) { return id == kCheckCrc32 ? 4 : id == kCheckCrc64 ? 8 : 0; }

template <class In>
ZC_XZ_FN uint32_t le32(const In& in, uint64_t off) {
  return in.byte(off) | in.byte(off + 1) << 8 | in.byte(off + 2) << 16 | in.byte(off + 3) << 24;
}

// A variable-length integer at in[*pos, end): 1..9 bytes of 7 bits, no zero
// byte after the first.  0: read; else kInput (the field ends at `end` = in_size)
// or `bad`.
template <class In>
ZC_XZ_FN int vli(const In& in, uint64_t* pos, uint64_t end, bool end_is_input, int bad, uint64_t* v) {
  uint64_t r = 0;
  int rc = bad;  // nine bytes without an end
  bool done = false;
  for (int k = 0; k < 9 && !done; ++k) {
    if (*pos >= end) {
      rc = end_is_input ? kInput : bad;
      done = true;
    } else {
      const uint32_t b = in.byte((*pos)++);
      r |= (uint64_t)(b & 0x7f) << (7 * k);
      if (b == 0 && k > 0) {
        done = true;
      } else if (!(b & 0x80)) {
        rc = kOk;
        done = true;
      }
    }
  }
  *v = r;
  return rc;
}

// the dictionary size of an LZMA2 property byte (<= 40)
ZC_XZ_FN uint32_t dict_size_of(uint32_t prop) {
  if (prop == 40) return 0xffffffffu;
  return (2u | (prop & 1)) << (prop / 2 + 11);
}

// FD 37 7A 58 5A 00
ZC_XZ_FN uint32_t magic_byte(uint32_t k) { return (uint32_t)(0x005A587A37FDull >> (8 * k)) & 0xff; }

// ---- the range decoder and the LZMA state ----

template <class In, class Probs>
struct Lzma {
  const In* in;
  Probs* probs;
  uint64_t ip, ilim;  // the chunk's compressed bytes are in[.., ilim)
  uint32_t range, code;
  uint32_t state, rep0, rep1, rep2, rep3;
  uint32_t lc, lclp, lp_mask, pos_mask;
  bool over;  // a read past ilim: the chunk is bad

  ZC_XZ_FN uint32_t next_byte() {
    if (ip >= ilim) {
      over = true;
      return 0;
    }
    return in->byte(ip++);
  }
  ZC_XZ_FN void normalize() {
    if (range < (1u << 24)) {
      range <<= 8;
      code = (code << 8) | next_byte();
    }
  }
  ZC_XZ_FN uint32_t bit(uint32_t i) {
    normalize();
    const uint32_t p = probs->ld(i);
    const uint32_t bound = (range >> 11) * p;
    uint32_t b;
    if (code < bound) {
      range = bound;
      probs->st(i, p + ((2048 - p) >> 5));
      b = 0;
    } else {
      range -= bound;
      code -= bound;
      probs->st(i, p - (p >> 5));
      b = 1;
    }
    return b;
  }
  // `bits` bits down a tree rooted at base: the value, 0 .. 2^bits - 1
  ZC_XZ_FN uint32_t tree(uint32_t base, uint32_t bits) {
    uint32_t s = 1;
    for (uint32_t k = 0; k < bits; ++k) s = (s << 1) | bit(base + s);
    return s - (1u << bits);
  }
  ZC_XZ_FN uint32_t tree_reverse(uint32_t base, uint32_t bits) {
    uint32_t s = 1, v = 0;
    for (uint32_t k = 0; k < bits; ++k) {
      const uint32_t b = bit(base + s);
      s = (s << 1) | b;
      v |= b << k;
    }
    return v;
  }
  ZC_XZ_FN uint32_t direct(uint32_t bits) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < bits; ++k) {
      normalize();
      range >>= 1;
      code -= range;
      const uint32_t mask = 0u - (code >> 31);
      code += range & mask;
      v = (v << 1) + (mask + 1);
    }
    return v;
  }
  ZC_XZ_FN uint32_t length(uint32_t base, uint32_t pos_state) {
    uint32_t len;
    if (!bit(base + kLenChoice)) {
      len = 2 + tree(base + kLenLow + pos_state * 8, 3);
    } else if (!bit(base + kLenChoice2)) {
      len = 2 + 8 + tree(base + kLenMid + pos_state * 8, 3);
    } else {
      len = 2 + 16 + tree(base + kLenHigh, 8);
    }
    return len;
  }
  ZC_XZ_FN void reset_state() {
    state = 0;
    rep0 = rep1 = rep2 = rep3 = 0;
  }
};

// ---- the walk ----

// Decodes the stream in[0, in_size) for an output of at most cap bytes.
template <class In, class Probs, class Out>
ZC_XZ_FN Result decode(const In& in, const uint64_t in_size, const uint64_t cap, Probs& probs, Out& out) {
  Result r{kOk, 0, 0, 0, 0};
  // ---- stream header: FD 37 7A 58 5A 00, two flag bytes, CRC32 ----
  for (uint32_t k = 0; k < 6 && r.status == kOk; ++k) {
    if (k >= in_size)
      r.status = kInput;
    else if (in.byte(k) != magic_byte(k))
      r.status = kFormat;
  }
  if (r.status != kOk) return r;
  if (in_size < 12) {
    r.status = kInput;
    return r;
  }
  const uint32_t flag0 = in.byte(6), flag1 = in.byte(7);
  if (crc32_of(in, 6, 2) != le32(in, 8)) {
    r.status = kHeader;
    return r;
  }
  r.check_id = flag1 & 15;
  if (flag0 != 0 || (flag1 & 0xf0) ||
      !(r.check_id == kCheckNone || r.check_id == kCheckCrc32 || r.check_id == kCheckCrc64)) {
    r.status = kUnsupported;
    return r;
  }
  uint64_t pos = 12;
  // ---- zero or one block ----
  if (pos >= in_size) {
    r.status = kInput;
    return r;
  }
  bool have_block = false;
  uint64_t unpadded = 0;  // the block's, for the index
  uint64_t op = 0;        // bytes written
  const uint32_t hsz = in.byte(pos);
  if (hsz != 0) {
    have_block = true;
    const uint64_t hstart = pos, hbytes = ((uint64_t)hsz + 1) * 4, hend = hstart + hbytes - 4;
    if (hstart + hbytes > in_size) {
      r.status = kInput;
      return r;
    }
    if (crc32_of(in, hstart, hbytes - 4) != le32(in, hend)) {
      r.status = kHeader;
      return r;
    }
    const uint32_t bflags = in.byte(hstart + 1);
    if (bflags & 0x3c) {
      r.status = kUnsupported;  // reserved bits
      return r;
    }
    if (bflags & 3) {
      r.status = kUnsupported;  // more than one filter
      return r;
    }
    uint64_t hp = hstart + 2;
    uint64_t want_csize = ~0ull, want_usize = ~0ull;
    int rc = kOk;
    if (bflags & 0x40) {
      rc = vli(in, &hp, hend, false, kHeader, &want_csize);
      if (rc == kOk && want_csize == 0) rc = kHeader;
    }
    if (rc == kOk && (bflags & 0x80)) rc = vli(in, &hp, hend, false, kHeader, &want_usize);
    uint64_t fid = 0, fprops = 0;
    if (rc == kOk) rc = vli(in, &hp, hend, false, kHeader, &fid);
    if (rc == kOk) rc = vli(in, &hp, hend, false, kHeader, &fprops);
    if (rc == kOk && fid != 0x21) rc = kUnsupported;
    if (rc == kOk && fprops != 1) rc = kUnsupported;
    if (rc == kOk && hp >= hend) rc = kHeader;
    uint32_t dprop = 0;
    if (rc == kOk) {
      dprop = in.byte(hp++);
      if (dprop > 40) rc = kUnsupported;
    }
    for (uint64_t k = hp; k < hend && rc == kOk; ++k)  // fewer than 1,024 bytes
      if (in.byte(k) != 0) rc = kUnsupported;          // header padding
    if (rc != kOk) {
      r.status = rc;
      return r;
    }
    const uint32_t dict_size = dict_size_of(dprop);
    pos = hstart + hbytes;
    const uint64_t data_start = pos;

    // ---- LZMA2 ----
    Lzma<In, Probs> z;
    z.in = &in;
    z.probs = &probs;
    z.ip = z.ilim = pos;
    z.range = 0xffffffffu;
    z.code = 0;
    z.lc = z.lclp = 0;
    z.lp_mask = z.pos_mask = 0;
    z.over = false;
    z.reset_state();
    bool need_dict_reset = true, need_props = true;
    bool in_chunk = false;   // an LZMA chunk is open
    uint64_t chunk_end = 0;  // the open chunk's uncompressed bytes end at this op
    uint64_t dict_start = 0; // op at the last dictionary reset
    uint32_t prev = 0;       // out[op - 1] when prev_known
    bool prev_known = true;
    int st = kBudget;
    uint64_t budget = cap + in_size + 64;
    if (budget < cap) budget = ~0ull;
    for (; budget > 0 && st == kBudget; --budget) {
      if (!in_chunk) {
        // ---- a chunk header, or the end ----
        if (pos >= in_size) {
          st = kInput;
          continue;
        }
        const uint32_t ctl = in.byte(pos++);
        if (ctl == 0) {
          st = kOk;
          continue;
        }
        if (ctl > 2 && ctl < 0x80) {
          st = kData;
          continue;
        }
        if (ctl >= 0xE0 || ctl == 1) {
          need_props = true;
          need_dict_reset = false;
          dict_start = op;
          prev = 0;
          prev_known = true;
        } else if (need_dict_reset) {
          st = kData;
          continue;
        }
        if (ctl < 0x80) {
          // a stored chunk: 16-bit size - 1, the bytes
          if (in_size - pos < 2) {
            st = kInput;
            continue;
          }
          const uint64_t n = ((uint64_t)in.byte(pos) << 8 | in.byte(pos + 1)) + 1;
          pos += 2;
          if (in_size - pos < n) {
            st = kInput;
            continue;
          }
          if (cap - op < n) {
            st = kOutput;
            continue;
          }
          out.stored(pos, op, (uint32_t)n);
          pos += n;
          op += n;
          prev_known = false;
          continue;
        }
        // an LZMA chunk: sizes - 1 (21 and 16 bits), properties when ctl >= 0xC0
        if (in_size - pos < 4) {
          st = kInput;
          continue;
        }
        const uint64_t usize = ((uint64_t)(ctl & 0x1f) << 16 | (uint64_t)in.byte(pos) << 8 | in.byte(pos + 1)) + 1;
        const uint64_t csize = ((uint64_t)in.byte(pos + 2) << 8 | in.byte(pos + 3)) + 1;
        pos += 4;
        if (ctl >= 0xC0) {
          if (pos >= in_size) {
            st = kInput;
            continue;
          }
          uint32_t d = in.byte(pos++);
          if (d > 224) {
            st = kData;
            continue;
          }
          const uint32_t lc = d % 9;
          d /= 9;
          const uint32_t lp = d % 5, pb = d / 5;
          if (lc + lp > 4) {
            st = kData;
            continue;
          }
          if (prob_count(lc + lp) > probs.cap()) {
            st = kNeedWide;
            continue;
          }
          z.lc = lc;
          z.lclp = lc + lp;
          z.lp_mask = (1u << lp) - 1;
          z.pos_mask = (1u << pb) - 1;
          need_props = false;
        } else if (need_props) {
          st = kData;
          continue;
        }
        if (ctl >= 0xA0) {
          z.reset_state();
          probs.fill(prob_count(z.lclp));
        }
        if (in_size - pos < csize) {
          st = kInput;
          continue;
        }
        if (csize < 5) {
          st = kData;
          continue;
        }
        // the range decoder's five bytes: the first is 0, as the encoder writes it
        if (in.byte(pos) != 0) {
          st = kData;
          continue;
        }
        z.ip = pos;
        z.ilim = pos + csize;
        z.range = 0xffffffffu;
        z.code = 0;
        for (int k = 0; k < 5; ++k) z.code = (z.code << 8) | z.next_byte();
        chunk_end = op + usize;  // op <= cap, usize <= 2^21
        in_chunk = true;
        continue;
      }
      // ---- one symbol ----
      const uint64_t dpos = op - dict_start;
      const uint32_t pos_state = (uint32_t)dpos & z.pos_mask;
      uint32_t len = 0;  // 0: a literal
      uint32_t lit = 0;
      bool bad = false;
      if (!z.bit(kIsMatch + z.state * kPosStatesMax + pos_state)) {
        if (!prev_known) {
          prev = out.get(op - 1);  // op > dict_start: only a match or a stored chunk clears prev_known
          prev_known = true;
        }
        const uint32_t base = kLiteral + 0x300u * ((((uint32_t)dpos & z.lp_mask) << z.lc) + (prev >> (8 - z.lc)));
        uint32_t s = 1;
        if (z.state < 7) {
          for (int k = 0; k < 8; ++k) s = (s << 1) | z.bit(base + s);
        } else {
          // after a match: the byte at the last distance steers the tree.  A
          // match state means a match was copied since the last reset of state
          // and dictionary, so rep0 < dpos.
          uint32_t mb = z.rep0 < dpos ? out.get(op - z.rep0 - 1) : 0;
          if (z.rep0 >= dpos) bad = true;
          uint32_t offset = 0x100;
          for (int k = 0; k < 8; ++k) {
            mb <<= 1;
            const uint32_t mbit = mb & offset;
            const uint32_t b = z.bit(base + offset + mbit + s);
            s = (s << 1) | b;
            offset &= b ? mbit : ~mbit;
          }
        }
        lit = s & 0xff;
        z.state = z.state < 4 ? 0 : z.state < 10 ? z.state - 3 : z.state - 6;
      } else if (!z.bit(kIsRep + z.state)) {
        // a match with a new distance
        len = z.length(kMatchLen, pos_state);
        const uint32_t slot = z.tree(kDistSlot + (len < 6 ? len - 2 : 3) * 64, 6);
        uint32_t d;
        if (slot < 4) {
          d = slot;
        } else {
          const uint32_t nb = (slot >> 1) - 1;
          d = 2 | (slot & 1);
          if (slot < 14) {
            d <<= nb;
            d += z.tree_reverse(kDistSpecial + d - slot - 1, nb);
          } else {
            d = (d << (nb - 4)) + z.direct(nb - 4);
            d <<= 4;
            d += z.tree_reverse(kDistAlign, 4);
          }
        }
        z.rep3 = z.rep2;
        z.rep2 = z.rep1;
        z.rep1 = z.rep0;
        z.rep0 = d;
        z.state = z.state < 7 ? 7 : 10;
      } else {
        if (!z.bit(kIsRep0 + z.state)) {
          if (!z.bit(kIsRep0Long + z.state * kPosStatesMax + pos_state)) {
            len = 1;  // a short rep
            z.state = z.state < 7 ? 9 : 11;
          }
        } else {
          uint32_t d;
          if (!z.bit(kIsRep1 + z.state)) {
            d = z.rep1;
          } else {
            if (!z.bit(kIsRep2 + z.state)) {
              d = z.rep2;
            } else {
              d = z.rep3;
              z.rep3 = z.rep2;
            }
            z.rep2 = z.rep1;
          }
          z.rep1 = z.rep0;
          z.rep0 = d;
        }
        if (len == 0) {
          len = z.length(kRepLen, pos_state);
          z.state = z.state < 7 ? 8 : 11;
        }
      }
      // ---- the symbol is read: validate, then write ----
      if (z.over || bad) {
        st = kData;
        continue;
      }
      if (len == 0) {
        if (op >= cap) {  // op < chunk_end inside a chunk
          st = kOutput;
          continue;
        }
        out.lit(op, lit);
        prev = lit;
        op += 1;
      } else {
        // the distance (rep0 + 1) reaches neither past the bytes since the last
        // dictionary reset nor past the dictionary; 0xffffffff is the end
        // marker, which LZMA2 does not have
        if ((uint64_t)z.rep0 >= dpos || z.rep0 >= dict_size) {
          st = kData;
          continue;
        }
        if (chunk_end - op < len) {
          st = kData;
          continue;
        }
        if (cap - op < len) {
          st = kOutput;
          continue;
        }
        out.copy(op, z.rep0 + 1, len);
        op += len;
        prev_known = false;
      }
      if (op == chunk_end) {
        // the chunk ends exactly here: its compressed bytes used, the coder at rest
        z.normalize();
        if (z.over || z.ip != z.ilim || z.code != 0) {
          st = kData;
          continue;
        }
        pos = z.ilim;
        in_chunk = false;
      }
    }
    r.decoded = op;
    if (st != kOk) {
      r.status = st;
      return r;
    }
    // ---- block padding, check ----
    const uint64_t csize = pos - data_start;
    if ((want_csize != ~0ull && want_csize != csize) || (want_usize != ~0ull && want_usize != op)) {
      r.status = kHeader;
      return r;
    }
    for (uint32_t k = 0; k < 3 && (pos - data_start) % 4 != 0; ++k) {
      if (pos >= in_size) {
        r.status = kInput;
        return r;
      }
      if (in.byte(pos++) != 0) {
        r.status = kData;
        return r;
      }
    }
    const uint32_t csz = check_size(r.check_id);
    if (in_size - pos < csz) {
      r.status = kInput;
      return r;
    }
    for (uint32_t k = 0; k < csz; ++k) r.stored |= (uint64_t)in.byte(pos + k) << (8 * k);
    pos += csz;
    unpadded = hbytes + csize + csz;
    if (pos >= in_size) {
      r.status = kInput;
      return r;
    }
    if (in.byte(pos) != 0) {
      r.status = kUnsupported;  // another block
      return r;
    }
  }
  // ---- index: 00, the record count, the records, padding, CRC32 ----
  const uint64_t xstart = pos;
  pos += 1;
  uint64_t nrec = 0, v_unpadded = 0, v_usize = 0;
  int rc = vli(in, &pos, in_size, true, kHeader, &nrec);
  if (rc == kOk && nrec != (have_block ? 1u : 0u)) rc = kHeader;
  if (rc == kOk && have_block) {
    rc = vli(in, &pos, in_size, true, kHeader, &v_unpadded);
    if (rc == kOk) rc = vli(in, &pos, in_size, true, kHeader, &v_usize);
    if (rc == kOk && (v_unpadded != unpadded || v_usize != r.decoded)) rc = kHeader;
  }
  for (uint32_t k = 0; k < 3 && rc == kOk && (pos - xstart) % 4 != 0; ++k) {
    if (pos >= in_size)
      rc = kInput;
    else if (in.byte(pos++) != 0)
      rc = kHeader;
  }
  if (rc == kOk && in_size - pos < 4) rc = kInput;
  if (rc == kOk && crc32_of(in, xstart, pos - xstart) != le32(in, pos)) rc = kHeader;
  if (rc != kOk) {
    r.status = rc;
    return r;
  }
  pos += 4;
  const uint64_t xbytes = pos - xstart;
  // ---- stream footer: CRC32, backward size, flags, 'Y' 'Z' ----
  if (in_size - pos < 12) {
    r.status = kInput;
    return r;
  }
  if (crc32_of(in, pos + 4, 6) != le32(in, pos) || in.byte(pos + 10) != 0x59 || in.byte(pos + 11) != 0x5A ||
      ((uint64_t)le32(in, pos + 4) + 1) * 4 != xbytes || in.byte(pos + 8) != flag0 || in.byte(pos + 9) != flag1) {
    r.status = kHeader;
    return r;
  }
  pos += 12;
  r.consumed = pos;
  // ---- stream padding with a second stream behind it ----
  uint64_t q = pos;
  uint64_t look = in_size - pos;  // the zeros are skipped within the walk's own bound
  for (; look > 0 && q < in_size && in.byte(q) == 0; --look) ++q;
  if (in_size - q >= 6) {
    bool again = true;
    for (uint32_t k = 0; k < 6; ++k) again = again && in.byte(q + k) == magic_byte(k);
    if (again) r.status = kUnsupported;
  }
  return r;
}

}  // namespace zcxz
