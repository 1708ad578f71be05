// LZO1X decoding for the restore path: the token walker and the framing rules,
// written for host and device alike (ZC_HD, as zc_lzo_core.h) so that a GPU
// bundle decompressor can run exactly what the CPU unit check
// (tests/lzo/unlzo_core_check.cpp, test infrastructure only) compares with
// liblzo2's own lzo1x_decompress_safe.  The library uses the framing rules on
// the host (zc_lzo_frame_info); the device decoder is not in this tree (DESIGN
// 4.7).
//
// What zbackup runs: Bundle::Reader::Reader (bundle.cc:179-214) feeds a bundle
// file's payload to the decoder of the bundle's compression method; for
// "lzo1x_1" that is LZO1X_1_Decoder::doProcessNoSize (compression.cc:472-490)
// = liblzo2 2.10's lzo1x_decompress_safe, under the framing of
// NoStreamAndUnknownSizeDecoder::doProcess (compression.cc:369-402).  The
// bundle is good exactly when the library returns LZO_E_OK and the decoded
// size equals the size in the frame (compression.cc:486,398).
//
// walk() is a token walker for the complete LZO1X format (whatever
// lzo1x_decompress_safe accepts, not only what lzo1x_1 emits: the M1 forms
// occur in lzo1x_999 output).  It never touches payload bytes: it reads
// control bytes through in.byte(i), only for i < csize, and hands fully
// validated operations to a sink:
//   sink.literal(src_off, dst_off, len)  out[dst_off + k] = in[src_off + k]
//   sink.match(dst_off, dist, len)       out[dst_off + k] = out[dst_off - dist + k]
//                                        in increasing k (dist < len replicates a
//                                        period: = out[dst_off - dist + k % dist],
//                                        so every source lies below dst_off)
//
// Validity of every emitted op: src_off + len <= csize, dst_off + len <= cap,
// 1 <= dist <= dst_off, len >= 1.  That is the whole memory-safety argument of
// a device decoder: its sink copies only what the walker proved in range.
//
// Termination: every iteration of every loop below (the main loop, the match
// loop, the zero-byte run loops) consumes at least one input byte, and ip <=
// csize is checked before each read (need_ip), so a walk ends within csize
// steps whatever the bytes are.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zclzo {

// liblzo2's codes (lzoconf.h), and the two of the framing
constexpr int kLzoOk = 0, kLzoInputOverrun = -4, kLzoOutputOverrun = -5, kLzoLookbehindOverrun = -6,
              kLzoInputNotConsumed = -8;
constexpr int kFrameBad = -100;   // fewer than 16 bytes, or 16 + csize > the bytes given
constexpr int kFrameSize = -101;  // the stream is fine, but its size is not the frame's
// the farthest any LZO1X match reaches back (M4: 0x4000 + 0x7fff)
constexpr uint32_t kMaxDistance = 0x4000 + 0x7fff;
constexpr uint32_t kDecFrame = 16;

// Walks the stream in[0, csize) for an output of at most cap bytes.  Returns
// the library's code; *produced = the bytes the emitted ops wrote (on an error:
// those before the failing token, for which no op is emitted).
template <class In, class Sink>
ZC_HD inline int walk(In& in, const uint32_t csize, const uint32_t cap, Sink& sink, uint32_t* produced) {
  uint32_t ip = 0, op = 0;
  uint64_t t;           // lengths accumulate 255 per zero byte: up to 255 * csize
  uint64_t lit;         // the literal run to copy
  uint32_t dist;
  uint64_t mlen;
  uint32_t trail;       // the low two bits of a match's second-to-last byte
  bool after_match;     // the literal run is a match's trailing one (1-3 bytes)
  int rc;
#define ZC_NEED_IP(x)                      \
  if ((uint64_t)(csize - ip) < (uint64_t)(x)) { \
    rc = kLzoInputOverrun;                 \
    goto done;                             \
  }
#define ZC_NEED_OP(x)                      \
  if ((uint64_t)(cap - op) < (uint64_t)(x)) {  \
    rc = kLzoOutputOverrun;                \
    goto done;                             \
  }
  ZC_NEED_IP(1);
  t = in.byte(0);
  if (t > 17) {
    ip = 1;
    t -= 17;
    if (t < 4) {
      trail = (uint32_t)t;
      goto match_next;
    }
    ZC_NEED_OP(t);
    ZC_NEED_IP(t + 3);
    lit = t;
    after_match = false;
    goto copy_literals;
  }
  for (;;) {
    ZC_NEED_IP(3);
    t = in.byte(ip++);
    if (t >= 16) goto match;
    if (t == 0) {
      while (in.byte(ip) == 0) {
        t += 255;
        ip++;
        ZC_NEED_IP(1);
      }
      t += 15 + in.byte(ip++);
    }
    ZC_NEED_OP(t + 3);
    ZC_NEED_IP(t + 6);
    lit = t + 3;
    after_match = false;
  copy_literals:
    // lit bytes and the token byte after them are in range (need_ip above)
    sink.literal(ip, op, (uint32_t)lit);
    ip += (uint32_t)lit;
    op += (uint32_t)lit;
    t = in.byte(ip++);
    if (!after_match && t < 16) {  // M1 after a literal run: 3 bytes from beyond the M2 range
      trail = (uint32_t)t & 3;
      dist = 1 + 0x800 + ((uint32_t)t >> 2) + (in.byte(ip++) << 2);
      mlen = 3;
      goto copy_match;
    }
  match:
    if (t >= 64) {  // M2
      trail = (uint32_t)t & 3;
      dist = 1 + (((uint32_t)t >> 2) & 7) + (in.byte(ip++) << 3);
      mlen = (t >> 5) + 1;
    } else if (t >= 16) {  // M3, M4
      const bool m4 = t < 32;
      dist = m4 ? ((uint32_t)t & 8) << 11 : 1;
      t &= m4 ? 7 : 31;
      if (t == 0) {
        while (in.byte(ip) == 0) {
          t += 255;
          ip++;
          ZC_NEED_IP(1);
        }
        t += (m4 ? 7 : 31) + in.byte(ip++);
      }
      ZC_NEED_IP(2);
      const uint32_t b0 = in.byte(ip), b1 = in.byte(ip + 1);
      ip += 2;
      dist += (b0 >> 2) + (b1 << 6);
      trail = b0 & 3;
      if (m4) {
        if (dist == 0) {  // the end marker
          rc = ip == csize ? kLzoOk : kLzoInputNotConsumed;
          goto done;
        }
        dist += 0x4000;
      }
      mlen = t + 2;
    } else {  // M1 after a match's trailing literals: 2 bytes
      trail = (uint32_t)t & 3;
      dist = 1 + ((uint32_t)t >> 2) + (in.byte(ip++) << 2);
      mlen = 2;
    }
  copy_match:
    if (dist > op) {
      rc = kLzoLookbehindOverrun;
      goto done;
    }
    ZC_NEED_OP(mlen);
    sink.match(op, dist, (uint32_t)mlen);
    op += (uint32_t)mlen;
    if (trail == 0) continue;
  match_next:
    ZC_NEED_OP(trail);
    ZC_NEED_IP(trail + 3);
    lit = trail;
    after_match = true;
    goto copy_literals;
  }
done:
#undef ZC_NEED_IP
#undef ZC_NEED_OP
  *produced = op;
  return rc;
}

// ---- the framing (NoStreamAndUnknownSizeDecoder::doProcess, compression.cc:369-402) ----
// LE32 decoded size at byte 0, LE32 compressed size at byte 8, the stream from
// byte 16; bytes after 16 + csize are unused input, not an error.
ZC_HD inline uint32_t ld_le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
ZC_HD inline int frame_read(const uint8_t* framed, uint64_t avail, uint32_t* n, uint32_t* csize) {
  if (avail < kDecFrame) return kFrameBad;
  *n = ld_le32(framed);
  *csize = ld_le32(framed + 8);
  if ((uint64_t)kDecFrame + *csize > avail) return kFrameBad;
  return kLzoOk;
}
// the walk's output bound: the decoder's buffer is the frame's size (compression.cc:383-388)
ZC_HD inline uint32_t frame_cap(uint32_t n, uint64_t out_cap) { return out_cap < n ? (uint32_t)out_cap : n; }
// the bundle's status from the walk's (compression.cc:486,398)
ZC_HD inline int frame_status(int rc, uint32_t produced, uint32_t n) {
  return rc != kLzoOk ? rc : produced == n ? kLzoOk : kFrameSize;
}

}  // namespace zclzo
