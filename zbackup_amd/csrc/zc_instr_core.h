// zc_instr_core.h -- a BackupInstruction stream parsed without walking it
// message by message: the definitions zc_instr.hip's kernels and the CPU check
// (tests/instr/instr_core_check.cpp) share.  What is parsed is
// zc_parse_instructions (zc_engine.cpp), restated: Message::parse per
// instruction (message.cc:24-42: a varint32 length, then the fields of
// BackupInstruction, zbackup.proto:149-159), entries in the order restore()
// acts on them (backup_restorer.cc:59-88: the chunk first, then the bytes).
//
//   hop    hop_at(p): where the message would end if one started at p -- the
//          position behind its length varint plus the length -- or kBad when
//          the varint is truncated or overlong or the length runs past the
//          end.  p < hop_at(p) <= n: a varint takes a byte at least.
//   exit   per tile of T positions, T a power of two: exit[p] = the first
//          position at or beyond the tile's end on p's chain of hops, or kBad.
//          Pointer doubling over the tile (tile_exits): log2 T rounds, after
//          round k a value has taken 2^k hops or left the tile; a chain inside
//          a tile has at most T hops.
//   chain  from 0, entry[tile of p] = p, p = exit[p]: the tile index grows with
//          every step, so at most `tiles` steps (chain_walk).  A tile no step
//          lands in lies inside one message and keeps kNone.
//   emit   per tile with an entry: the true messages from the entry to the
//          tile's end, parsed (tile_walk): once to count entries, messages and
//          the BYTES sizes and to find the tile's first error, once more to
//          write the records at the tile's place in the output.
//
// Only positions the chain reaches are message starts: a payload's bytes are
// hopped over like any others, and nothing they spell is parsed as a message.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcin {

constexpr uint32_t kBad = 0xffffffffu;   // a hop or an exit that is no position
constexpr uint32_t kNone = 0xffffffffu;  // a tile without a message start
constexpr uint64_t kSizeLimit = 0xffffffffull;  // streams stay below 2^32 - 1 bytes: positions and kBad differ
constexpr uint32_t kTileDefault = 8192;  // two 4-byte LDS buffers of T positions: 64 KiB
constexpr uint32_t kTileMin = 64;

// the host parser's failures, in its words (zc_parse_instructions)
enum Err : uint32_t {
  kOk = 0,
  kErrLenVarint,    // at the message's start
  kErrLenPastEnd,   // at the message's start
  kErrField,        // the rest: at the field's tag byte
  kErrFieldVarint,
  kErrFieldPastEnd,
  kErrChunkSize,
  kErrChunkTwice,
  kErrBytesTwice,
  kErrCount
};
inline const char* err_text(uint32_t e) {
  static const char* const t[kErrCount] = {"",
                                           "truncated or overlong length varint",
                                           "instruction length past the end of the stream",
                                           "a field other than chunk_to_emit / bytes_to_emit",
                                           "truncated field length",
                                           "field past the end of its instruction",
                                           "chunk_to_emit is not a 24-byte chunk id",
                                           "chunk_to_emit twice in one instruction",
                                           "bytes_to_emit twice in one instruction"};
  return e < kErrCount ? t[e] : "";
}

// an error as one word, so that the smallest is the first in the stream
constexpr uint64_t kNoError = ~0ull;
ZC_HD inline uint64_t err_key(uint64_t at, uint32_t e) { return at << 8 | e; }

// a varint of at most 32 bits' worth of 7-bit groups inside [*pos, end); five bytes at the most
ZC_HD inline bool varint(const uint8_t* d, uint64_t* pos, uint64_t end, uint64_t* v) {
  *v = 0;
  for (int k = 0; k < 5; k++) {
    if (*pos >= end) return false;
    const uint8_t b = d[(*pos)++];
    *v |= (uint64_t)(b & 0x7f) << (7 * k);
    if (!(b & 0x80)) return *v <= 0xffffffffull;
  }
  return false;
}

// the frame of a message at p < n: its body [*body, *end), or the length error
ZC_HD inline uint32_t frame_at(const uint8_t* d, uint64_t n, uint64_t p, uint64_t* body, uint64_t* end) {
  uint64_t pos = p, len;
  if (!varint(d, &pos, n, &len)) return kErrLenVarint;
  if (len > n - pos) return kErrLenPastEnd;
  *body = pos;
  *end = pos + len;
  return kOk;
}

ZC_HD inline uint32_t hop_at(const uint8_t* d, uint64_t n, uint64_t p) {
  uint64_t body, end;
  if (frame_at(d, n, p, &body, &end) != kOk) return kBad;
  return (uint32_t)end;  // p < body <= end <= n < 2^32 - 1
}

// One tile's exits by pointer doubling.  a: hop[base + i] for i < cnt (cnt <= T
// positions, the tile [base, base + cnt)); b: room for cnt more.  A value below
// base + cnt is a position of the tile, any other (kBad too) is final.
// `rounds` = log2 T.  Returns the buffer that holds the exits.  Single-threaded
// form of zc_in_exits' rounds, for the CPU check.
inline uint32_t* tile_exits(uint32_t* a, uint32_t* b, uint32_t base, uint32_t cnt, uint32_t rounds) {
  const uint32_t end = base + cnt;
  for (uint32_t r = 0; r < rounds; r++) {  // bound: rounds
    for (uint32_t i = 0; i < cnt; i++) b[i] = a[i] < end ? a[a[i] - base] : a[i];
    uint32_t* t = a;
    a = b;
    b = t;
  }
  return a;
}

// what a tile's walk adds up
struct TileSum {
  uint32_t entries, messages;
  uint64_t bytes;  // the BYTES entries' sizes
  uint64_t error;  // err_key of the tile's first error, or kNoError
};

// The true messages that start in [p, tile_end), p the tile's entry.  out: NULL
// counts; else the 48-byte records (twelve 32-bit words each) are written from
// out on.  The walk ends at the tile's first error.
// Bounds: the outer loop runs once per message start, each at least a byte
// behind the last, so at most tile_end - p times; the field loop runs at most
// three times, since a third field repeats a tag and is an error.
ZC_HD inline TileSum tile_walk(const uint8_t* d, uint64_t n, uint64_t p, uint64_t tile_end, uint32_t* out) {
  TileSum s{0, 0, 0, kNoError};
  while (p < tile_end) {
    uint64_t pos, end;
    const uint32_t fe = frame_at(d, n, p, &pos, &end);
    if (fe != kOk) {
      s.error = err_key(p, fe);
      return s;
    }
    bool has_chunk = false, has_bytes = false;
    uint64_t id_at = 0, data_off = 0, size = 0;
    while (pos < end) {
      const uint64_t fat = pos;
      const uint8_t tag = d[pos++];
      uint32_t e = kOk;
      uint64_t flen = 0;
      if (tag != 0x0a && tag != 0x12)
        e = kErrField;
      else if (!varint(d, &pos, end, &flen))
        e = kErrFieldVarint;
      else if (flen > end - pos)
        e = kErrFieldPastEnd;
      else if (tag == 0x0a)
        e = flen != 24 ? kErrChunkSize : has_chunk ? kErrChunkTwice : kOk;
      else
        e = has_bytes ? kErrBytesTwice : kOk;
      if (e != kOk) {
        s.error = err_key(fat, e);
        return s;
      }
      if (tag == 0x0a) {
        has_chunk = true;
        id_at = pos;
      } else {
        has_bytes = true;
        data_off = pos;
        size = flen;
      }
      pos += flen;
    }
    if (out) {
      if (has_chunk) {
        out[0] = 0;  // ZC_INSTR_CHUNK
        for (int k = 0; k < 6; k++) {
          const uint8_t* q = d + id_at + 4 * k;
          out[1 + k] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        for (int k = 7; k < 12; k++) out[k] = 0;
        out += 12;
      }
      if (has_bytes) {
        out[0] = 1;  // ZC_INSTR_BYTES
        for (int k = 1; k < 8; k++) out[k] = 0;
        out[8] = (uint32_t)data_off;
        out[9] = (uint32_t)(data_off >> 32);
        out[10] = (uint32_t)size;
        out[11] = (uint32_t)(size >> 32);
        out += 12;
      }
    }
    s.entries += (has_chunk ? 1u : 0u) + (has_bytes ? 1u : 0u);
    s.messages++;
    if (has_bytes) s.bytes += size;
    p = end;
  }
  return s;
}

// the tile a test asked for: a power of two from kTileMin up, no larger than
// the default; anything else gives the default
inline uint32_t tile_for(const char* env) {
  if (!env || !*env) return kTileDefault;
  uint64_t v = 0;
  for (const char* c = env; *c; c++) {
    if (*c < '0' || *c > '9' || v > kTileDefault) return kTileDefault;
    v = v * 10 + (uint64_t)(*c - '0');
  }
  if (v < kTileMin || v > kTileDefault || (v & (v - 1))) return kTileDefault;
  return (uint32_t)v;
}
inline uint32_t log2_of(uint32_t t) {
  uint32_t r = 0;
  while ((1u << r) < t) r++;
  return r;
}

}  // namespace zcin
