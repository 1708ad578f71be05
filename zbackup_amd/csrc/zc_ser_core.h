// zc_ser_core.h -- records to their BackupInstruction stream, the definitions
// zc_ser.hip's kernels, zc_serialized_size and the CPU check
// (tests/ser/ser_core_check.cpp) share.  What is written is
// zc_serialize_records (zc_engine.cpp), restated: Message::serialize per record
// (message.cc:16-23), one message each --
//
//   varint(body)  tag  varint(field)  bytes
//
// with tag 0x12 and the stream's bytes [offset, offset + size) when the record's
// kind is ZC_BYTES (field = size), and tag 0x0a and the 24-byte chunk id --
// sha1[16], then rolling little-endian -- for every other kind value
// (field = 24); body = 1 + the field's varint + field.
//
// A message's length is a pure function of (kind, size), so the position of
// every message is an exclusive scan of the lengths.  What stands before a
// payload -- the header -- is at most kHeaderMax bytes; a chunk's whole message
// is kChunkMessage bytes.
//
// The device writes a group of kGroup consecutive records per wave.  A record
// whose payload is longer than kStage is `big`: its header is staged with the
// messages around it, its payload copied apart in pieces of kPiece bytes.  The
// big records cut the group into runs (run_last): a run is a maximal range of
// lanes whose staged bytes -- whole messages, and the header of the big record
// that ends the run -- are contiguous in the output.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcser {

constexpr uint32_t kKindBytes = 2;    // ZC_BYTES
constexpr uint32_t kChunkId = 24;     // ChunkId::toBlob
constexpr uint32_t kChunkMessage = 27;
constexpr uint32_t kHeaderMax = 11;   // two varints of five bytes at the most, and the tag
constexpr uint32_t kStage = 128;      // the longest payload assembled in LDS
constexpr uint32_t kStagedMax = 133;  // the longest staged message: 2 + 1 + 2 + kStage
constexpr uint32_t kGroup = 64;
constexpr uint32_t kRunMax = kGroup * kStagedMax;  // the most staged bytes of a run
constexpr uint64_t kPiece = 64 * 1024;             // zclzo::kPiece, the other copies' piece
static_assert(kStage >= 127, "every bytes_to_emit the engine emits is staged (backup_creator.cc:114)");
static_assert(kStagedMax >= kChunkMessage && kStagedMax >= kHeaderMax, "a run's bound covers chunks and headers");

// a record as the kernels and the host read it: zc_record's fields, sha1 as four little-endian words
struct Rec {
  uint64_t offset;
  uint32_t size, kind;
  uint64_t rolling;
  uint32_t sha[4];
};

// bound: ten 7-bit groups hold 64 bits
ZC_HD inline uint32_t varint_len(uint64_t v) {
  uint32_t k = 1;
  for (; k < 10 && v >= 0x80; k++) v >>= 7;
  return k;
}
ZC_HD inline uint32_t put_varint(uint8_t* p, uint64_t v) {
  uint32_t k = 0;
  for (; k < 9 && v >= 0x80; k++) {
    p[k] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  p[k] = (uint8_t)v;
  return k + 1;
}

ZC_HD inline uint64_t field_len(uint32_t kind, uint32_t size) { return kind == kKindBytes ? size : kChunkId; }
ZC_HD inline uint64_t body_len(uint32_t kind, uint32_t size) {
  const uint64_t f = field_len(kind, size);
  return 1 + varint_len(f) + f;
}
// the bytes in front of the payload
ZC_HD inline uint32_t header_len(uint32_t kind, uint32_t size) {
  return varint_len(body_len(kind, size)) + 1 + varint_len(field_len(kind, size));
}
ZC_HD inline uint64_t message_len(uint32_t kind, uint32_t size) {
  const uint64_t b = body_len(kind, size);
  return varint_len(b) + b;
}
// the header at p (room: kHeaderMax); returns header_len
ZC_HD inline uint32_t put_header(uint8_t* p, uint32_t kind, uint32_t size) {
  uint32_t k = put_varint(p, body_len(kind, size));
  p[k++] = kind == kKindBytes ? 0x12 : 0x0a;
  return k + put_varint(p + k, field_len(kind, size));
}
// the chunk id at p (room: kChunkId)
ZC_HD inline void put_chunk_id(uint8_t* p, const Rec& r) {
  for (uint32_t k = 0; k < 16; k++) p[k] = (uint8_t)(r.sha[k >> 2] >> (8 * (k & 3)));
  for (uint32_t k = 0; k < 8; k++) p[16 + k] = (uint8_t)(r.rolling >> (8 * k));
}

ZC_HD inline bool is_big(uint32_t kind, uint32_t size) { return kind == kKindBytes && size > kStage; }
// the bytes of a record's message that are staged with its run
ZC_HD inline uint32_t staged_len(uint32_t kind, uint32_t size) {
  return is_big(kind, size) ? header_len(kind, size) : (uint32_t)message_len(kind, size);
}
// the copies of a big record's payload, none for any other
ZC_HD inline uint32_t pieces(uint32_t kind, uint32_t size) {
  return is_big(kind, size) ? (uint32_t)(((uint64_t)size + kPiece - 1) / kPiece) : 0;
}

// The run that starts at lane lo < cnt of a group of cnt <= kGroup records,
// bit l of big set when lane l's record is big: its last lane.  The next run
// starts behind it; a group has at most cnt runs.
ZC_HD inline uint32_t run_last(uint64_t big, uint32_t lo, uint32_t cnt) {
  const uint64_t m = big >> lo;  // lo < 64
  uint32_t hi = cnt - 1;
  if (m) {
    const uint32_t z = (uint32_t)__builtin_ctzll(m);
    if (lo + z < hi) hi = lo + z;
  }
  return hi;
}

}  // namespace zcser
