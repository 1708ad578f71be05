// The reader of an index file's plaintext, for host and device alike (ZC_HD,
// as zc_lzo_dec.h, zc_gc_core.h and zc_range_core.h): the varint reader, the
// frame walker that goes from one bundle's header to the next, and the record
// walker inside one BundleInfo.  The kernels of zc_index.hip and the CPU unit
// check (tests/index/index_core_check.cpp) run exactly this code.
//
// What zbackup runs: IndexFile::Reader (index_file.cc:44-76) over
// Message::parse (message.cc:24-42) and EncryptedFile::InputStream
// (encrypted_file.cc:130-209), driven by ChunkIndex::loadIndex
// (chunk_index.cc:26-79); the messages are zbackup.proto:107-145.
//
// The plaintext, in order:
//   [R: 16 random bytes, with a key only]
//   varint32 len, FileHeader{version = 1}                     02 08 01
//   pairs of  varint32 len, IndexBundleHeader{id: 24 bytes}   1A 0A 18 <24>
//             varint32 len, BundleInfo                        repeated 0A <len> ChunkRecord
//   varint32 0                                                the header without an id ends the list
//   the little-endian Adler-32 of every byte before it
//   [PKCS#7 padding of 1..16 bytes, with a key only]
// ChunkRecord = 0A 18 <24-byte id> and 10 <varint32 size>, in either order.
//
// Strictness.  libprotobuf skips fields it does not know, lets a later field
// replace an earlier one and reads tags as varints of any length.  This reader
// is narrower, as zc_parse_instructions is: a tag is the one byte the writer
// emits, every field appears at most once, nothing else is accepted.  Length
// and value varints may be padded (up to 5 bytes) as long as the value fits 32
// bits.
//
// Status.  A file's status is the first failure met reading it front to back;
// the padding comes first, since it fixes where the file ends, and the
// Adler-32 last, where the reference checks it.  kTruncated is kept for the
// file's own end: a frame's length varint or the message it announces running
// past it, or no room for the Adler-32.  Whatever goes wrong inside a
// message's announced bytes is kBadMessage (or the id / version codes).
//
// Termination.  Every loop below consumes at least one byte per trip and
// carries a trip bound computed from the byte count before it starts; there is
// no goto, and no loop ends on a data value alone.  The byte source `in` is
// only ever asked for byte(i) with i < n (the file's or the extent's end).
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcidx {

// the codes of ZC_INDEX_* (include/zchunk.h)
constexpr int kOk = 0, kBadSize = 1, kBadPadding = 2, kTruncated = 3, kBadVersion = 4, kBadMessage = 5,
              kBadBundleId = 6, kBadChunkId = 7, kBadAdler = 8;

constexpr uint32_t kIdBytes = 24;
constexpr uint32_t kMinBundleBytes = 28;  // a bundle takes at least this much of a file
constexpr uint32_t kMinRecordBytes = 30;  // a record takes at least this much of a BundleInfo
// how far into a record the body walker can look before it has decided: both
// fields with 5-byte varints (1 + 5 + 24, 1 + 5) and the tag of a third field
constexpr uint32_t kRecordLook = 37;
constexpr uint32_t kHopLook = 6;  // a record's tag and its length varint

// varint reader: what it met
constexpr int kVarOk = 0, kVarEnd = 1, kVarBad = 2;

// One varint32 at pos, never reading at or past `limit`.  kVarEnd: the bytes
// ran out; kVarBad: a sixth byte would be needed, or the value needs more than
// 32 bits.  pos moves past what was read.  At most 5 trips.
template <class In>
ZC_HD inline int read_varint32(const In& in, uint64_t& pos, uint64_t limit, uint32_t* v) {
  uint64_t x = 0;
  for (int k = 0; k < 5; ++k) {
    if (pos >= limit) return kVarEnd;
    const uint32_t b = in.byte(pos++);
    x |= (uint64_t)(b & 0x7f) << (7 * k);
    if (!(b & 0x80)) {
      if (x > 0xffffffffull) return kVarBad;
      *v = (uint32_t)x;
      return kVarOk;
    }
  }
  return kVarBad;
}

// ---- the frame walker ----

struct Frame {
  uint64_t pos;  // the next unread byte
  uint64_t end;  // the plaintext's end (the padding taken off)
};

// The length varint in front of a message, at the file's level: the message
// must lie inside [pos, end).
template <class In>
ZC_HD inline int frame_len(const In& in, Frame* f, uint32_t* len) {
  const int v = read_varint32(in, f->pos, f->end, len);
  if (v == kVarEnd) return kTruncated;
  if (v == kVarBad) return kBadMessage;
  if (*len > f->end - f->pos) return kTruncated;
  return kOk;
}

// Size, padding, R and FileHeader of a file of n bytes.  On kOk, f stands at
// the first IndexBundleHeader.
template <class In>
ZC_HD inline int frame_open(const In& in, uint64_t n, bool keyed, Frame* f) {
  f->pos = 0;
  f->end = n;
  if (n == 0 || (keyed && n % 16)) return kBadSize;
  if (keyed) {
    const uint32_t pad = in.byte(n - 1);
    bool ok = pad >= 1 && pad <= 16;
    for (uint32_t k = 0; k < 16; ++k)
      if (ok && k < pad && in.byte(n - 1 - k) != pad) ok = false;
    if (!ok) return kBadPadding;
    f->end = n - pad;
    if (f->end < 16) return kTruncated;  // R
    f->pos = 16;
  }
  uint32_t len;
  const int rc = frame_len(in, f, &len);
  if (rc != kOk) return rc;
  const uint64_t mend = f->pos + len;
  bool have = false;
  uint32_t version = 0;
  // every trip consumes the tag byte at least: len trips at most
  for (uint64_t trip = 0; trip < len && f->pos < mend; ++trip) {
    const uint32_t tag = in.byte(f->pos++);
    if (tag != 0x08 || have) return kBadMessage;
    if (read_varint32(in, f->pos, mend, &version) != kVarOk) return kBadMessage;
    have = true;
  }
  if (!have) return kBadMessage;
  if (version != 1) return kBadVersion;
  return kOk;
}

constexpr int kFrameBundle = -1, kFrameEnd = -2;

// The next IndexBundleHeader and, when it has an id, the BundleInfo after it.
// kFrameBundle: id_off / info_off / info_len are set and f stands behind the
// BundleInfo; kFrameEnd: the list ended and f->pos is where the stored
// Adler-32 lies (4 bytes, inside the plaintext); else a status.  Consumes at
// least one byte, and kMinBundleBytes on kFrameBundle.
template <class In>
ZC_HD inline int frame_next(const In& in, Frame* f, uint64_t* id_off, uint64_t* info_off, uint32_t* info_len) {
  uint32_t len;
  int rc = frame_len(in, f, &len);
  if (rc != kOk) return rc;
  if (len == 0) return f->end - f->pos < 4 ? kTruncated : kFrameEnd;
  const uint64_t mend = f->pos + len;
  if (in.byte(f->pos++) != 0x0A) return kBadMessage;
  uint32_t l;
  if (read_varint32(in, f->pos, mend, &l) != kVarOk) return kBadMessage;
  if (l > mend - f->pos) return kBadMessage;
  if (l != kIdBytes) return kBadBundleId;
  *id_off = f->pos;
  f->pos += kIdBytes;
  if (f->pos != mend) return kBadMessage;  // a second field: a repeat or a stranger
  rc = frame_len(in, f, info_len);
  if (rc != kOk) return rc;
  *info_off = f->pos;
  f->pos += *info_len;
  return kFrameBundle;
}

// the bundles a file of n bytes can hold, and the frame walker's trip bound
ZC_HD inline uint64_t max_bundles(uint64_t n) { return n / kMinBundleBytes; }
// the records bytes of BundleInfo can hold
ZC_HD inline uint64_t max_records(uint64_t bytes) { return bytes / kMinRecordBytes; }

// ---- the record walker ----

// A record's tag and length at pos (pos < end).  On kOk body / blen are its
// bytes and pos stands behind it.  Consumes at least two bytes.
template <class In>
ZC_HD inline int record_hop(const In& in, uint64_t& pos, uint64_t end, uint64_t* body, uint32_t* blen) {
  if (in.byte(pos++) != 0x0A) return kBadMessage;
  if (read_varint32(in, pos, end, blen) != kVarOk) return kBadMessage;
  if (*blen > end - pos) return kBadMessage;
  *body = pos;
  pos += *blen;
  return kOk;
}

// The two fields of the ChunkRecord in [pos, pos + blen).  Three trips at
// most: a third field is a repeat or a stranger whatever it is.  Looks at no
// byte beyond pos + kRecordLook.
template <class In>
ZC_HD inline int record_body(const In& in, uint64_t pos, uint32_t blen, uint64_t* id_off, uint32_t* size) {
  const uint64_t mend = pos + blen;
  bool have_id = false, have_size = false;
  for (int trip = 0; trip < 3 && pos < mend; ++trip) {
    const uint32_t tag = in.byte(pos++);
    if (tag == 0x0A) {
      if (have_id) return kBadMessage;
      uint32_t l;
      if (read_varint32(in, pos, mend, &l) != kVarOk) return kBadMessage;
      if (l > mend - pos) return kBadMessage;
      if (l != kIdBytes) return kBadChunkId;
      *id_off = pos;
      pos += kIdBytes;
      have_id = true;
    } else if (tag == 0x10) {
      if (have_size) return kBadMessage;
      if (read_varint32(in, pos, mend, size) != kVarOk) return kBadMessage;
      have_size = true;
    } else {
      return kBadMessage;
    }
  }
  return have_id && have_size ? kOk : kBadMessage;
}

// Every record of the BundleInfo in [off, off + len), in order:
// sink(k, id_off, size) for record k.  *count = the records read before the
// walk ended.  The trip bound: a hop consumes two bytes at least.
template <class In, class Sink>
ZC_HD inline int walk_records(const In& in, uint64_t off, uint32_t len, Sink& sink, uint32_t* count) {
  uint64_t pos = off;
  const uint64_t end = off + len;
  const uint32_t bound = len / 2 + 1;
  uint32_t k = 0;
  int rc = kOk;
  for (uint32_t trip = 0; trip < bound && pos < end; ++trip) {
    uint64_t body = 0, id_off = 0;
    uint32_t blen = 0, size = 0;
    rc = record_hop(in, pos, end, &body, &blen);
    if (rc == kOk) rc = record_body(in, body, blen, &id_off, &size);
    if (rc != kOk) break;
    sink(k, id_off, size);
    ++k;
  }
  *count = k;
  return rc;
}

// Adler-32 of bytes [0, n) of a source; the kernels use zc_adler32's kernel,
// this is for the serial reader below
template <class In>
ZC_HD inline uint32_t adler32_of(const In& in, uint64_t n) {
  uint64_t a = 1, b = 0, i = 0;
  while (i < n) {
    const uint64_t k = n - i < 5552 ? n - i : 5552;  // sums stay under 2^32
    for (uint64_t j = 0; j < k; ++j) {
      a += in.byte(i + j);
      b += a;
    }
    a %= 65521;
    b %= 65521;
    i += k;
  }
  return (uint32_t)(b << 16 | a);
}

// One whole file, serially: the definition the kernels' three passes add up
// to.  sink.bundle(b, id_off, info_off, info_len) for every bundle, then
// sink.record(b, k, id_off, size) for each of its records.  A status other
// than kOk means the file contributes nothing, whatever the sink has seen.
template <class In, class Sink>
ZC_HD inline int read_file(const In& in, uint64_t n, bool keyed, Sink& sink) {
  Frame f;
  int rc = frame_open(in, n, keyed, &f);
  if (rc != kOk) return rc;
  const uint64_t bound = max_bundles(f.end - f.pos) + 1;  // and the terminator
  uint64_t b = 0;
  for (uint64_t trip = 0; trip < bound; ++trip) {
    uint64_t id_off = 0, info_off = 0;
    uint32_t info_len = 0;
    rc = frame_next(in, &f, &id_off, &info_off, &info_len);
    if (rc != kFrameBundle) break;
    sink.bundle(b, id_off, info_off, info_len);
    struct Rec {
      Sink& s;
      uint64_t b;
      ZC_HD void operator()(uint32_t k, uint64_t id_off, uint32_t size) { s.record(b, k, id_off, size); }
    } rec{sink, b};
    uint32_t count = 0;
    rc = walk_records(in, info_off, info_len, rec, &count);
    if (rc != kOk) return rc;
    ++b;
    rc = kTruncated;  // a walk that ran out of trips ran out of bytes
  }
  if (rc != kFrameEnd) return rc;
  uint32_t stored = 0;
  for (int k = 0; k < 4; ++k) stored |= (uint32_t)in.byte(f.pos + k) << (8 * k);
  return adler32_of(in, f.pos) == stored ? kOk : kBadAdler;
}

// ---- the writer's arithmetic (zc_index_serialize, zc_index_file_size) ----

ZC_HD inline uint32_t varint_len(uint32_t v) {
  uint32_t n = 1;
  for (int k = 0; k < 4 && v >= 0x80; ++k) {
    v >>= 7;
    ++n;
  }
  return n;
}
ZC_HD inline uint32_t record_len(uint32_t size) { return 2 + kIdBytes + 1 + varint_len(size); }  // ChunkRecord's bytes
// bytes of a whole file whose serialized part (FileHeader to the terminator) is `body` bytes
ZC_HD inline uint64_t file_size(uint64_t body, bool keyed) {
  return keyed ? (16 + body + 4) / 16 * 16 + 16 : body + 4;
}

}  // namespace zcidx
