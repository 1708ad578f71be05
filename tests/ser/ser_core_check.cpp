// CPU check of zc_ser_core.h: the length function, the header and chunk-id
// writers and the run decomposition zc_ser.hip's kernels use, single-threaded,
// against a plain serializer written from Message::serialize (message.cc:16-23)
// and BackupInstruction (zbackup.proto:149-159): a varint32 of the body's size,
// then the body -- one length-delimited field, 1 (chunk_to_emit) or 2
// (bytes_to_emit).
//
// emulate() walks the records the way the device does: positions from the
// exclusive scan of the lengths, groups of 64, runs cut at the big records,
// every run assembled in a buffer of the kernel's LDS size at the output's
// 16-byte phase and then copied out, the big payloads in 64 KiB pieces.  It
// counts the writes to every output byte: each is written exactly once.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zc_ser_core.h"

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(c, ...)             \
  do {                            \
    g_checks++;                   \
    if (!(c)) {                   \
      printf("FAIL %s: ", #c);    \
      printf(__VA_ARGS__);        \
      printf("\n");               \
      if (++g_fail > 20) exit(1); \
    }                             \
  } while (0)

// ---- the plain serializer ----
static void plain_varint(std::string& s, uint64_t v) {
  while (v >= 0x80) {
    s.push_back((char)(uint8_t)(v | 0x80));
    v >>= 7;
  }
  s.push_back((char)(uint8_t)v);
}
// everything in front of a field's bytes, for a field of `len` bytes
static std::string plain_header(int field, uint64_t len) {
  std::string inner;
  inner.push_back((char)(field << 3 | 2));
  plain_varint(inner, len);
  std::string s;
  plain_varint(s, inner.size() + len);
  return s + inner;
}
static std::string plain_message(const zcser::Rec& r, const uint8_t* stream) {
  if (r.kind == 2) return plain_header(2, r.size) + std::string((const char*)stream + r.offset, r.size);
  std::string id;
  for (int k = 0; k < 4; k++)
    for (int b = 0; b < 4; b++) id.push_back((char)(uint8_t)(r.sha[k] >> (8 * b)));
  for (int b = 0; b < 8; b++) id.push_back((char)(uint8_t)(r.rolling >> (8 * b)));
  return plain_header(1, 24) + id;
}

// ---- the device's walk ----
constexpr uint32_t kLds = (15 + zcser::kRunMax + 15) / 16 * 16;  // zc_ser.hip's kLdsBytes

static void emulate(const std::vector<zcser::Rec>& recs, const uint8_t* stream, std::vector<uint8_t>& out,
                    std::vector<uint8_t>& hits) {
  const size_t n = recs.size();
  std::vector<uint64_t> pos(n + 1, 0);
  for (size_t i = 0; i < n; i++) pos[i + 1] = pos[i] + zcser::message_len(recs[i].kind, recs[i].size);
  out.assign(pos[n], 0);
  hits.assign(pos[n], 0);
  std::vector<uint8_t> lds(kLds);
  for (size_t first = 0; first < n; first += zcser::kGroup) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(zcser::kGroup, n - first);
    uint64_t big = 0;
    for (uint32_t l = 0; l < cnt; l++)
      if (zcser::is_big(recs[first + l].kind, recs[first + l].size)) big |= 1ull << l;
    uint32_t lo = 0, runs = 0;
    while (lo < cnt) {
      CHECK(++runs <= zcser::kGroup, "group at %zu: more than 64 runs", first);
      const uint32_t hi = zcser::run_last(big, lo, cnt);
      CHECK(hi >= lo && hi < cnt, "run_last(%llx, %u, %u) = %u", (unsigned long long)big, lo, cnt, hi);
      for (uint32_t l = lo; l < hi; l++) CHECK(!(big >> l & 1), "a big record inside a run");
      CHECK(hi == cnt - 1 || (big >> hi & 1), "a run ends before the group without a big record");
      const zcser::Rec& last = recs[first + hi];
      const uint64_t a = pos[first + lo];
      const uint64_t len = pos[first + hi] + zcser::staged_len(last.kind, last.size) - a;
      CHECK(len <= zcser::kRunMax, "a run of %llu bytes", (unsigned long long)len);
      const uint32_t phase = (uint32_t)(a & 15);
      memset(lds.data(), 0xcc, lds.size());
      for (uint32_t l = lo; l <= hi; l++) {
        const zcser::Rec& r = recs[first + l];
        const uint32_t at = phase + (uint32_t)(pos[first + l] - a);
        const uint32_t staged = zcser::staged_len(r.kind, r.size);
        CHECK((uint64_t)at + staged <= kLds, "lane %u writes LDS [%u, +%u)", l, at, staged);
        uint8_t hdr[zcser::kHeaderMax + 8];
        memset(hdr, 0xee, sizeof hdr);
        const uint32_t h = zcser::put_header(hdr, r.kind, r.size);
        CHECK(h == zcser::header_len(r.kind, r.size) && h <= zcser::kHeaderMax && hdr[h] == 0xee, "header of %u bytes",
              h);
        memcpy(&lds[at], hdr, h);
        if (r.kind != zcser::kKindBytes) {
          CHECK(staged == zcser::kChunkMessage && h + zcser::kChunkId == staged, "a chunk message of %u bytes", staged);
          zcser::put_chunk_id(&lds[at + h], r);
        } else if (!zcser::is_big(r.kind, r.size)) {
          CHECK(at + staged - r.size == at + h, "the payload does not end the message");
          memcpy(&lds[at + h], stream + r.offset, r.size);
        }
      }
      for (uint64_t b = 0; b < len; b++) {
        out[a + b] = lds[phase + b];
        hits[a + b]++;
      }
      lo = hi + 1;
    }
  }
  for (size_t i = 0; i < n; i++) {
    const zcser::Rec& r = recs[i];
    const uint32_t pc = zcser::pieces(r.kind, r.size);
    CHECK((pc != 0) == zcser::is_big(r.kind, r.size), "pieces of record %zu", i);
    const uint64_t dst = pos[i] + zcser::header_len(r.kind, r.size);
    for (uint32_t q = 0; q < pc; q++) {
      const uint64_t at = q * zcser::kPiece, len = std::min<uint64_t>(zcser::kPiece, r.size - at);
      CHECK(at < r.size, "an empty piece");
      memcpy(&out[dst + at], stream + r.offset + at, len);
      for (uint64_t b = 0; b < len; b++) hits[dst + at + b]++;
    }
  }
}

static void compare(const char* what, const std::vector<zcser::Rec>& recs, const uint8_t* stream) {
  std::string want;
  for (const zcser::Rec& r : recs) {
    const std::string m = plain_message(r, stream);
    CHECK(m.size() == zcser::message_len(r.kind, r.size), "%s: message_len(%u, %u)", what, r.kind, r.size);
    want += m;
  }
  std::vector<uint8_t> out, hits;
  emulate(recs, stream, out, hits);
  CHECK(out.size() == want.size(), "%s: %zu bytes, the serializer gives %zu", what, out.size(), want.size());
  if (out.size() != want.size()) return;
  CHECK(!out.size() || !memcmp(out.data(), want.data(), out.size()), "%s: the bytes differ", what);
  size_t wrong = 0;
  for (uint8_t h : hits) wrong += h != 1;
  CHECK(!wrong, "%s: %zu output bytes not written exactly once", what, wrong);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_rng += 0x9e3779b97f4a7c15ull;
  uint64_t z = g_rng;
  z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ z >> 27) * 0x94d049bb133111ebull;
  return z ^ z >> 31;
}

static zcser::Rec chunk(uint32_t kind) {
  zcser::Rec r{};
  r.kind = kind;
  r.size = (uint32_t)rnd();  // a chunk's size and offset are not serialized
  r.offset = rnd();
  r.rolling = rnd();
  for (uint32_t& w : r.sha) w = (uint32_t)rnd();
  return r;
}
static zcser::Rec raw(uint64_t offset, uint32_t size) {
  zcser::Rec r{};
  r.kind = zcser::kKindBytes;
  r.offset = offset;
  r.size = size;
  r.rolling = rnd();  // not serialized
  return r;
}

int main() {
  // the outer and inner varint steps, each with one below and one above
  const uint64_t steps[] = {0,     1,       125,     126,     127,           128,       16381,
                            16383, 16384,   2097148, 2097151, 2097152,       (1u << 28) - 6, 1u << 28};
  std::vector<uint32_t> sizes;
  for (uint64_t s : steps)
    for (int d = -1; d <= 1; d++)
      if (s + d <= 0xffffffffull && !(s == 0 && d < 0)) sizes.push_back((uint32_t)(s + d));
  sizes.push_back(0xffffffffu);
  const uint32_t kFull = 2097153;  // the longest payload written out; the others: lengths and headers
  std::vector<uint8_t> stream(kFull + 64);
  for (uint8_t& b : stream) b = (uint8_t)rnd();

  for (uint32_t size : sizes) {
    const std::string h = plain_header(2, size);
    uint8_t buf[32];
    memset(buf, 0xee, sizeof buf);
    const uint32_t k = zcser::put_header(buf, zcser::kKindBytes, size);
    CHECK(k == h.size() && k == zcser::header_len(zcser::kKindBytes, size) && k <= zcser::kHeaderMax &&
              !memcmp(buf, h.data(), k) && buf[k] == 0xee,
          "header of %u bytes", size);
    CHECK(zcser::message_len(zcser::kKindBytes, size) == h.size() + (uint64_t)size, "message_len of %u bytes", size);
    CHECK(zcser::staged_len(zcser::kKindBytes, size) == (size <= zcser::kStage ? h.size() + size : h.size()),
          "staged_len of %u bytes", size);
    CHECK(zcser::pieces(zcser::kKindBytes, size) == (size <= zcser::kStage ? 0 : (size + 65535ull) / 65536),
          "pieces of %u bytes", size);
    if (size > kFull) continue;
    // alone, and between chunks at every phase of the output
    for (uint32_t lead = 0; lead < 16; lead += (size > 70000 ? 5 : 1)) {
      std::vector<zcser::Rec> recs;
      if (lead) recs.push_back(raw(3, lead));
      recs.push_back(chunk(0));
      recs.push_back(raw(lead + 1, size));
      recs.push_back(chunk(1));
      char what[64];
      snprintf(what, sizeof what, "size %u lead %u", size, lead);
      compare(what, recs, stream.data());
    }
  }
  // every kind value but ZC_BYTES is a chunk
  for (uint32_t kind : {0u, 1u, 3u, 7u, 0xffffffffu}) {
    const zcser::Rec r = chunk(kind);
    CHECK(zcser::message_len(kind, r.size) == 27 && zcser::header_len(kind, r.size) == 3 && !zcser::pieces(kind, r.size),
          "chunk kind %u", kind);
    compare("a chunk", {r}, stream.data());
  }
  compare("no records", {}, stream.data());
  CHECK(zcser::kStagedMax == zcser::message_len(zcser::kKindBytes, zcser::kStage), "kStagedMax");
  // run_last on its own
  CHECK(zcser::run_last(0, 0, 64) == 63 && zcser::run_last(0, 5, 7) == 6, "no big record");
  CHECK(zcser::run_last(1ull << 63, 0, 64) == 63 && zcser::run_last(1ull << 63, 63, 64) == 63, "the last lane");
  CHECK(zcser::run_last(0x11, 0, 64) == 0 && zcser::run_last(0x11, 1, 64) == 4 && zcser::run_last(0x11, 5, 64) == 63,
        "two big records");
  CHECK(zcser::run_last(~0ull, 17, 64) == 17, "all big");
  // record counts around the group, every mix
  for (size_t n : {1, 63, 64, 65, 127, 128, 129, 700}) {
    for (int mix = 0; mix < 5; mix++) {
      std::vector<zcser::Rec> recs;
      for (size_t i = 0; i < n; i++) {
        const bool bytes = mix == 1 || (mix == 2 && (i & 1)) || (mix >= 3 && rnd() % 3 == 0);
        if (!bytes) {
          recs.push_back(chunk((uint32_t)(rnd() % 2)));
          continue;
        }
        uint32_t size = (uint32_t)(rnd() % 130);
        if (mix == 4 && rnd() % 4 == 0) size = 120 + (uint32_t)(rnd() % 70000);
        if (mix == 4 && rnd() % 50 == 0) size = (uint32_t)(rnd() % kFull);
        recs.push_back(raw(rnd() % (stream.size() - size), size));
      }
      char what[64];
      snprintf(what, sizeof what, "%zu records mix %d", n, mix);
      compare(what, recs, stream.data());
    }
  }
  // a group of big records only, and big records at a group's two ends
  {
    std::vector<zcser::Rec> recs;
    for (int i = 0; i < 64; i++) recs.push_back(raw(i, 129 + (uint32_t)i));
    compare("64 big records", recs, stream.data());
    recs.clear();
    for (int i = 0; i < 192; i++)
      recs.push_back(i % 64 == 0 || i % 64 == 63 ? raw(i, 70000 + (uint32_t)i) : i & 1 ? raw(i, 5) : chunk(0));
    compare("big records at the ends", recs, stream.data());
  }
  if (g_fail) return 1;
  printf("ok %ld checks\n", g_checks);
  return 0;
}
