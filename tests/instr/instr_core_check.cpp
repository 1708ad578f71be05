// CPU check of zc_instr_core.h: the steps zc_instr.hip's kernels run (hop, tile
// exits, chain, emit), single-threaded and tile by tile at T = 64, T = 256 and
// the default, against a plain serial parser written from Message::parse
// (message.cc:24-42) and BackupInstruction (zbackup.proto:149-159).
// Input: a file of cases, each a little-endian u64 length and the bytes
// (tests/instr_cases.py writes it).  On every case and tile: hop[p] > p,
// exit[p] >= the tile's end, the chain's positions strictly increase.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zc_instr_core.h"

static int g_fail = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      printf("FAIL %s: ", #c);        \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
      if (++g_fail > 20) exit(1);     \
    }                                 \
  } while (0)

struct Rec {
  uint32_t w[12];
};
struct Parsed {
  std::vector<Rec> recs;
  uint64_t messages = 0, bytes = 0;
  std::string error;  // "<what> at byte <N>", or empty
};

// the serial parser: one message after another
static bool rd_varint(const std::vector<uint8_t>& d, size_t* pos, size_t end, uint64_t* v) {
  *v = 0;
  for (int k = 0; k < 5; k++) {
    if (*pos >= end) return false;
    const uint8_t b = d[(*pos)++];
    *v |= (uint64_t)(b & 0x7f) << (7 * k);
    if (!(b & 0x80)) return *v <= 0xffffffffull;
  }
  return false;
}
static Parsed serial(const std::vector<uint8_t>& d) {
  Parsed r;
  const size_t n = d.size();
  size_t pos = 0;
  auto bad = [&](const char* what, size_t at) {
    r.error = std::string(what) + " at byte " + std::to_string(at);
    r.recs.clear();
    return r;
  };
  while (pos < n) {
    const size_t at = pos;
    uint64_t len;
    if (!rd_varint(d, &pos, n, &len)) return bad("truncated or overlong length varint", at);
    if (len > n - pos) return bad("instruction length past the end of the stream", at);
    const size_t end = pos + len;
    Rec chunk{}, bytes{};
    bool hc = false, hb = false;
    while (pos < end) {
      const size_t fat = pos;
      const uint8_t tag = d[pos++];
      if (tag != 0x0a && tag != 0x12) return bad("a field other than chunk_to_emit / bytes_to_emit", fat);
      uint64_t fl;
      if (!rd_varint(d, &pos, end, &fl)) return bad("truncated field length", fat);
      if (fl > end - pos) return bad("field past the end of its instruction", fat);
      if (tag == 0x0a) {
        if (fl != 24) return bad("chunk_to_emit is not a 24-byte chunk id", fat);
        if (hc) return bad("chunk_to_emit twice in one instruction", fat);
        hc = true;
        chunk.w[0] = 0;
        memcpy(&chunk.w[1], &d[pos], 24);
      } else {
        if (hb) return bad("bytes_to_emit twice in one instruction", fat);
        hb = true;
        bytes.w[0] = 1;
        const uint64_t off = pos, size = fl;
        memcpy(&bytes.w[8], &off, 8);
        memcpy(&bytes.w[10], &size, 8);
        r.bytes += size;
      }
      pos += fl;
    }
    if (hc) r.recs.push_back(chunk);
    if (hb) r.recs.push_back(bytes);
    r.messages++;
  }
  return r;
}

// the core's steps, as the kernels order them
static Parsed stepped(const std::vector<uint8_t>& d, uint32_t T) {
  Parsed r;
  const uint64_t n = d.size();
  if (!n) return r;
  const uint8_t* p = d.data();
  const uint32_t tiles = (uint32_t)((n + T - 1) / T), rounds = zcin::log2_of(T);
  std::vector<uint32_t> exits(n), a(T), b(T), entry(tiles, zcin::kNone), cnt(tiles);
  std::vector<uint64_t> place(tiles);
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t base = t * T, c = (uint32_t)std::min<uint64_t>(T, n - base);
    for (uint32_t i = 0; i < c; i++) {
      a[i] = zcin::hop_at(p, n, base + i);
      CHECK(a[i] > base + i, "hop[%u] = %u", base + i, a[i]);
      CHECK(a[i] == zcin::kBad || a[i] <= n, "hop[%u] = %u past %llu", base + i, a[i], (unsigned long long)n);
    }
    const uint32_t* x = zcin::tile_exits(a.data(), b.data(), base, c, rounds);
    for (uint32_t i = 0; i < c; i++) {
      CHECK(x[i] >= base + c, "exit[%u] = %u, tile end %u", base + i, x[i], base + c);
      exits[base + i] = x[i];
    }
  }
  uint32_t pos = 0, last_tile = 0;
  for (uint32_t k = 0; k < tiles && pos < n; k++) {
    const uint32_t t = pos / T;
    CHECK(k == 0 || t > last_tile, "chain step %u stays in tile %u", k, t);
    last_tile = t;
    entry[t] = pos;
    const uint32_t x = exits[pos];
    if (x == zcin::kBad) break;
    CHECK(x > pos, "chain does not advance at %u", pos);
    pos = x;
  }
  uint64_t error = zcin::kNoError, total = 0;
  for (uint32_t t = 0; t < tiles; t++) {
    cnt[t] = 0;
    place[t] = total;
    if (entry[t] == zcin::kNone) continue;
    const uint64_t end = std::min<uint64_t>(n, (uint64_t)(t + 1) * T);
    const zcin::TileSum s = zcin::tile_walk(p, n, entry[t], end, nullptr);
    cnt[t] = s.entries;
    total += s.entries;
    r.messages += s.messages;
    r.bytes += s.bytes;
    if (s.error < error) error = s.error;
  }
  if (error != zcin::kNoError) {
    r.error = std::string(zcin::err_text((uint32_t)(error & 0xff))) + " at byte " + std::to_string(error >> 8);
    return r;
  }
  r.recs.resize(total);
  for (uint32_t t = 0; t < tiles; t++) {
    if (entry[t] == zcin::kNone || !cnt[t]) continue;
    const uint64_t end = std::min<uint64_t>(n, (uint64_t)(t + 1) * T);
    const zcin::TileSum s = zcin::tile_walk(p, n, entry[t], end, r.recs[place[t]].w);
    CHECK(s.entries == cnt[t], "tile %u wrote %u entries, counted %u", t, s.entries, cnt[t]);
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  // the tile the environment asks for: what tile_for accepts and what it does not
  CHECK(zcin::tile_for(nullptr) == zcin::kTileDefault && zcin::tile_for("64") == 64 && zcin::tile_for("4096") == 4096,
        "tile_for");
  CHECK(zcin::tile_for("32") == zcin::kTileDefault && zcin::tile_for("100") == zcin::kTileDefault &&
            zcin::tile_for("65536") == zcin::kTileDefault && zcin::tile_for("x") == zcin::kTileDefault,
        "tile_for refusals");
  uint64_t cases = 0, checks = 0;
  for (;;) {
    uint64_t len;
    if (fread(&len, 8, 1, f) != 1) break;
    std::vector<uint8_t> d(len);
    if (len && fread(d.data(), 1, len, f) != len) return 2;
    const Parsed want = serial(d);
    for (uint32_t T : {64u, 256u, zcin::kTileDefault}) {
      const Parsed got = stepped(d, T);
      CHECK(got.error == want.error, "case %llu T %u: '%s' vs '%s'", (unsigned long long)cases, T, got.error.c_str(),
            want.error.c_str());
      if (want.error.empty()) {
        CHECK(got.messages == want.messages && got.bytes == want.bytes, "case %llu T %u: %llu messages vs %llu",
              (unsigned long long)cases, T, (unsigned long long)got.messages, (unsigned long long)want.messages);
        CHECK(got.recs.size() == want.recs.size() &&
                  (want.recs.empty() || !memcmp(got.recs.data(), want.recs.data(), 48 * want.recs.size())),
              "case %llu T %u: records differ (%zu vs %zu)", (unsigned long long)cases, T, got.recs.size(),
              want.recs.size());
      }
      checks++;
    }
    cases++;
  }
  fclose(f);
  if (g_fail) return 1;
  printf("ok %llu cases %llu checks\n", (unsigned long long)cases, (unsigned long long)checks);
  return 0;
}
