// TEST INFRASTRUCTURE: zc_range_core.h on the host.  The per-piece routine the
// kernel of zc_range.hip runs (the search, the walk, the clip), with a byte
// sink that aborts on any access outside its slot or its destination, against a
// direct restatement of IndexedRestorer::saveData's walk (std::upper_bound, one
// step back, the Outputer's clip).  Prints "ok N": the reads compared.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zc_range_core.h"

namespace {

constexpr uint64_t kPiece = 65536;  // zclzo::kPiece: the host cuts reads into these
uint64_t g_checks = 0;

[[noreturn]] void die(const std::string& what) {
  fprintf(stderr, "FAIL: %s\n", what.c_str());
  abort();
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  g_rng += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_rng;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Stream {
  std::vector<std::vector<uint8_t>> slots;
  std::vector<uint64_t> slot_size, pos, off, size;
  std::vector<uint32_t> slot;

  uint64_t n() const { return off.size(); }
  uint64_t total() const { return pos.back(); }
  zcrange::Index view() const {
    return zcrange::Index{pos.data(), slot.data(), off.data(), n(), slot_size.data(), (uint32_t)slot_size.size()};
  }
};

// entries of the given sizes, each somewhere in one of n_slots payloads
Stream make_stream(const std::vector<uint64_t>& sizes, uint32_t n_slots, uint64_t slot_bytes) {
  Stream s;
  s.slots.resize(n_slots);
  for (uint32_t k = 0; k < n_slots; ++k) {
    s.slots[k].resize(slot_bytes + k);  // sizes differ, so a slot mix-up shows
    for (uint8_t& b : s.slots[k]) b = (uint8_t)rnd();
    s.slot_size.push_back(s.slots[k].size());
  }
  uint64_t sum = 0;
  for (uint64_t z : sizes) {
    const uint32_t k = n_slots ? (uint32_t)(rnd() % n_slots) : 0;
    if (z > s.slot_size[k]) die("make_stream: an entry larger than its slot");
    // ends flush with the slot now and then: the bound check's edge
    const uint64_t room = s.slot_size[k] - z;
    const uint64_t o = rnd() % 4 == 0 ? room : rnd() % (room + 1);
    s.pos.push_back(sum);
    s.slot.push_back(k);
    s.off.push_back(o);
    s.size.push_back(z);
    sum += z;
  }
  s.pos.push_back(sum);
  return s;
}

// saveData, restated (backup_restorer.cc:228-316)
void naive_read(const Stream& s, uint64_t offset, uint64_t size, uint8_t* data) {
  if (offset + size > s.total() || offset + size < offset) die("naive_read: out of range");
  if (!s.n()) return;
  // the first entry whose range starts after offset, then one back
  std::vector<uint64_t>::const_iterator it = std::upper_bound(s.pos.begin(), s.pos.begin() + s.n(), offset);
  if (it == s.pos.begin()) die("naive_read: nothing starts at or before the offset");
  uint64_t e = (uint64_t)(it - s.pos.begin()) - 1;
  uint64_t position = s.pos[e];
  for (; e < s.n() && size; ++e) {
    const uint64_t chunk_size = s.size[e];
    uint64_t start = 0;
    if (position < offset) start = offset - position;
    uint64_t end = chunk_size;
    if (position + chunk_size > offset + size) end = offset + size - position;
    const uint64_t part = end - start;
    memcpy(data, s.slots[s.slot[e]].data() + s.off[e] + start, part);
    offset += part;
    data += part;
    size -= part;
    position += chunk_size;
  }
  if (size) die("naive_read: the walk ended early");
}

// the byte sink: aborts on any access outside the slot or the piece
struct ByteSink {
  const Stream* s;
  uint8_t* dst;        // the piece's destination
  uint64_t piece;      // its size
  uint64_t next = 0;   // the calls tile the piece in order
  bool operator()(uint32_t slot, uint64_t src_off, uint64_t at, uint64_t len) {
    if (slot >= s->slots.size()) die("sink: slot out of range");
    if (src_off > s->slots[slot].size() || len > s->slots[slot].size() - src_off) die("sink: read outside the slot");
    if (at != next || len == 0 || len > piece - at) die("sink: write outside the piece, or out of order");
    memcpy(dst + at, s->slots[slot].data() + src_off, len);
    next = at + len;
    return true;
  }
};

// one read the way zc_range_read serves it: pieces of at most 64 KiB
void piece_read(const Stream& s, uint64_t offset, uint64_t size, uint8_t* data) {
  const zcrange::Index v = s.view();
  for (uint64_t k = 0; k < size; k += kPiece) {
    const uint64_t len = std::min(kPiece, size - k);
    ByteSink sink{&s, data + k, len};
    const uint32_t bits = zcrange::serve_piece(v, offset + k, len, sink);
    if (bits) die("serve_piece raised status " + std::to_string(bits));
    if (sink.next != len) die("serve_piece left part of a piece unwritten");
  }
}

void check_read(const Stream& s, uint64_t offset, uint64_t size) {
  static std::vector<uint8_t> want, got;
  want.assign(size + 32, 0xEE);
  got.assign(size + 32, 0xEE);
  naive_read(s, offset, size, want.data() + 16);
  piece_read(s, offset, size, got.data() + 16);
  if (want != got)
    die("read [" + std::to_string(offset) + ", +" + std::to_string(size) + ") of a stream of " +
        std::to_string(s.n()) + " entries differs");
  // the slots the read touches: mark_slots against the entries that overlap it
  std::vector<uint8_t> seen(s.slots.size(), 0), expect(s.slots.size(), 0);
  zcrange::mark_slots(s.view(), offset, size, seen.data());
  for (uint64_t e = 0; e < s.n() && size; ++e)
    if (s.size[e] && s.pos[e] < offset + size && s.pos[e + 1] > offset) expect[s.slot[e]] = 1;
  if (seen != expect) die("mark_slots differs at offset " + std::to_string(offset));
  ++g_checks;
}

// every read whose start or end lies at an entry edge -1 / 0 / +1, for reads of
// 0, 1 and 64 KiB + 1 bytes (and the other lengths given), and the whole stream
void check_edges(const Stream& s, const std::vector<uint64_t>& lens, bool whole) {
  const uint64_t total = s.total();
  for (uint64_t e = 0; e <= s.n(); ++e)
    for (int d = -1; d <= 1; ++d) {
      if ((d < 0 && s.pos[e] == 0) || (d > 0 && s.pos[e] == total)) continue;
      const uint64_t edge = s.pos[e] + (uint64_t)(int64_t)d;
      for (uint64_t len : lens) {
        if (len <= total - edge) check_read(s, edge, len);  // starts there
        if (len <= edge) check_read(s, edge - len, len);    // ends there
      }
    }
  if (whole) check_read(s, 0, total);
  check_read(s, total, 0);  // 0 bytes at the very end: allowed, as in the reference
}

void check_search(const Stream& s) {
  // upper_bound against the standard library's at every edge and beside it
  for (uint64_t e = 0; e <= s.n(); ++e)
    for (int d = -1; d <= 1; ++d) {
      const uint64_t x = s.pos[e] + (uint64_t)(int64_t)d;
      const uint64_t want = (uint64_t)(std::upper_bound(s.pos.begin(), s.pos.begin() + s.n(), x) - s.pos.begin());
      if (zcrange::upper_bound(s.pos.data(), s.n(), x) != want) die("upper_bound differs");
    }
}

const uint64_t kSizes[] = {0, 1, 2, 15, 16, 17, 65535, 65536, 65537};

std::vector<uint64_t> random_sizes(size_t n) {
  std::vector<uint64_t> v(n);
  for (uint64_t& z : v) z = kSizes[rnd() % 9];
  return v;
}

}  // namespace

int main() {
  const std::vector<uint64_t> lens = {0, 1, 65537};
  // n = 0: the only read is 0 bytes at 0
  {
    Stream s = make_stream({}, 1, 16);
    check_read(s, 0, 0);
    check_search(s);
  }
  // n = 1 and n = 2, every size and every pair of sizes
  for (uint64_t a : kSizes) {
    Stream s = make_stream({a}, 2, 70000);
    check_search(s);
    check_edges(s, lens, true);
    for (uint64_t b : kSizes) {
      Stream t = make_stream({a, b}, 2, 70000);
      check_search(t);
      check_edges(t, {0, 1, 2, 17, 65537}, true);
    }
  }
  // runs of empty entries at the start, in the middle and at the end
  {
    std::vector<uint64_t> z(7, 0);
    for (uint64_t a : {1, 16, 65537}) z.push_back((uint64_t)a);
    z.insert(z.end(), 9, 0);
    for (uint64_t a : {65536, 2, 15}) z.push_back((uint64_t)a);
    z.insert(z.end(), 5, 0);
    Stream s = make_stream(z, 3, 70000);
    check_search(s);
    check_edges(s, {0, 1, 2, 16, 65536, 65537, 131075}, true);
    Stream only = make_stream(std::vector<uint64_t>(11, 0), 1, 16);  // nothing but empty entries
    check_search(only);
    check_edges(only, lens, true);
  }
  // n = 1,000 entries of random sizes from the list, in five slots
  {
    Stream s = make_stream(random_sizes(1000), 5, 1 << 20);
    check_search(s);
    check_edges(s, lens, true);
    for (int i = 0; i < 2000; ++i) {
      const uint64_t o = rnd() % (s.total() + 1);
      check_read(s, o, std::min<uint64_t>(rnd() % 300000, s.total() - o));
    }
  }
  // tiny entries: many of them in one piece
  {
    std::vector<uint64_t> z;
    for (int i = 0; i < 3000; ++i) z.push_back(rnd() % 4);
    Stream s = make_stream(z, 2, 4096);
    check_search(s);
    check_edges(s, {0, 1, 100}, true);
  }
  // positions on both sides of 2^32: one extent emitted many times
  {
    const uint64_t ext = 1 << 20, reps = 4200;
    Stream s;
    s.slots.resize(1);
    s.slots[0].resize(ext);
    for (uint8_t& b : s.slots[0]) b = (uint8_t)rnd();
    s.slot_size.push_back(ext);
    for (uint64_t i = 0; i < reps; ++i) {
      s.pos.push_back(i * ext);
      s.slot.push_back(0);
      s.off.push_back(0);
      s.size.push_back(ext);
    }
    s.pos.push_back(reps * ext);
    check_search(s);
    const uint64_t two32 = 1ull << 32;
    for (uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)16, (uint64_t)65537, (uint64_t)131077})
      for (int d = -2; d <= 2; ++d) {
        check_read(s, two32 + (uint64_t)(int64_t)d, len);              // starts at 2^32 +- d
        check_read(s, two32 + (uint64_t)(int64_t)d - len, len);        // ends there
        check_read(s, two32 - len / 2 + (uint64_t)(int64_t)d, len);    // straddles it
        check_read(s, s.total() - len, len);                           // ends at the total
      }
    for (uint64_t e = 4090; e <= 4100; ++e)  // the edges around 2^32 (entry 4096 starts there)
      for (int d = -1; d <= 1; ++d)
        for (uint64_t len : lens) {
          check_read(s, s.pos[e] + (uint64_t)(int64_t)d, len);
          check_read(s, s.pos[e] + (uint64_t)(int64_t)d - len, len);
        }
  }
  // a range at fault is refused, and nothing of it reaches the sink
  {
    Stream s = make_stream({100, 200, 300}, 1, 1000);
    s.off[1] = 900;  // 900 + 200 > 1000
    uint8_t buf[600];
    ByteSink sink{&s, buf, 600};
    if (zcrange::serve_piece(s.view(), 0, 600, sink) != zcrange::kBadRange || sink.next != 100)
      die("an entry past its slot was not refused");
    s.off[1] = 0;
    s.slot[2] = 7;
    ByteSink sink2{&s, buf, 600};
    if (zcrange::serve_piece(s.view(), 0, 600, sink2) != zcrange::kBadSlot || sink2.next != 300)
      die("an entry naming no slot was not refused");
    g_checks += 2;
  }
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
