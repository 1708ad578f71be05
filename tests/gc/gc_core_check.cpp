// CPU unit check of zc_gc_core.h (test infrastructure only): the id table's
// insert and lookup, exactly as the kernels of zc_gc.hip run them, against
// std::set / std::map on
//   * random ids with repeats at table loads from one id to capacity - 1
//     (processing positions in shuffled order: the slot must end with the
//     smallest position of its id whatever came first);
//   * ids that differ from one another in byte 0 only, in byte 23 only, in the
//     crypto-hash half only or in the rolling-hash half only (a partial
//     compare would merge them);
//   * thousands of ids that share one slot hash, in a table they nearly fill:
//     every probe run wraps around the table's end;
//   * capacity_for's rule, with and without the test hook.
// Prints "ok <checks>"; exits non-zero on the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <vector>

#include "zc_gc_core.h"

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static void die(const char* what, long at) {
  printf("MISMATCH %s at %ld\n", what, at);
  exit(1);
}

typedef std::array<uint8_t, 24> Blob;
static long checks = 0;

// Insert ids[order[k]] for every k, then check every inserted id, and
// `strangers` ids that are not there, against a map id -> smallest position.
// The ids live in an exactly sized heap array, so a read past it is caught.
static uint32_t run_table(const std::vector<Blob>& blobs, const std::vector<uint32_t>& order, uint64_t slots,
                          const std::vector<Blob>& strangers, const char* what) {
  const size_t n = blobs.size();
  uint64_t* ids = (uint64_t*)malloc(std::max<size_t>(n, 1) * 24);
  for (size_t i = 0; i < n; i++) memcpy((uint8_t*)ids + 24 * i, blobs[i].data(), 24);
  uint32_t* table = (uint32_t*)malloc(slots * 4);
  for (uint64_t s = 0; s < slots; s++) table[s] = zcgc::kEmpty;
  std::map<Blob, uint32_t> want;
  uint32_t longest = 0;
  for (uint32_t p : order) {
    const uint32_t steps = zcgc::insert(table, slots - 1, ids, p);
    if (!steps || steps > slots) die(what, p);
    longest = std::max(longest, steps);
    auto it = want.find(blobs[p]);
    if (it == want.end())
      want[blobs[p]] = p;
    else
      it->second = std::min(it->second, p);
  }
  // the table holds each id once
  uint64_t filled = 0;
  for (uint64_t s = 0; s < slots; s++) filled += table[s] != zcgc::kEmpty;
  if (filled != want.size()) die(what, -1);
  for (size_t i = 0; i < n; i++) {
    uint32_t steps = 0;
    const uint32_t got = zcgc::lookup(table, slots - 1, ids, zcgc::load_id(ids, i), &steps);
    if (got != want[blobs[i]] || !steps || steps > slots) die(what, (long)i);
    longest = std::max(longest, steps);
    checks++;
  }
  for (size_t i = 0; i < strangers.size(); i++) {
    if (want.count(strangers[i])) continue;
    zcgc::Id key;
    memcpy(key.w, strangers[i].data(), 24);
    uint32_t steps = 0;
    if (zcgc::lookup(table, slots - 1, ids, key, &steps) != zcgc::kEmpty || !steps || steps > slots)
      die(what, -2 - (long)i);
    checks++;
  }
  free(table);
  free(ids);
  return longest;
}

static Blob random_blob() {
  Blob b;
  for (int k = 0; k < 3; k++) {
    const uint64_t w = rnd();
    memcpy(b.data() + 8 * k, &w, 8);
  }
  return b;
}

static std::vector<uint32_t> shuffled(size_t n) {
  std::vector<uint32_t> o(n);
  for (size_t i = 0; i < n; i++) o[i] = (uint32_t)i;
  for (size_t i = n; i > 1; i--) std::swap(o[i - 1], o[rnd() % i]);
  return o;
}

int main() {
  // random ids, each about twice, from 1 id up to capacity - 1 distinct ids
  for (uint64_t slots : {2ull, 4ull, 64ull, 1024ull}) {
    std::vector<uint64_t> loads = {1, slots / 2, slots - 1};
    if (slots > 8) loads.insert(loads.end(), {slots / 4, slots - 2, slots * 3 / 4});
    for (uint64_t distinct : loads) {
      if (!distinct) continue;
      std::vector<Blob> pool(distinct), blobs, strangers(40);
      for (auto& b : pool) b = random_blob();
      for (auto& b : strangers) b = random_blob();
      blobs = pool;
      for (uint64_t k = 0; k < distinct; k++) blobs.push_back(pool[rnd() % distinct]);
      std::swap(blobs[0], blobs[blobs.size() - 1]);
      const uint32_t longest = run_table(blobs, shuffled(blobs.size()), slots, strangers, "random ids");
      if (distinct == slots - 1 && slots >= 64 && longest < 8) die("a nearly full table without long probe runs", (long)slots);
    }
  }
  // near-equal ids: one base id with a single byte, or one half, changed
  {
    const Blob base = random_blob();
    std::vector<Blob> blobs = {base};
    for (int v = 1; v < 256; v++) {
      Blob a = base, b = base;
      a[0] ^= (uint8_t)v;   // byte 0 only
      b[23] ^= (uint8_t)v;  // byte 23 only
      blobs.push_back(a);
      blobs.push_back(b);
    }
    for (int k = 0; k < 200; k++) {
      Blob a = base, b = base;
      const uint64_t x = rnd(), y = rnd(), z = rnd() | 1;
      memcpy(a.data(), &x, 8);  // the crypto-hash half only (bytes 0..15)
      memcpy(a.data() + 8, &y, 8);
      uint64_t w;
      memcpy(&w, base.data() + 16, 8);
      w ^= z;  // the rolling-hash half only (bytes 16..23)
      memcpy(b.data() + 16, &w, 8);
      blobs.push_back(a);
      blobs.push_back(b);
    }
    const size_t distinct = blobs.size();
    for (size_t k = 0; k < distinct; k++) blobs.push_back(blobs[k]);  // and each once more
    std::vector<Blob> strangers;
    for (int byte = 0; byte < 24; byte++) {  // ids one byte away from an id that is there
      Blob s = blobs[1 + (size_t)byte * 7];
      s[byte] ^= 0x80;
      strangers.push_back(s);
    }
    for (uint64_t slots : {1024ull, 2048ull, 4096ull}) {
      if (slots <= distinct) continue;
      run_table(blobs, shuffled(blobs.size()), slots, strangers, "near-equal ids");
    }
  }
  // thousands of ids with one slot hash: w0 is chosen so that the fold, and so
  // the hash, is the same for every id; the start slot is the table's last
  // but two, so every run wraps
  {
    const uint64_t slots = 4096, n = 4000;
    uint64_t fold = 0;
    for (uint64_t c = 1;; c++) {
      zcgc::Id probe = {{c, 0, 0}};
      if (zcgc::slot_hash(probe, slots - 1) == slots - 3) {
        fold = c;
        break;
      }
    }
    std::vector<Blob> blobs(n);
    for (auto& b : blobs) {
      const uint64_t w1 = rnd(), w2 = rnd();
      const uint64_t w0 = fold ^ zcgc::rotl64(w1, 21) ^ zcgc::rotl64(w2, 42);
      memcpy(b.data(), &w0, 8);
      memcpy(b.data() + 8, &w1, 8);
      memcpy(b.data() + 16, &w2, 8);
      zcgc::Id id;
      memcpy(id.w, b.data(), 24);
      if (zcgc::slot_hash(id, slots - 1) != slots - 3) die("built ids do not share a hash", 0);
    }
    std::vector<Blob> strangers(8);
    for (auto& b : strangers) b = random_blob();
    strangers.push_back(blobs[5]);
    strangers.back()[11] ^= 1;
    for (size_t k = 0; k < 500; k++) blobs.push_back(blobs[k * 3]);
    const uint32_t longest = run_table(blobs, shuffled(blobs.size()), slots, strangers, "one slot hash");
    if (longest < n || longest > n + 1) die("the longest run of a full collision chain", longest);
  }
  // the capacity rule
  {
    using zcgc::capacity_for;
    const uint64_t none = 0;
    if (capacity_for(0, none) != 2 || capacity_for(1, none) != 2 || capacity_for(2, none) != 4 ||
        capacity_for(63, none) != 128 || capacity_for(64, none) != 128 || capacity_for(65, none) != 256 ||
        capacity_for(1024, none) != 2048 || capacity_for(1025, none) != 4096 ||
        capacity_for(0xfffffffeull, none) != (1ull << 33))
      die("capacity_for", 0);
    if (capacity_for(63, 6) != 64 || capacity_for(64, 6) != 128 || capacity_for(64, 7) != 128 ||
        capacity_for(1023, 10) != 1024 || capacity_for(1024, 10) != 2048 || capacity_for(1024, 11) != 2048 ||
        capacity_for(1000, 30) != 2048 || capacity_for(1000, -3) != 2048 || capacity_for(1000, 99) != 2048 ||
        capacity_for(1, 1) != 2 || capacity_for(3, 2) != 4)
      die("capacity_for with the test hook", 0);
    checks += 20;
  }
  printf("ok %ld\n", checks);
  return 0;
}
