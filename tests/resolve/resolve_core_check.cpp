// CPU unit check of zc_resolve_core.h (test infrastructure only): the chunk
// index built single-threaded with exactly the steps the kernels of
// zc_resolve.hip run -- bundle_of / record_of, zcgc::insert, insert_pair, find,
// resolve_entry -- against std::map / std::set on
//   * random repositories with ids shared between bundles and repeated inside
//     one, in bundles of 0 to a few hundred records, at table loads from the
//     default capacity down to one free slot;
//   * bundles of 0, 1, 64, 65 and 5,000 records in one input;
//   * ids that share one slot hash in a table they nearly fill, among foreign
//     ids: the probe runs wrap around the table's end;
//   * an id in 2 and in 5 bundles (the first bundle in input order owns it);
//   * an id twice in a bundle while an earlier bundle owns it (the flag is
//     exact), and twice in a bundle no entry uses;
//   * three records of 2^32 - 1 bytes in one bundle (64-bit offsets), size-0
//     records, an empty input, entries of bytes only, missing ids.
// Every array is an exactly sized heap block, so a table index outside its
// capacity is caught by the sanitizer; a walk longer than the capacity aborts.
// Prints "ok <checks>"; exits non-zero on the first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <set>
#include <vector>

#include "zc_resolve_core.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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
struct Rec {
  Blob id;
  uint32_t size;
};
typedef std::vector<std::vector<Rec>> Bundles;
struct Ent {
  uint32_t kind;
  Blob id;
  uint64_t data_off, size;
};
static long checks = 0;

static Blob random_blob() {
  Blob b;
  for (int k = 0; k < 3; k++) {
    const uint64_t w = rnd();
    memcpy(b.data() + 8 * k, &w, 8);
  }
  return b;
}
static Blob blob_with_fold(uint64_t fold) {
  const uint64_t w1 = rnd(), w2 = rnd();
  const uint64_t w0 = fold ^ zcgc::rotl64(w1, 21) ^ zcgc::rotl64(w2, 42);
  Blob b;
  memcpy(b.data(), &w0, 8);
  memcpy(b.data() + 8, &w1, 8);
  memcpy(b.data() + 16, &w2, 8);
  return b;
}
static zcgc::Id id_of(const Blob& b) {
  zcgc::Id v;
  memcpy(v.w, b.data(), 24);
  return v;
}

template <class T>
static T* exact(size_t n) {
  return (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
}

// Builds the index over `bundles` in tables of `slots` slots and checks it and
// the resolve of `entries` against the containers.  Returns the longest walk.
static uint32_t run_case(const Bundles& bundles, const std::vector<Ent>& entries, int test_bits, const char* what) {
  const uint32_t B = (uint32_t)bundles.size();
  uint64_t N = 0;
  for (const auto& b : bundles) N += b.size();
  const uint64_t slots = zcgc::capacity_for(N, test_bits), mask = slots - 1;
  // zc_gc_input's layout
  uint64_t* ids = exact<uint64_t>(3 * N);
  uint32_t* sizes = exact<uint32_t>(N);
  uint64_t* bf = exact<uint64_t>(B + 1);
  uint64_t* run = exact<uint64_t>(N + 1);
  {
    uint64_t r = 0;
    bf[0] = 0;
    run[0] = 0;
    for (uint32_t b = 0; b < B; b++) {
      for (const Rec& rec : bundles[b]) {
        memcpy((uint8_t*)ids + 24 * r, rec.id.data(), 24);
        sizes[r] = rec.size;
        run[r + 1] = run[r] + rec.size;
        r++;
      }
      bf[b + 1] = r;
    }
  }
  // zc_rs_place
  uint64_t* idp = exact<uint64_t>(3 * N);
  uint32_t* szp = exact<uint32_t>(N);
  uint64_t* offp = exact<uint64_t>(N);
  uint32_t* bund = exact<uint32_t>(N);
  for (uint64_t p = 0; p < N; p++) {
    const uint32_t b = zcrs::bundle_of(bf, B, p);
    if (b >= B || bf[b] > p || p >= bf[b + 1]) die(what, (long)p);
    const uint64_t r = zcrs::record_of(bf, b, p);
    if (r < bf[b] || r >= bf[b + 1] || zcrs::record_of(bf, b, r) != p) die(what, (long)p);
    memcpy(idp + 3 * p, ids + 3 * r, 24);
    szp[p] = sizes[r];
    offp[p] = run[r] - run[bf[b]];
    bund[p] = b;
  }
  // the tables, positions in a shuffled order: the result must not depend on it
  uint32_t* table = exact<uint32_t>(slots);
  uint32_t* pairs = exact<uint32_t>(slots);
  for (uint64_t s = 0; s < slots; s++) table[s] = pairs[s] = zcgc::kEmpty;
  std::vector<uint8_t> bdup(B, 0);
  std::vector<uint32_t> order(N);
  for (uint64_t p = 0; p < N; p++) order[p] = (uint32_t)p;
  for (uint64_t p = N; p > 1; p--) std::swap(order[p - 1], order[rnd() % p]);
  uint32_t longest = 0;
  for (uint32_t p : order) {
    uint32_t steps = zcgc::insert(table, mask, idp, p);
    if (!steps || steps > slots) die(what, p);
    longest = std::max(longest, steps);
    bool twice = false;
    steps = zcrs::insert_pair(pairs, mask, idp, bund, p, &twice);
    if (!steps || steps > slots) die(what, p);
    longest = std::max(longest, steps);
    if (twice) bdup[bund[p]] = 1;
  }
  // the containers: registerNewChunkId in loadIndex order, Bundle::Reader's map
  struct Where {
    uint32_t bundle, size;
    uint64_t off;
  };
  std::map<Blob, Where> owner;
  std::vector<uint8_t> want_dup(B, 0);
  for (uint32_t b = 0; b < B; b++) {
    std::vector<uint64_t> off(bundles[b].size());
    std::set<Blob> seen;
    uint64_t next = 0;
    for (size_t x = 0; x < bundles[b].size(); x++) {
      if (!seen.insert(bundles[b][x].id).second) want_dup[b] = 1;
      off[x] = next;
      next += bundles[b][x].size;
    }
    for (size_t x = bundles[b].size(); x--;)
      owner.insert({bundles[b][x].id, Where{b, bundles[b][x].size, off[x]}});
  }
  for (uint32_t b = 0; b < B; b++) {
    if (bdup[b] != want_dup[b]) die(what, -100 - (long)b);
    checks++;
  }
  uint64_t filled = 0;
  for (uint64_t s = 0; s < slots; s++) filled += table[s] != zcgc::kEmpty;
  if (filled != owner.size()) die(what, -1);
  // findChunk for every record
  for (uint32_t b = 0; b < B; b++)
    for (const Rec& rec : bundles[b]) {
      uint32_t steps = 0;
      const zcrs::Hit h = zcrs::find(table, mask, idp, bund, offp, szp, id_of(rec.id), &steps);
      const Where& w = owner.at(rec.id);
      if (h.bundle != w.bundle || h.off != w.off || h.size != w.size || !steps || steps > slots) die(what, -2);
      longest = std::max(longest, steps);
      checks++;
    }
  // the resolve
  uint64_t pos = 0;
  for (size_t e = 0; e < entries.size(); e++) {
    uint32_t steps = 0;
    const Ent& in = entries[e];
    const zcrs::Entry r = zcrs::resolve_entry(table, mask, idp, bund, offp, szp, in.kind, id_of(in.id), in.data_off,
                                              in.size, &steps);
    if (steps > slots) die(what, (long)e);
    longest = std::max(longest, steps);
    if (in.kind == zcrs::kKindBytes) {
      if (!r.bytes || r.bundle != zcrs::kNoBundle || r.off != in.data_off || r.size != in.size) die(what, (long)e);
    } else {
      auto it = owner.find(in.id);
      if (r.bytes) die(what, (long)e);
      if (it == owner.end()) {
        if (r.bundle != zcrs::kNoBundle || r.size != 0 || r.off != 0) die(what, (long)e);
      } else if (r.bundle != it->second.bundle || r.off != it->second.off || r.size != it->second.size) {
        die(what, (long)e);
      }
    }
    pos += r.size;
    checks++;
  }
  (void)pos;
  free(ids);
  free(sizes);
  free(bf);
  free(run);
  free(idp);
  free(szp);
  free(offp);
  free(bund);
  free(table);
  free(pairs);
  return longest;
}

static std::vector<Ent> entries_over(const Bundles& bundles, size_t n, size_t strangers) {
  std::vector<Blob> ids;
  for (const auto& b : bundles)
    for (const Rec& r : b) ids.push_back(r.id);
  std::vector<Ent> out;
  for (size_t k = 0; k < n; k++) {
    if (ids.empty() || rnd() % 5 == 0)
      out.push_back(Ent{zcrs::kKindBytes, Blob{}, rnd() % 1000, rnd() % 50});
    else
      out.push_back(Ent{zcrs::kKindChunk, ids[rnd() % ids.size()], 0, 0});
  }
  for (size_t k = 0; k < strangers; k++) out.push_back(Ent{zcrs::kKindChunk, random_blob(), 0, 0});
  return out;
}

static Bundles random_repo(size_t n_records, size_t pool_size, size_t max_records) {
  std::vector<Rec> pool(pool_size);
  for (Rec& r : pool) r = Rec{random_blob(), (uint32_t)(rnd() % 70000)};
  Bundles out;
  size_t left = n_records;
  while (left) {
    const size_t k = std::min<size_t>(rnd() % (max_records + 1), left);
    std::vector<Rec> b;
    for (size_t j = 0; j < k; j++) b.push_back(pool[rnd() % pool.size()]);
    out.push_back(b);
    left -= k;
  }
  return out;
}

int main() {
  // empty inputs
  run_case({}, {}, 0, "empty");
  run_case({}, entries_over({}, 5, 3), 0, "empty index");
  run_case({{}, {}, {}}, entries_over({}, 5, 3), 0, "bundles without records");
  // random repositories: a small pool gives repeats across and inside bundles
  for (size_t n : {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097}) {
    for (size_t pool : {n, n / 2 + 1, n / 8 + 1}) {
      const Bundles repo = random_repo(n, pool, n < 100 ? 9 : 300);
      const std::vector<Ent> ent = entries_over(repo, n, 7);
      run_case(repo, ent, 0, "random");
      // the smallest table that still leaves a free slot
      int bits = 1;
      while ((1ull << bits) <= n) bits++;
      run_case(repo, ent, bits, "random, forced table");
    }
  }
  // bundle shapes
  {
    Bundles repo;
    for (size_t k : {0, 1, 64, 65, 5000, 0, 3}) {
      std::vector<Rec> b;
      for (size_t j = 0; j < k; j++) b.push_back(Rec{random_blob(), (uint32_t)(1 + rnd() % 70000)});
      repo.push_back(b);
    }
    run_case(repo, entries_over(repo, 3000, 9), 0, "bundle shapes");
  }
  // one slot hash, a table of 64 slots, 40 + 8 + foreign ids
  {
    const uint64_t fold = rnd();
    std::vector<Rec> recs;
    for (int k = 0; k < 40; k++) recs.push_back(Rec{blob_with_fold(fold), (uint32_t)(10 + k)});
    for (int k = 0; k < 20; k++) recs.push_back(Rec{random_blob(), 5});
    Bundles repo;
    for (size_t at = 0; at < recs.size(); at += 7)
      repo.push_back(std::vector<Rec>(recs.begin() + at, recs.begin() + std::min(at + 7, recs.size())));
    std::vector<Ent> ent = entries_over(repo, 200, 5);
    for (int k = 0; k < 5; k++) ent.push_back(Ent{zcrs::kKindChunk, blob_with_fold(fold), 0, 0});
    const uint32_t longest = run_case(repo, ent, 6, "one slot hash");
    if (longest < 40) die("one slot hash: longest walk", longest);
  }
  // owners
  {
    const Blob x = random_blob(), y = random_blob(), p = random_blob(), q = random_blob();
    const Bundles repo = {{{p, 11}}, {{q, 3}, {x, 100}}, {{y, 200}}, {{x, 100}}, {{y, 200}}, {{y, 200}, {p, 11}},
                          {{y, 200}}, {{q, 3}, {y, 200}}};
    run_case(repo, entries_over(repo, 50, 2), 0, "owners");
    // twice in a bundle, an earlier bundle owns the id; twice in a bundle nothing uses
    const Bundles dup = {{{x, 9}}, {{q, 4}}, {{x, 9}, {y, 8}, {x, 9}}, {{x, 9}, {q, 4}}, {{p, 7}, {p, 7}}};
    run_case(dup, entries_over(dup, 50, 2), 0, "duplicates");
    run_case(dup, entries_over(dup, 50, 2), 4, "duplicates, forced table");
    // 64-bit offsets, size 0
    const Bundles big = {{{q, 1}}, {{x, 0xffffffffu}, {y, 0xffffffffu}, {p, 0xffffffffu}, {q, 1}}, {{random_blob(), 0}}};
    run_case(big, entries_over(big, 50, 2), 0, "three records of 2^32 - 1");
  }
  printf("ok %ld\n", checks);
  return 0;
}
