// The resident chunk index's steps, for host and device alike (ZC_HD, as
// zc_gc_core.h, whose id table this builds on unchanged): where a processing
// position lies, the (id, bundle) table that finds a bundle holding one id
// twice, the owner lookup, and the per-entry step of a resolve.  The CPU unit
// check (tests/resolve/resolve_core_check.cpp) runs exactly this code against
// std::map / std::set.
//
// What zbackup runs: ChunkIndex::findChunk (chunk_index.cc:119-161) over the
// table loadIndex / registerNewChunkId filled (chunk_index.cc:26-79,163-182),
// then Bundle::Reader's map of one bundle (bundle.cc:220-251).
//
// Layout.  Everything is kept by *processing position* (zc_gc.hip): bundle b
// owns positions [bf[b], bf[b+1]), its records reversed inside, so the smallest
// position of an id is registerNewChunkId's first registration.  Per position:
// the id (24 bytes, packed), the record's size, its payload offset in its
// bundle (the sum of the sizes in front of it in BundleInfo order, 64 bits) and
// its bundle.  The id table is zcgc's; the pair table has the same shape, but a
// slot's key is (id, bundle) of the position it holds.
#pragma once
#include <stdint.h>

#include "zc_gc_core.h"

namespace zcrs {

constexpr uint32_t kNoBundle = 0xffffffffu;  // a lookup that found no owner
constexpr uint32_t kKindChunk = 0, kKindBytes = 1;  // ZC_INSTR_CHUNK / ZC_INSTR_BYTES

// the bundle whose range holds position (or record) p: the last b with
// bf[b] <= p.  nb >= 1 and bf[nb] > p, so the answer is in [0, nb).
ZC_HD inline uint32_t bundle_of(const uint64_t* bf, uint32_t nb, uint64_t p) {
  uint32_t lo = 0, hi = nb;
  for (int it = 0; it < 33 && hi - lo > 1; it++) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bf[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// the record at position p of bundle b, and back (the map is its own inverse)
ZC_HD inline uint64_t record_of(const uint64_t* bf, uint32_t b, uint64_t p) { return bf[b] + (bf[b + 1] - 1 - p); }

// where an (id, bundle) pair starts probing
ZC_HD inline uint64_t pair_hash(const zcgc::Id& v, uint32_t bundle, uint64_t mask) {
  return (zcgc::mix64(zcgc::id_fold(v) ^ ((uint64_t)bundle + 1) * 0x9E3779B97F4A7C15ull) >> 20) & mask;
}

// Insert position p under the key (idp[p], bund[p]) into pairs[0 .. mask].
// *twice is set when another position with the same key is met: the bundle
// holds the id twice (exDuplicateChunks, bundle.cc:229-230).  Two positions
// with one key walk the same slots, none of which is ever emptied, so the later
// CAS of the two meets the earlier whoever it was: the answer is exact, and the
// same for every bundle whatever other bundles hold the id.  Returns the slots
// visited, or 0 when the bounded walk found no free slot.
ZC_HD inline uint32_t insert_pair(uint32_t* pairs, uint64_t mask, const uint64_t* idp, const uint32_t* bund,
                                  uint32_t p, bool* twice) {
  const zcgc::Id me = zcgc::load_id(idp, p);
  const uint32_t b = bund[p];
  uint64_t s = pair_hash(me, b, mask);
  for (uint64_t step = 0; step <= mask; step++) {
    const uint32_t owner = zcgc::slot_cas(&pairs[s], zcgc::kEmpty, p);
    if (owner == zcgc::kEmpty) return (uint32_t)step + 1;
    if (owner != p && bund[owner] == b && zcgc::id_equal(zcgc::load_id(idp, owner), me)) {
      *twice = true;
      return (uint32_t)step + 1;
    }
    s = (s + 1) & mask;
  }
  return 0;
}

// findChunk's answer for one id
struct Hit {
  uint32_t bundle;  // kNoBundle: the index has no such id
  uint32_t size;
  uint64_t off;     // offset in the bundle's payload
};
ZC_HD inline Hit find(const uint32_t* table, uint64_t mask, const uint64_t* idp, const uint32_t* bund,
                      const uint64_t* offp, const uint32_t* szp, const zcgc::Id& key, uint32_t* steps) {
  Hit h;
  const uint32_t f = zcgc::lookup(table, mask, idp, key, steps);
  if (f == zcgc::kEmpty) {
    h.bundle = kNoBundle;
    h.size = 0;
    h.off = 0;
    return h;
  }
  h.bundle = bund[f];
  h.size = szp[f];
  h.off = offp[f];
  return h;
}

// One entry of a BackupInstruction stream, resolved: a CHUNK entry is its
// owner's (bundle, off, size), a BYTES entry lies in the stream itself.
struct Entry {
  uint32_t bundle;  // CHUNK: the owner's bundle or kNoBundle; BYTES: kNoBundle
  uint32_t bytes;   // 1: a BYTES entry (its slot is the instruction stream's)
  uint64_t off, size;
};
ZC_HD inline Entry resolve_entry(const uint32_t* table, uint64_t mask, const uint64_t* idp, const uint32_t* bund,
                                 const uint64_t* offp, const uint32_t* szp, uint32_t kind, const zcgc::Id& id,
                                 uint64_t data_off, uint64_t size, uint32_t* steps) {
  Entry e;
  if (kind == kKindBytes) {
    *steps = 0;
    e.bundle = kNoBundle;
    e.bytes = 1;
    e.off = data_off;
    e.size = size;
    return e;
  }
  const Hit h = find(table, mask, idp, bund, offp, szp, id, steps);
  e.bundle = h.bundle;
  e.bytes = 0;
  e.off = h.off;
  e.size = h.size;
  return e;
}

}  // namespace zcrs
