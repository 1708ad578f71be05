// The exact chunk-id table of garbage collection, for host and device alike
// (ZC_HD, as zc_aes_core.h and zc_lzo_dec.h): the slot hash, the 24-byte
// compare and the insert / lookup steps the kernels of zc_gc.hip run.  The CPU
// unit check (tests/gc/gc_core_check.cpp) runs exactly this code against
// std::set.
//
// What zbackup runs: BundleCollector's usedChunkSet / overallChunkSet lookups
// (backup_collector.cc:51-67,129-144) and ChunkIndex::addChunk on the fresh
// reindex (chunk_index.cc:163-202), one ordered-container lookup per id.
//
// Layout.  An id is ChunkId::toBlob's 24 bytes (chunk_id.cc:19-27), kept packed
// at 24-byte stride and read as three 8-byte words: a 24-byte stride keeps
// every id 8-byte aligned, so no repacking pass and no padding bytes cross the
// bus; a gathered id touches one or two 64-byte lines either way.  The table
// is open addressing over 32-bit slots, linear probing, capacity a power of
// two.  A slot holds the *position* of the record that owns it (kEmpty: none),
// never a key: keys are compared by reading the owner's id.  A slot's id never
// changes once set; its position only falls (insert keeps the minimum over
// equal ids), so the final table does not depend on who came first.
//
// Every loop is bounded by the capacity the host fixed; nothing waits on
// another thread: a lost CAS hands back the occupant, which is compared once.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcgc {

constexpr uint32_t kEmpty = 0xffffffffu;
constexpr uint32_t kIdWords = 3;  // 24 bytes

struct Id {
  uint64_t w[kIdWords];
};

// id number p of a packed array (8-byte aligned)
ZC_HD inline Id load_id(const uint64_t* ids, uint64_t p) {
  const uint64_t* q = ids + p * kIdWords;
  Id v;
  v.w[0] = q[0];
  v.w[1] = q[1];
  v.w[2] = q[2];
  return v;
}

ZC_HD inline bool id_equal(const Id& a, const Id& b) {
  return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2])) == 0;
}

ZC_HD inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// All 24 bytes folded to one word, then a 64-bit finalizer (the multiply /
// xor-shift avalanche of MurmurHash3's fmix64).  The fold is a plain xor of
// rotations, so the check program can build ids that share a hash.
ZC_HD inline uint64_t id_fold(const Id& v) { return v.w[0] ^ rotl64(v.w[1], 21) ^ rotl64(v.w[2], 42); }
ZC_HD inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
// the slot an id starts probing at (mask = capacity - 1)
ZC_HD inline uint64_t slot_hash(const Id& v, uint64_t mask) { return (mix64(id_fold(v)) >> 20) & mask; }

// The two read-modify-write steps on a slot.  On the device they are the
// hardware's 32-bit atomics; the host check is single-threaded.
ZC_HD inline uint32_t slot_cas(uint32_t* slot, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(slot, expect, v);
#else
  const uint32_t old = *slot;
  if (old == expect) *slot = v;
  return old;
#endif
}
ZC_HD inline void slot_min(uint32_t* slot, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(slot, v);
#else
  if (v < *slot) *slot = v;
#endif
}

// Insert position p (its id: ids[p]) into table[0 .. mask].  An empty slot is
// taken with one CAS; a slot whose owner has the same id keeps the smaller
// position.  Returns the slots visited (>= 1), or 0 when the bounded walk found
// neither (a table with no free slot: the host never makes one).  A table has
// at most 2^33 slots, and a walk that long is never reported exactly.
ZC_HD inline uint32_t insert(uint32_t* table, uint64_t mask, const uint64_t* ids, uint32_t p) {
  const Id me = load_id(ids, p);
  uint64_t s = slot_hash(me, mask);
  for (uint64_t step = 0; step <= mask; step++) {
    // the CAS is the read: it hands back the occupant when the slot is taken,
    // whether it was taken before or in this instant by another lane
    const uint32_t owner = slot_cas(&table[s], kEmpty, p);
    if (owner == kEmpty) return (uint32_t)step + 1;
    if (owner == p || id_equal(load_id(ids, owner), me)) {
      slot_min(&table[s], p);
      return (uint32_t)step + 1;
    }
    s = (s + 1) & mask;
  }
  return 0;
}

// The position the table holds for id `key` (the smallest inserted position
// with that id once all inserts are done), or kEmpty.  *steps: slots visited.
ZC_HD inline uint32_t lookup(const uint32_t* table, uint64_t mask, const uint64_t* ids, const Id& key,
                             uint32_t* steps) {
  uint64_t s = slot_hash(key, mask);
  for (uint64_t step = 0; step <= mask; step++) {
    const uint32_t owner = table[s];
    if (owner == kEmpty) {
      *steps = (uint32_t)step + 1;
      return kEmpty;
    }
    if (id_equal(load_id(ids, owner), key)) {
      *steps = (uint32_t)step + 1;
      return owner;
    }
    s = (s + 1) & mask;
  }
  *steps = mask < 0xffffffffull ? (uint32_t)mask + 1 : 0xffffffffu;
  return kEmpty;
}

// Table capacity for n ids: the power of two >= 2 n (at least 2 slots), or
// 2^test_bits when that is smaller and still leaves one free slot (n < 2^bits).
ZC_HD inline uint64_t capacity_for(uint64_t n, int test_bits) {
  uint64_t cap = 2;
  while (cap < 2 * n) cap <<= 1;
  if (test_bits >= 1 && test_bits <= 32) {
    const uint64_t forced = 1ull << test_bits;
    if (forced < cap && n < forced) cap = forced;
  }
  return cap;
}

}  // namespace zcgc
