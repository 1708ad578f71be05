// Random-access restore: the search and the clip of one piece of a read, for
// host and device alike (ZC_HD, as zc_gc_core.h and zc_meta_core.h).  The
// kernel of zc_range.hip, the host checks of the zc_range_* calls and the CPU
// unit check (tests/range/range_core_check.cpp) run exactly this code.
//
// What zbackup runs: BackupRestorer::IndexedRestorer::saveData
// (backup_restorer.cc:228-316): an upper_bound over the instructions' stream
// positions, one step back, then a walk forward that copies each
// instruction's overlap with the requested range (its Outputer).
//
// The index.  Entry e -- a chunk_to_emit or a bytes_to_emit, in stream order --
// covers the stream positions [pos[e], pos[e + 1]): pos is the exclusive
// running sum of the sizes, pos[n] the stream's length.  Its bytes lie at
// off[e] of the resident payload slot[e].  An empty entry has pos[e] ==
// pos[e + 1]; of a run of entries with one position the search lands on the
// last, so the empty ones are never visited from the front.
//
// Every loop is bounded before it starts: the search by 64 halvings, the walk
// by the entries left.  Nothing waits on anything.
#pragma once
#include <stdint.h>

#ifndef ZC_HD
#define ZC_HD
#endif

namespace zcrange {

// status bits a piece can raise (the host has checked all of it before; a
// piece that finds one of these copies nothing of the range at fault)
constexpr uint32_t kBadSlot = 1;    // slot[e] >= n_slots
constexpr uint32_t kNoPayload = 2;  // the slot has no resident payload
constexpr uint32_t kBadRange = 4;   // off[e] + the bytes wanted end past the slot's size

struct Index {
  const uint64_t* pos;   // n + 1
  const uint32_t* slot;  // n
  const uint64_t* off;   // n
  uint64_t n;
  const uint64_t* slot_size;  // n_slots
  uint32_t n_slots;
};

// the number of i < n with pos[i] <= x: std::upper_bound's result over pos[0 .. n)
ZC_HD inline uint64_t upper_bound(const uint64_t* pos, uint64_t n, uint64_t x) {
  uint64_t lo = 0, len = n;
  for (int step = 0; step < 64; ++step) {
    if (!len) break;
    const uint64_t half = len >> 1;
    if (pos[lo + half] <= x) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return lo;
}

// the entry whose range holds stream position x (saveData's `--it`); n >= 1 and
// pos[0] == 0, so the bound is at least 1.  For x == pos[n] it is the last entry.
ZC_HD inline uint64_t first_entry(const uint64_t* pos, uint64_t n, uint64_t x) {
  const uint64_t ub = upper_bound(pos, n, x);
  return ub ? ub - 1 : 0;
}

// One piece [p0, p0 + size) of a read, size >= 1, p0 + size <= pos[n].  For
// every entry that overlaps it, sink(slot, source offset in the slot, offset in
// the piece, bytes) is called once, in stream order; the calls tile the piece.
// Returns the status bits raised (0: all of the piece was handed to the sink);
// a range at fault is not handed over and ends the walk.
template <class Sink>
ZC_HD inline uint32_t serve_piece(const Index& ix, uint64_t p0, uint64_t size, Sink& sink) {
  if (!ix.n || !size) return 0;
  const uint64_t p1 = p0 + size;
  const uint64_t e0 = first_entry(ix.pos, ix.n, p0);
  const uint64_t trip = ix.n - e0;  // fixed before the loop
  uint64_t e = e0;
  for (uint64_t k = 0; k < trip; ++k, ++e) {
    const uint64_t a = ix.pos[e];
    if (a >= p1) break;
    const uint64_t b = ix.pos[e + 1];
    // the Outputer's clip, at both ends
    const uint64_t start = a < p0 ? p0 - a : 0;
    const uint64_t end = (b > p1 ? p1 : b) - a;
    if (end <= start) continue;  // an empty entry, or one that ends at p0
    const uint32_t s = ix.slot[e];
    if (s >= ix.n_slots) return kBadSlot;
    const uint64_t o = ix.off[e], cap = ix.slot_size[s];
    if (o > cap || end > cap - o) return kBadRange;
    if (!sink(s, o + start, a + start - p0, end - start)) return kNoPayload;
  }
  return 0;
}

// The distinct slots a read [offset, offset + size) touches, marked in
// seen[0 .. n_slots): the same search and walk, with nothing copied.
ZC_HD inline void mark_slots(const Index& ix, uint64_t offset, uint64_t size, uint8_t* seen) {
  if (!ix.n || !size) return;
  const uint64_t p1 = offset + size;
  const uint64_t e0 = first_entry(ix.pos, ix.n, offset);
  const uint64_t trip = ix.n - e0;
  uint64_t e = e0;
  for (uint64_t k = 0; k < trip; ++k, ++e) {
    if (ix.pos[e] >= p1) break;
    if (ix.pos[e + 1] > ix.pos[e] && ix.pos[e + 1] > offset && ix.slot[e] < ix.n_slots) seen[ix.slot[e]] = 1;
  }
}

}  // namespace zcrange
