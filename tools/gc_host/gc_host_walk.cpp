// The reference's garbage-collection walk on one host core, for tools/gc_rate.py
// to time beside zc_gc_plan on the same input (a measurement aid, not product
// code).  It restates what `zbackup gc` does per id with the containers the
// reference declares: usedChunkSet and overallChunkSet are std::set<ChunkId>
// (backup_restorer.hh:51, backup_collector.hh), overallBundleSet a
// std::set<Bundle::Id> (backup_collector.hh:33); the fresh reindex that
// Writer::add consults is ChunkIndex's hash table keyed by the rolling hash
// (chunk_index.hh), here an unordered_multimap on the same key.
//
//   mark   every used id inserted into usedChunkSet   (restore() with a ChunkSet, per backup)
//   walk   loadIndex -> processChunk per record, finishBundle per bundle,
//          copyUsedChunks -> addChunk per used record of a repacked bundle
//
// Build: g++ -O3 -std=c++17 -shared -fPIC gc_host_walk.cpp -o libgc_host_walk.so
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <set>
#include <unordered_map>

namespace {
struct Id {
  uint8_t b[24];
  bool operator<(const Id& o) const { return memcmp(b, o.b, 24) < 0; }
  bool operator==(const Id& o) const { return memcmp(b, o.b, 24) == 0; }
  uint64_t rolling() const {
    uint64_t r;
    memcpy(&r, b + 16, 8);
    return r;
  }
};
double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
}  // namespace

extern "C" int gc_host_walk(const uint8_t* ids, const uint32_t* sizes, uint64_t n, const uint64_t* bundle_first,
                            const uint8_t* bundle_ids, uint64_t nb, const uint64_t* index_first, uint64_t ni,
                            const uint8_t* used, uint64_t nu, uint32_t flags, uint64_t max_payload, double* mark_ms,
                            double* walk_ms, uint64_t* counts) {
  (void)n;
  const bool deep = flags & 1, repack = flags & 2;
  const Id* id = (const Id*)ids;
  const Id* bid = (const Id*)bundle_ids;
  auto t = std::chrono::steady_clock::now();
  std::set<Id> used_set;
  for (uint64_t u = 0; u < nu; u++) used_set.insert(((const Id*)used)[u]);
  *mark_ms = ms_since(t);

  t = std::chrono::steady_clock::now();
  std::set<Id> overall_chunks, overall_bundles;
  std::unordered_multimap<uint64_t, Id> reindex;
  uint64_t counted = 0, counted_used = 0, n_copy = 0, n_new = 0, removed = 0;
  for (uint64_t i = 0; i < ni; i++) {
    bool open = false;
    uint64_t payload = 0;
    for (uint64_t b = index_first[i]; b < index_first[i + 1]; b++) {
      uint64_t total = 0, nused = 0;
      for (uint64_t r = bundle_first[b + 1]; r-- > bundle_first[b];) {
        if (deep && !overall_chunks.insert(id[r]).second) continue;
        total++;
        if (used_set.find(id[r]) != used_set.end()) nused++;
      }
      counted += total;
      counted_used += nused;
      bool copies = false;
      if (nused == 0 && total != 0)
        removed++;
      else if (nused < total || repack)
        copies = true;
      else if (deep && total == 0)
        removed += overall_bundles.insert(bid[b]).second;
      else if (deep)
        overall_bundles.insert(bid[b]);
      if (!copies) continue;
      for (uint64_t r = bundle_first[b + 1]; r-- > bundle_first[b];) {
        if (used_set.find(id[r]) == used_set.end()) continue;
        bool have = false;
        auto range = reindex.equal_range(id[r].rolling());
        for (auto it = range.first; it != range.second && !have; ++it) have = it->second == id[r];
        if (have) continue;
        reindex.emplace(id[r].rolling(), id[r]);
        if (!open) {
          open = true;
          payload = 0;
          n_new++;
        }
        if (payload + sizes[r] > max_payload) {
          payload = 0;
          n_new++;
        }
        payload += sizes[r];
        n_copy++;
      }
    }
  }
  *walk_ms = ms_since(t);
  counts[0] = counted;
  counts[1] = counted_used;
  counts[2] = n_copy;
  counts[3] = n_new;
  counts[4] = removed;
  return 0;
}
