// zc_gc.hip -- garbage collection: mark the used chunks and plan the repack on
// the GPU.  `zbackup gc` (zutils.cc:450-505) walks every chunk record of every
// index file through BundleCollector (backup_collector.cc:17-144): a lookup in
// usedChunkSet per record, one in overallChunkSet under --gc-deep, and one in
// the fresh reindex per copied chunk (chunk_index.cc:185-202).  Here those
// lookups are an exact table of the 24-byte ids in HBM (zc_gc_core.h).
//
// Everything on the device works in *processing positions*: the order the
// reference visits records in (a bundle's records from the last to the first).
// Bundle b owns the same range [bundle_first[b], bundle_first[b+1]) of
// positions as of records, reversed inside.
//
//   phase 1   zc_gc_permute   ids, sizes -> position order; each position's record and bundle
//             zc_gc_insert    every position into the table, equal ids keep the smallest
//             zc_gc_mark      every used id looked up; mark[first position of the id] = 1
//             zc_gc_flags     per position: COUNTED (deep: it is the id's first position),
//                             USED (its id's mark); a size that differs from the first's
//             zc_gc_counts    per bundle (a wave each): COUNTED, and COUNTED & USED
//   host      the per-bundle actions in bundle order (finishBundle needs overallBundleSet)
//   phase 2   zc_gc_insert_cand  the USED positions of REPACK bundles into a fresh table
//             zc_gc_copied       COPIED = the candidate is its id's first; flags out per record
//             zc_gc_tile_sums / zc_gc_tile_scan / zc_gc_compact
//                                the COPIED positions, ascending = copy order, with the
//                                running sum of their sizes
//   host      Writer::add's bundling rule over the copy list, per index file
//
// The outputs are functions of the final tables, and a table's final state
// does not depend on the order of the inserts (zc_gc_core.h), so two calls
// give the same bytes.  Only max_probe (a statistic) depends on the schedule.
//
// Every loop bound below is a count the host computed from validated input;
// every kernel is grid-stride; no kernel waits on another wave or workgroup,
// spins, or ends on a data value; a probe walk ends after `capacity` slots at
// the latest.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <set>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_gc_core.h"

namespace zc {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kTileItems = 4;                    // positions per thread of a compaction tile
constexpr uint32_t kTile = kBlock * kTileItems;       // positions per tile
constexpr uint64_t kCountLimit = 0xffffffffull;       // counts stay below 2^32 - 1

// what the kernels report, one copy on the device
struct GcDev {
  unsigned long long mismatch;  // min over (position << 32 | first position) of a size mismatch
  unsigned long long copy_bytes;
  uint32_t n_copy;
  uint32_t max_probe;
  uint32_t internal;  // bit 0: an insert found no slot; bit 1: a lookup of an inserted id failed
  uint32_t pad;
};

__device__ inline void note_probe(GcDev* dev, uint32_t longest) {
  if (longest) atomicMax(&dev->max_probe, longest);
}

__global__ __launch_bounds__(kBlock) void zc_gc_permute(const uint64_t* __restrict__ ids,
                                                        const uint32_t* __restrict__ sizes,
                                                        const uint64_t* __restrict__ bf, uint32_t nb, uint64_t n,
                                                        uint64_t* __restrict__ idp, uint32_t* __restrict__ szp,
                                                        uint32_t* __restrict__ recp, uint32_t* __restrict__ bund) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    // the bundle whose range holds p: the last b with bf[b] <= p (bf[nb] = n > p)
    uint32_t lo = 0, hi = nb;  // the answer is in [lo, hi)
    for (int it = 0; it < 33 && hi - lo > 1; it++) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (bf[mid] <= p)
        lo = mid;
      else
        hi = mid;
    }
    const uint64_t r = bf[lo] + (bf[lo + 1] - 1 - p);
    const zcgc::Id v = zcgc::load_id(ids, r);
    idp[3 * p] = v.w[0];
    idp[3 * p + 1] = v.w[1];
    idp[3 * p + 2] = v.w[2];
    szp[p] = sizes[r];
    recp[p] = (uint32_t)r;
    bund[p] = lo;
  }
}

__global__ __launch_bounds__(kBlock) void zc_gc_insert(uint32_t* __restrict__ table, uint64_t mask,
                                                       const uint64_t* __restrict__ idp, uint64_t n, GcDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    const uint32_t steps = zcgc::insert(table, mask, idp, (uint32_t)p);
    if (!steps) atomicOr(&dev->internal, 1u);
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

__global__ __launch_bounds__(kBlock) void zc_gc_mark(const uint32_t* __restrict__ table, uint64_t mask,
                                                     const uint64_t* __restrict__ idp,
                                                     const uint64_t* __restrict__ used, uint64_t nu,
                                                     uint8_t* __restrict__ mark, GcDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t u = (uint64_t)blockIdx.x * kBlock + threadIdx.x; u < nu; u += stride) {
    uint32_t steps;
    const uint32_t f = zcgc::lookup(table, mask, idp, zcgc::load_id(used, u), &steps);
    if (f != zcgc::kEmpty) mark[f] = 1;  // every writer stores the same byte
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

__global__ __launch_bounds__(kBlock) void zc_gc_flags(const uint32_t* __restrict__ table, uint64_t mask,
                                                      const uint64_t* __restrict__ idp,
                                                      const uint32_t* __restrict__ szp,
                                                      const uint8_t* __restrict__ mark, uint64_t n, int deep,
                                                      uint8_t* __restrict__ flagp, GcDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    uint32_t steps;
    const uint32_t f = zcgc::lookup(table, mask, idp, zcgc::load_id(idp, p), &steps);
    longest = max(longest, steps);
    if (f == zcgc::kEmpty) {
      atomicOr(&dev->internal, 2u);
      flagp[p] = 0;
      continue;
    }
    if (szp[f] != szp[p]) atomicMin(&dev->mismatch, (unsigned long long)p << 32 | f);
    const uint32_t counted = deep ? (f == (uint32_t)p) : 1u;
    flagp[p] = (uint8_t)(counted * ZC_GC_REC_COUNTED | (mark[f] ? ZC_GC_REC_USED : 0u));
  }
  note_probe(dev, longest);
}

// a wave per bundle: its lanes stride the bundle's positions
__global__ __launch_bounds__(kBlock) void zc_gc_counts(const uint8_t* __restrict__ flagp,
                                                       const uint64_t* __restrict__ bf, uint32_t nb,
                                                       uint32_t* __restrict__ btotal, uint32_t* __restrict__ bused) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t b = (uint64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64; b < nb; b += waves) {
    const uint64_t end = bf[b + 1];
    uint32_t total = 0, used = 0;
    for (uint64_t p = bf[b] + lane; p < end; p += 64) {
      const uint32_t f = flagp[p];
      total += f & 1u;
      used += (f & 3u) == 3u;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      total += __shfl_xor(total, m, 64);
      used += __shfl_xor(used, m, 64);
    }
    if (lane == 0) {
      btotal[b] = total;
      bused[b] = used;
    }
  }
}

__device__ inline bool is_candidate(const uint8_t* flagp, const uint32_t* bund, const uint8_t* action, uint64_t p) {
  return (flagp[p] & ZC_GC_REC_USED) && action[bund[p]] == ZC_GC_ACT_REPACK;
}

__global__ __launch_bounds__(kBlock) void zc_gc_insert_cand(uint32_t* __restrict__ table, uint64_t mask,
                                                            const uint64_t* __restrict__ idp,
                                                            const uint8_t* __restrict__ flagp,
                                                            const uint32_t* __restrict__ bund,
                                                            const uint8_t* __restrict__ action, uint64_t n,
                                                            GcDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    if (!is_candidate(flagp, bund, action, p)) continue;
    const uint32_t steps = zcgc::insert(table, mask, idp, (uint32_t)p);
    if (!steps) atomicOr(&dev->internal, 1u);
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

// COPIED = a candidate that is the first of its id among the candidates; every
// position's final flags go to its record
__global__ __launch_bounds__(kBlock) void zc_gc_copied(const uint32_t* __restrict__ table, uint64_t mask,
                                                       const uint64_t* __restrict__ idp, uint8_t* __restrict__ flagp,
                                                       const uint32_t* __restrict__ bund,
                                                       const uint8_t* __restrict__ action,
                                                       const uint32_t* __restrict__ recp, uint64_t n,
                                                       uint8_t* __restrict__ flagr, GcDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    uint8_t f = flagp[p];
    if (is_candidate(flagp, bund, action, p)) {
      uint32_t steps;
      const uint32_t first = zcgc::lookup(table, mask, idp, zcgc::load_id(idp, p), &steps);
      longest = max(longest, steps);
      if (first == zcgc::kEmpty) atomicOr(&dev->internal, 2u);
      if (first == (uint32_t)p) f |= ZC_GC_REC_COPIED;
      flagp[p] = f;
    }
    flagr[recp[p]] = f;
  }
  note_probe(dev, longest);
}

// exclusive scan of (c, s) over the block's 256 threads; *tc, *ts: the block's sums
__device__ inline void block_scan(uint32_t& c, uint64_t& s, uint32_t* lc, uint64_t* ls, uint32_t* tc, uint64_t* ts) {
  const uint32_t t = threadIdx.x;
  const uint32_t c0 = c;
  const uint64_t s0 = s;
  lc[t] = c;
  ls[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    const uint32_t ac = t >= d ? lc[t - d] : 0;
    const uint64_t as = t >= d ? ls[t - d] : 0;
    __syncthreads();
    lc[t] += ac;
    ls[t] += as;
    __syncthreads();
  }
  c = lc[t] - c0;
  s = ls[t] - s0;
  *tc = lc[kBlock - 1];
  *ts = ls[kBlock - 1];
  __syncthreads();  // the arrays may be reused
}

__global__ __launch_bounds__(kBlock) void zc_gc_tile_sums(const uint8_t* __restrict__ flagp,
                                                          const uint32_t* __restrict__ szp, uint64_t n,
                                                          uint32_t ntiles, uint32_t* __restrict__ tcount,
                                                          uint64_t* __restrict__ tsize) {
  __shared__ uint32_t lc[kBlock];
  __shared__ uint64_t ls[kBlock];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kTile + threadIdx.x * kTileItems;
    uint32_t c = 0;
    uint64_t s = 0;
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n && (flagp[base + k] & ZC_GC_REC_COPIED)) {
        c++;
        s += szp[base + k];
      }
    uint32_t tc;
    uint64_t ts;
    block_scan(c, s, lc, ls, &tc, &ts);
    if (threadIdx.x == 0) {
      tcount[tile] = tc;
      tsize[tile] = ts;
    }
  }
}

// one workgroup: the tiles' sums to exclusive prefixes, 256 at a time
__global__ __launch_bounds__(kBlock) void zc_gc_tile_scan(uint32_t* __restrict__ tcount, uint64_t* __restrict__ tsize,
                                                          uint32_t ntiles, GcDev* dev) {
  __shared__ uint32_t lc[kBlock];
  __shared__ uint64_t ls[kBlock];
  uint32_t carry_c = 0;
  uint64_t carry_s = 0;
  for (uint32_t base = 0; base < ntiles; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    uint32_t c = i < ntiles ? tcount[i] : 0;
    uint64_t s = i < ntiles ? tsize[i] : 0;
    uint32_t tc;
    uint64_t ts;
    block_scan(c, s, lc, ls, &tc, &ts);
    if (i < ntiles) {
      tcount[i] = carry_c + c;
      tsize[i] = carry_s + s;
    }
    carry_c += tc;
    carry_s += ts;
  }
  if (threadIdx.x == 0) {
    dev->n_copy = carry_c;
    dev->copy_bytes = carry_s;
  }
}

__global__ __launch_bounds__(kBlock) void zc_gc_compact(const uint8_t* __restrict__ flagp,
                                                        const uint32_t* __restrict__ szp,
                                                        const uint32_t* __restrict__ recp, uint64_t n,
                                                        uint32_t ntiles, const uint32_t* __restrict__ tcount,
                                                        const uint64_t* __restrict__ tsize, uint64_t cap,
                                                        uint32_t* __restrict__ copy, uint64_t* __restrict__ run) {
  __shared__ uint32_t lc[kBlock];
  __shared__ uint64_t ls[kBlock];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kTile + threadIdx.x * kTileItems;
    uint32_t c = 0;
    uint64_t s = 0;
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n && (flagp[base + k] & ZC_GC_REC_COPIED)) {
        c++;
        s += szp[base + k];
      }
    uint32_t tc;
    uint64_t ts;
    block_scan(c, s, lc, ls, &tc, &ts);
    uint64_t at = (uint64_t)tcount[tile] + c;
    uint64_t bytes = tsize[tile] + s;
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n && (flagp[base + k] & ZC_GC_REC_COPIED)) {
        if (at < cap) {  // cap = the scratch list's room, n
          copy[at] = recp[base + k];
          run[at] = bytes;
        }
        at++;
        bytes += szp[base + k];
      }
  }
}

template <class T>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = std::max<size_t>(n, 1);
    return hipSuccess;
  }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};

// pinned host memory: the read-backs land here at the link's rate, without the
// runtime pinning and unpinning the caller's pages around every copy
template <class T>
struct Pinned {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = std::max<size_t>(n, 1);
    return hipSuccess;
  }
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
};

int arg_error(std::string& err, const std::string& msg) {
  err = msg;
  return ZC_ERR_ARG;
}
int hip_error(std::string& err, hipError_t e, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  err = hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZC_ERR_NOMEM : ZC_ERR_HIP;
}
#define GCK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

struct Id24 {
  uint8_t b[24];
  bool operator<(const Id24& o) const { return memcmp(b, o.b, 24) < 0; }
};

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

}  // namespace

struct GcScratch {
  Buf<uint64_t> ids, idp, used, bf, tsize, run;
  Buf<uint32_t> sizes, szp, recp, bund, table, btotal, bused, tcount, copy;
  Buf<uint8_t> mark, flagp, flagr, action;
  Buf<GcDev> dev;
  hipEvent_t ev[6] = {};
  int cus = 0;
  GcTimes times{};
  Pinned<uint32_t> h_btotal, h_bused, h_copy;
  Pinned<uint64_t> h_run;
  Pinned<uint8_t> h_flags;
  // host lists of the last call, kept for their capacity (fresh pages per call
  // cost more than the bundling rule itself at millions of copies)
  std::vector<uint32_t> h_cbundle, h_of, h_nb_index;
  std::vector<uint64_t> h_coff, h_sz, h_nb_size;
  ~GcScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

GcScratch* gc_scratch_new() { return new GcScratch(); }
void gc_scratch_free(GcScratch* s) { delete s; }
const GcTimes* gc_times(const GcScratch* s) { return &s->times; }

int gc_validate(const zc_gc_input* in, const zc_gc_output* out, std::string& err) {
  if (!in || !out) return arg_error(err, "null input or output");
  const uint64_t N = in->n_records, B = in->n_bundles, I = in->n_indexes, U = in->n_used;
  char msg[200];
  if (N >= kCountLimit || U >= kCountLimit || B >= kCountLimit || I >= kCountLimit) {
    snprintf(msg, sizeof msg, "%llu records, %llu used ids, %llu bundles, %llu index files: each must stay below 2^32 - 1",
             (unsigned long long)N, (unsigned long long)U, (unsigned long long)B, (unsigned long long)I);
    return arg_error(err, msg);
  }
  if (in->flags & ~(uint32_t)(ZC_GC_DEEP | ZC_GC_REPACK | ZC_GC_CONCAT)) return arg_error(err, "unknown flag");
  if ((N && (!in->ids || !in->sizes)) || (B && (!in->bundle_first || !in->bundle_ids)) ||
      (I && !in->index_first) || (U && !in->used))
    return arg_error(err, "null input array");
  if ((N && !out->record_flags) || (B && (!out->bundle_total || !out->bundle_used || !out->bundle_action)) ||
      (I && !out->indexes) || (out->copy_cap && (!out->copy || !out->copy_bundle || !out->copy_off)) ||
      (out->new_bundle_cap && (!out->new_bundle_index || !out->new_bundle_size)))
    return arg_error(err, "null output array");
  // a NULL range array of no entries stands for {0}
  auto ranges = [&](const char* name, const uint64_t* first, uint64_t cnt, uint64_t end, const char* what) {
    if (!first) {
      if (end == 0) return true;
      snprintf(msg, sizeof msg, "%s is empty but there are %llu %s", name, (unsigned long long)end, what);
      return false;
    }
    if (first[0] != 0) {
      snprintf(msg, sizeof msg, "%s[0] = %llu, not 0", name, (unsigned long long)first[0]);
      return false;
    }
    for (uint64_t k = 0; k < cnt; k++)
      if (first[k + 1] < first[k]) {
        snprintf(msg, sizeof msg, "%s[%llu] = %llu is below %s[%llu] = %llu", name, (unsigned long long)(k + 1),
                 (unsigned long long)first[k + 1], name, (unsigned long long)k, (unsigned long long)first[k]);
        return false;
      }
    if (first[cnt] != end) {
      snprintf(msg, sizeof msg, "%s ends at %llu, there are %llu %s", name, (unsigned long long)first[cnt],
               (unsigned long long)end, what);
      return false;
    }
    return true;
  };
  if (!ranges("bundle_first", in->bundle_first, B, N, "records")) return arg_error(err, msg);
  if (!ranges("index_first", in->index_first, I, B, "bundles")) return arg_error(err, msg);
  return ZC_OK;
}

namespace {

int grid_for(const GcScratch* s, uint64_t items) {
  const uint64_t blocks = (items + kBlock - 1) / kBlock;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * 16));
}

// finishBundle (backup_collector.cc:69-127) for every bundle in order, and
// finishIndex's bookkeeping (lines 24-42)
void decide(const zc_gc_input* in, const uint32_t* btotal, const uint32_t* bused, zc_gc_output* out) {
  const bool deep = in->flags & ZC_GC_DEEP, repack = in->flags & ZC_GC_REPACK, concat = in->flags & ZC_GC_CONCAT;
  std::set<Id24> seen;  // overallBundleSet
  for (uint64_t i = 0; i < in->n_indexes; i++) {
    zc_gc_index x{};
    for (uint64_t b = in->index_first[i]; b < in->index_first[i + 1]; b++) {
      const uint32_t total = btotal[b], used = bused[b];
      out->bundle_total[b] = total;
      out->bundle_used[b] = used;
      x.total += total;
      x.used += used;
      uint8_t act;
      if (used == 0 && total != 0) {
        act = ZC_GC_ACT_REMOVE;
      } else if (used < total || repack) {
        act = ZC_GC_ACT_REPACK;
      } else {
        Id24 id;
        memcpy(id.b, in->bundle_ids + 24 * b, 24);
        if (deep && total == 0)
          act = seen.insert(id).second ? ZC_GC_ACT_REMOVE : ZC_GC_ACT_DROP_RECORD;
        else {
          if (deep) seen.insert(id);
          act = ZC_GC_ACT_KEEP;
        }
      }
      out->bundle_action[b] = act;
      if (act == ZC_GC_ACT_KEEP)
        x.kept++;
      else
        x.modified = 1;
      if (act == ZC_GC_ACT_REMOVE) x.removed++;
      if (act == ZC_GC_ACT_REPACK) x.modified_bundles++;
    }
    x.necessary = x.used > 0;  // processChunk sets it with usedChunks++ (line 65)
    x.unlink = x.modified || (deep && !x.necessary) || concat;
    out->indexes[i] = x;
  }
}

}  // namespace

int gc_plan(GcScratch* s, const zc_gc_input* in, zc_gc_output* out, hipStream_t st, std::string& err) {
  const uint64_t N = in->n_records, B = in->n_bundles, U = in->n_used;
  const bool deep = in->flags & ZC_GC_DEEP;
  out->n_copy = 0;
  out->n_new_bundles = 0;
  s->times = GcTimes{};
  if (!s->cus) {
    int dev = 0, cus = 0;
    GCK(hipGetDevice(&dev));
    GCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    s->cus = std::max(cus, 1);
    for (hipEvent_t& e : s->ev) GCK(hipEventCreate(&e));
  }
  const char* tb = getenv("ZC_TEST_GC_BITS");
  const uint64_t slots = zcgc::capacity_for(N, tb ? atoi(tb) : 0);
  const uint64_t mask = slots - 1;
  s->times.table_slots = slots;

  GCK(s->h_btotal.ensure(B));
  GCK(s->h_bused.ensure(B));
  uint32_t *btotal = s->h_btotal.p, *bused = s->h_bused.p;
  memset(btotal, 0, 4 * B);
  memset(bused, 0, 4 * B);
  GcDev h{};
  h.mismatch = ~0ull;
  auto t0 = Clock::now();
  auto t_host0 = t0, t_host1 = t0;
  if (N) {
    // ---- phase 1 ----
    GCK(s->ids.ensure(3 * N));
    GCK(s->idp.ensure(3 * N));
    GCK(s->used.ensure(3 * U));
    GCK(s->bf.ensure(B + 1));
    GCK(s->sizes.ensure(N));
    GCK(s->szp.ensure(N));
    GCK(s->recp.ensure(N));
    GCK(s->bund.ensure(N));
    GCK(s->table.ensure(slots));
    GCK(s->btotal.ensure(B));
    GCK(s->bused.ensure(B));
    GCK(s->mark.ensure(N));
    GCK(s->flagp.ensure(N));
    GCK(s->flagr.ensure(N));
    GCK(s->action.ensure(B));
    GCK(s->dev.ensure(1));
    t0 = Clock::now();  // the buffers are made once and kept
    GCK(hipEventRecord(s->ev[0], st));
    GCK(hipMemcpyAsync(s->ids.p, in->ids, 24 * N, hipMemcpyHostToDevice, st));
    GCK(hipMemcpyAsync(s->sizes.p, in->sizes, 4 * N, hipMemcpyHostToDevice, st));
    GCK(hipMemcpyAsync(s->bf.p, in->bundle_first, 8 * (B + 1), hipMemcpyHostToDevice, st));
    if (U) GCK(hipMemcpyAsync(s->used.p, in->used, 24 * U, hipMemcpyHostToDevice, st));
    GCK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
    GCK(hipMemsetAsync(s->table.p, 0xff, 4 * slots, st));
    GCK(hipMemsetAsync(s->mark.p, 0, N, st));
    GCK(hipEventRecord(s->ev[1], st));
    const int gn = grid_for(s, N);
    zc_gc_permute<<<gn, kBlock, 0, st>>>(s->ids.p, s->sizes.p, s->bf.p, (uint32_t)B, N, s->idp.p, s->szp.p, s->recp.p,
                                         s->bund.p);
    zc_gc_insert<<<gn, kBlock, 0, st>>>(s->table.p, mask, s->idp.p, N, s->dev.p);
    GCK(hipEventRecord(s->ev[2], st));
    if (U) zc_gc_mark<<<grid_for(s, U), kBlock, 0, st>>>(s->table.p, mask, s->idp.p, s->used.p, U, s->mark.p, s->dev.p);
    zc_gc_flags<<<gn, kBlock, 0, st>>>(s->table.p, mask, s->idp.p, s->szp.p, s->mark.p, N, deep ? 1 : 0, s->flagp.p,
                                       s->dev.p);
    zc_gc_counts<<<grid_for(s, B * 64), kBlock, 0, st>>>(s->flagp.p, s->bf.p, (uint32_t)B, s->btotal.p, s->bused.p);
    GCK(hipGetLastError());
    GCK(hipEventRecord(s->ev[3], st));
    GCK(hipMemcpyAsync(btotal, s->btotal.p, 4 * B, hipMemcpyDeviceToHost, st));
    GCK(hipMemcpyAsync(bused, s->bused.p, 4 * B, hipMemcpyDeviceToHost, st));
    GCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
    GCK(hipStreamSynchronize(st));
    t_host0 = Clock::now();
    float ms = 0;
    GCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.upload_ms = ms;
    GCK(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
    s->times.build_ms = ms;
    GCK(hipEventElapsedTime(&ms, s->ev[2], s->ev[3]));
    s->times.probe_ms = ms;
    s->times.readback_ms = ms_between(t0, t_host0) - s->times.upload_ms - s->times.build_ms - s->times.probe_ms;
    s->times.max_probe = h.max_probe;
    if (h.internal) {
      err = "the id table lost an entry (internal error)";
      return ZC_ERR_STATE;
    }
    if (h.mismatch != ~0ull) {
      // positions back to records: the same bundle range, reversed
      auto record_of = [&](uint64_t p) {
        const uint64_t* bf = in->bundle_first;
        const uint64_t b = (uint64_t)(std::upper_bound(bf, bf + B + 1, p) - bf) - 1;
        return bf[b] + (bf[b + 1] - 1 - p);
      };
      const uint64_t r = record_of(h.mismatch >> 32), f = record_of(h.mismatch & 0xffffffffull);
      char msg[200];
      snprintf(msg, sizeof msg,
               "records %llu (size %u) and %llu (size %u) have the same chunk id and different sizes",
               (unsigned long long)f, in->sizes[f], (unsigned long long)r, in->sizes[r]);
      return arg_error(err, msg);
    }
  } else {
    t_host0 = Clock::now();
  }

  // ---- the host's decisions ----
  decide(in, btotal, bused, out);
  bool any_repack = false;
  for (uint64_t b = 0; b < B && !any_repack; b++) any_repack = out->bundle_action[b] == ZC_GC_ACT_REPACK;
  t_host1 = Clock::now();
  s->times.host_ms = ms_between(t_host0, t_host1);

  // ---- phase 2 ----
  uint64_t M = 0;
  const uint32_t* copy = nullptr;
  const uint64_t* run = nullptr;
  if (N) {
    const int gn = grid_for(s, N);
    const uint32_t ntiles = (uint32_t)((N + kTile - 1) / kTile);
    GCK(s->tcount.ensure(ntiles));
    GCK(s->tsize.ensure(ntiles));
    GCK(s->copy.ensure(N));
    GCK(s->run.ensure(N));
    GCK(hipMemcpyAsync(s->action.p, out->bundle_action, B, hipMemcpyHostToDevice, st));
    GCK(hipEventRecord(s->ev[4], st));
    if (any_repack) {
      GCK(hipMemsetAsync(s->table.p, 0xff, 4 * slots, st));
      zc_gc_insert_cand<<<gn, kBlock, 0, st>>>(s->table.p, mask, s->idp.p, s->flagp.p, s->bund.p, s->action.p, N,
                                               s->dev.p);
    }
    zc_gc_copied<<<gn, kBlock, 0, st>>>(s->table.p, mask, s->idp.p, s->flagp.p, s->bund.p, s->action.p, s->recp.p, N,
                                        s->flagr.p, s->dev.p);
    if (any_repack) {
      const int gt = (int)std::min<uint64_t>(ntiles, (uint64_t)s->cus * 16);
      zc_gc_tile_sums<<<gt, kBlock, 0, st>>>(s->flagp.p, s->szp.p, N, ntiles, s->tcount.p, s->tsize.p);
      zc_gc_tile_scan<<<1, kBlock, 0, st>>>(s->tcount.p, s->tsize.p, ntiles, s->dev.p);
      zc_gc_compact<<<gt, kBlock, 0, st>>>(s->flagp.p, s->szp.p, s->recp.p, N, ntiles, s->tcount.p, s->tsize.p, N,
                                           s->copy.p, s->run.p);
    }
    GCK(hipGetLastError());
    GCK(hipEventRecord(s->ev[5], st));
    GCK(s->h_flags.ensure(N));
    GCK(hipMemcpyAsync(s->h_flags.p, s->flagr.p, N, hipMemcpyDeviceToHost, st));
    GCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
    GCK(hipStreamSynchronize(st));
    s->times.max_probe = h.max_probe;
    if (h.internal) {
      err = "the candidate table lost an entry (internal error)";
      return ZC_ERR_STATE;
    }
    M = any_repack ? h.n_copy : 0;
    if (M > N) {
      err = "the copy list is longer than the input (internal error)";
      return ZC_ERR_STATE;
    }
    GCK(s->h_copy.ensure(M));
    GCK(s->h_run.ensure(M));
    if (M) {
      GCK(hipMemcpyAsync(s->h_copy.p, s->copy.p, 4 * M, hipMemcpyDeviceToHost, st));
      GCK(hipMemcpyAsync(s->h_run.p, s->run.p, 8 * M, hipMemcpyDeviceToHost, st));
      GCK(hipStreamSynchronize(st));
    }
    copy = s->h_copy.p;
    run = s->h_run.p;
    memcpy(out->record_flags, s->h_flags.p, N);
    float ms = 0;
    GCK(hipEventElapsedTime(&ms, s->ev[4], s->ev[5]));
    s->times.copy_ms = ms;
    s->times.readback_ms += ms_between(t_host1, Clock::now()) - ms;
  }

  // ---- Writer::add's bundling rule over the copy list, a fresh bundle per index file ----
  const auto t_rule = Clock::now();
  out->n_copy = M;
  std::vector<uint32_t>&cbundle = s->h_cbundle, &nb_index = s->h_nb_index, &of = s->h_of;
  std::vector<uint64_t>&coff = s->h_coff, &nb_size = s->h_nb_size, &sz = s->h_sz;
  cbundle.resize(M);
  coff.resize(M);
  nb_index.clear();
  nb_size.clear();
  {
    uint64_t b = 0, i = 0, k = 0;
    while (k < M) {
      // the index file of entry k (records and positions share their bundle's range)
      while (in->bundle_first[b + 1] <= copy[k]) b++;
      while (in->index_first[i + 1] <= b) i++;
      const uint64_t rec_end = in->bundle_first[in->index_first[i + 1]];
      uint64_t k1 = k;
      sz.clear();
      while (k1 < M && copy[k1] < rec_end) sz.push_back(in->sizes[copy[k1++]]);
      of.resize(sz.size());
      size_t nb = 0;
      if (zc_bundle_plan(sz.data(), sz.size(), in->max_payload, of.data(), &nb) != ZC_OK) {
        err = "zc_bundle_plan failed (internal error)";
        return ZC_ERR_STATE;
      }
      const size_t base = nb_index.size();
      nb_index.resize(base + nb, (uint32_t)i);
      nb_size.resize(base + nb, 0);
      uint64_t start = run[k];  // the running size where the entry's bundle began
      for (uint64_t j = k; j < k1; j++) {
        if (j > k && of[j - k] != of[j - k - 1]) start = run[j];
        cbundle[j] = (uint32_t)(base + of[j - k]);
        coff[j] = run[j] - start;
        nb_size[base + of[j - k]] += sz[j - k];
      }
      k = k1;
    }
  }
  out->n_new_bundles = nb_index.size();
  if (M > out->copy_cap || nb_index.size() > out->new_bundle_cap) {
    char msg[200];
    snprintf(msg, sizeof msg, "%llu copy entries in %llu new bundles, room for %llu and %llu",
             (unsigned long long)M, (unsigned long long)nb_index.size(), (unsigned long long)out->copy_cap,
             (unsigned long long)out->new_bundle_cap);
    return arg_error(err, msg);
  }
  if (M) {
    memcpy(out->copy, copy, 4 * M);
    memcpy(out->copy_bundle, cbundle.data(), 4 * M);
    memcpy(out->copy_off, coff.data(), 8 * M);
  }
  if (!nb_index.empty()) {
    memcpy(out->new_bundle_index, nb_index.data(), 4 * nb_index.size());
    memcpy(out->new_bundle_size, nb_size.data(), 8 * nb_size.size());
  }
  s->times.host_ms += ms_between(t_rule, Clock::now());
  return ZC_OK;
}

}  // namespace zc
