// zc_resolve.hip -- the resident chunk index: which bundle holds a chunk id, and
// where, answered in HBM for a whole backup at a time.  The reference resolves
// a restore in three places: ChunkStorage::Reader::get (chunk_storage.cc:214-260)
// asks ChunkIndex::findChunk (chunk_index.cc:119-161) for the bundle of an id,
// the table it asks was filled by loadIndex / registerNewChunkId
// (chunk_index.cc:26-79,163-182), and Bundle::Reader (bundle.cc:220-251) says
// where the chunk lies in that bundle's payload.  Here the table is garbage
// collection's exact id table (zc_gc_core.h), kept with each record's payload
// offset, and a resolve is one probe per chunk_to_emit (zc_resolve_core.h).
//
//   build     zc_scan_tile_sums / zc_scan_tile_scan / zc_scan_write (zc_scan_body.h)
//                                 the running sum of `sizes` over all records
//             zc_rs_place         records into processing order (zc_gc.hip): per position
//                                 its id, size, bundle and payload offset = the running sum
//                                 at the record less the running sum at its bundle's first
//             zc_rs_bundle_sizes  per bundle: the running sum across it
//             zc_rs_insert        every position into the id table, equal ids keep the smallest
//             zc_rs_insert_pairs  every position into the (id, bundle) table; a key met
//                                 twice flags its bundle
//             zc_rs_count         the id table's filled slots, the flagged bundles
//   lookup    zc_rs_lookup        findChunk for a batch of ids
//   resolve   zc_rs_probe         per entry: the owner's bundle, offset, size; used-bundle
//                                 flags; the missing and duplicate-using entries, counted, with
//                                 the smallest entry of each
//             the three scan kernels over the used flags (bundle -> slot) and over the
//             entry sizes (dst)
//             zc_rs_used          the used bundles, ascending, with their payload sizes
//             zc_rs_slots         per entry: its slot
//   replay    zc_rp_pieces        per entry: its copies of at most 64 KiB (zclzo::kPiece), scanned
//             zc_rp_copy          a wave per piece: the entry by binary search over the scan, then
//                                 zccopy::wave_copy from the entry's slot to the output
//
// The outputs are functions of the final tables, which do not depend on the
// order of the inserts (zc_gc_core.h, zc_resolve_core.h); only max_probe (a
// statistic) depends on the schedule.  Every loop bound is a count the host
// fixed before the launch from validated input; every kernel is grid-stride; no
// kernel waits on another wave or workgroup, spins, or ends on a data value; a
// probe walk ends after `capacity` slots at the latest.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_copy_body.h"
#include "zc_device.h"
#include "zc_lzo_core.h"
#include "zc_resolve_core.h"
#include "zc_scan_body.h"

static_assert(sizeof(zc_instruction) == 48, "zc_instruction is read as twelve 32-bit words");
static_assert(ZC_INSTR_CHUNK == zcrs::kKindChunk && ZC_INSTR_BYTES == zcrs::kKindBytes, "entry kinds");

namespace zc {

namespace {

constexpr int kBlock = zcscan::kBlock;
constexpr uint32_t kTile = zcscan::kTile;  // values per scan tile (zc_scan_body.h)
constexpr uint64_t kCountLimit = 0xffffffffull;  // counts stay below 2^32 - 1

// what the kernels report, one copy on the device
struct RsDev {
  unsigned long long first_missing, first_dup;  // the smallest such entry (~0: none)
  unsigned long long total[2];                  // a scan's sum: [0] sizes / used flags, [1] entry sizes
  unsigned long long n_distinct, n_flagged;
  uint32_t n_missing, n_dup_used;
  uint32_t max_probe;
  uint32_t internal;  // bit 0: an insert found no slot
};

__device__ inline void note_probe(RsDev* dev, uint32_t longest) {
  if (longest) atomicMax(&dev->max_probe, longest);
}

__global__ __launch_bounds__(kBlock) void zc_rs_place(const uint64_t* __restrict__ ids,
                                                      const uint32_t* __restrict__ sizes,
                                                      const uint64_t* __restrict__ bf, uint32_t nb, uint64_t n,
                                                      const uint64_t* __restrict__ run, uint64_t* __restrict__ idp,
                                                      uint32_t* __restrict__ szp, uint64_t* __restrict__ offp,
                                                      uint32_t* __restrict__ bund) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    const uint32_t b = zcrs::bundle_of(bf, nb, p);
    const uint64_t r = zcrs::record_of(bf, b, p);
    const zcgc::Id v = zcgc::load_id(ids, r);
    idp[3 * p] = v.w[0];
    idp[3 * p + 1] = v.w[1];
    idp[3 * p + 2] = v.w[2];
    szp[p] = sizes[r];
    offp[p] = run[r] - run[bf[b]];
    bund[p] = b;
  }
}

__global__ __launch_bounds__(kBlock) void zc_rs_bundle_sizes(const uint64_t* __restrict__ bf, uint64_t nb,
                                                             const uint64_t* __restrict__ run,
                                                             uint64_t* __restrict__ bsize) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += stride)
    bsize[b] = run[bf[b + 1]] - run[bf[b]];
}

__global__ __launch_bounds__(kBlock) void zc_rs_insert(uint32_t* __restrict__ table, uint64_t mask,
                                                       const uint64_t* __restrict__ idp, uint64_t n, RsDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    const uint32_t steps = zcgc::insert(table, mask, idp, (uint32_t)p);
    if (!steps) atomicOr(&dev->internal, 1u);
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

__global__ __launch_bounds__(kBlock) void zc_rs_insert_pairs(uint32_t* __restrict__ pairs, uint64_t mask,
                                                             const uint64_t* __restrict__ idp,
                                                             const uint32_t* __restrict__ bund, uint64_t n,
                                                             uint8_t* __restrict__ bdup, RsDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    bool twice = false;
    const uint32_t steps = zcrs::insert_pair(pairs, mask, idp, bund, (uint32_t)p, &twice);
    if (!steps) atomicOr(&dev->internal, 1u);
    if (twice) bdup[bund[p]] = 1;  // every writer stores the same byte
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

// the id table's filled slots (= distinct ids) and the flagged bundles
__global__ __launch_bounds__(kBlock) void zc_rs_count(const uint32_t* __restrict__ table, uint64_t slots,
                                                      const uint8_t* __restrict__ bdup, uint64_t nb, RsDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t filled = 0, flagged = 0;
  for (uint64_t s = first; s < slots; s += stride) filled += table[s] != zcgc::kEmpty;
  for (uint64_t b = first; b < nb; b += stride) flagged += bdup[b] != 0;
  for (int m = 32; m >= 1; m >>= 1) {
    filled += __shfl_xor(filled, m, 64);
    flagged += __shfl_xor(flagged, m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (filled) atomicAdd(&dev->n_distinct, (unsigned long long)filled);
    if (flagged) atomicAdd(&dev->n_flagged, (unsigned long long)flagged);
  }
}

// what a resolve or a lookup reads of an index
struct IndexView {
  const uint32_t* table;
  uint64_t mask;
  const uint64_t* idp;
  const uint32_t* bund;
  const uint64_t* offp;
  const uint32_t* szp;
  const uint8_t* bdup;
};

__global__ __launch_bounds__(kBlock) void zc_rs_lookup(IndexView ix, const uint64_t* __restrict__ keys, uint64_t n,
                                                       uint32_t* __restrict__ bundle, uint64_t* __restrict__ off,
                                                       uint32_t* __restrict__ size, RsDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint32_t steps;
    const zcrs::Hit h = zcrs::find(ix.table, ix.mask, ix.idp, ix.bund, ix.offp, ix.szp, zcgc::load_id(keys, i), &steps);
    bundle[i] = h.bundle;
    off[i] = h.off;
    size[i] = h.size;
    longest = max(longest, steps);
  }
  note_probe(dev, longest);
}

// ins: the zc_instruction array as 32-bit words (the id sits at byte 4, so it
// is read in halves; data_off and size at bytes 32 and 40 are 8-byte aligned)
__global__ __launch_bounds__(kBlock) void zc_rs_probe(IndexView ix, const uint32_t* __restrict__ ins, uint64_t n,
                                                      uint32_t* __restrict__ ebund, uint64_t* __restrict__ eoff,
                                                      uint64_t* __restrict__ esize, uint8_t* __restrict__ bused,
                                                      RsDev* dev) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t longest = 0, missing = 0, dups = 0;
  unsigned long long first_missing = ~0ull, first_dup = ~0ull;
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
    const uint32_t* w = ins + 12 * e;
    zcgc::Id id;
    for (int k = 0; k < 3; k++) id.w[k] = (uint64_t)w[1 + 2 * k] | (uint64_t)w[2 + 2 * k] << 32;
    const uint64_t* q = (const uint64_t*)(w + 8);
    uint32_t steps;
    const zcrs::Entry r =
        zcrs::resolve_entry(ix.table, ix.mask, ix.idp, ix.bund, ix.offp, ix.szp, w[0], id, q[0], q[1], &steps);
    longest = max(longest, steps);
    // a BYTES entry gets the number below kNoBundle: no bundle has it (the counts stay below 2^32 - 1)
    ebund[e] = r.bytes ? zcrs::kNoBundle - 1 : r.bundle;
    eoff[e] = r.off;
    esize[e] = r.size;
    if (!r.bytes) {
      if (r.bundle == zcrs::kNoBundle) {
        missing++;
        first_missing = min(first_missing, (unsigned long long)e);
      } else {
        bused[r.bundle] = 1;  // every writer stores the same byte
        if (ix.bdup[r.bundle]) {
          dups++;
          first_dup = min(first_dup, (unsigned long long)e);
        }
      }
    }
  }
  note_probe(dev, longest);
  if (missing) {
    atomicAdd(&dev->n_missing, missing);
    atomicMin(&dev->first_missing, first_missing);
  }
  if (dups) {
    atomicAdd(&dev->n_dup_used, dups);
    atomicMin(&dev->first_dup, first_dup);
  }
}

// slotof: the exclusive scan of the used flags, so bundle b is slot slotof[b]
__global__ __launch_bounds__(kBlock) void zc_rs_used(const uint8_t* __restrict__ bused,
                                                     const uint64_t* __restrict__ slotof,
                                                     const uint64_t* __restrict__ bsize, uint64_t nb,
                                                     uint32_t* __restrict__ used, uint64_t* __restrict__ used_size) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += stride)
    if (bused[b]) {
      used[slotof[b]] = (uint32_t)b;  // slotof[b] < the used bundles <= nb, the room of both lists
      used_size[slotof[b]] = bsize[b];
    }
}

__global__ __launch_bounds__(kBlock) void zc_rs_slots(const uint32_t* __restrict__ ebund,
                                                      const uint64_t* __restrict__ slotof, uint64_t n,
                                                      const RsDev* __restrict__ dev, uint32_t* __restrict__ slot) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint32_t n_used = (uint32_t)dev->total[0];
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
    const uint32_t b = ebund[e];
    slot[e] = b == zcrs::kNoBundle ? zcrs::kNoBundle : b == zcrs::kNoBundle - 1 ? n_used : (uint32_t)slotof[b];
  }
}

constexpr uint64_t kPiece = zclzo::kPiece;  // the scatter's piece: a long entry is split over waves

__global__ __launch_bounds__(kBlock) void zc_rp_pieces(const uint64_t* __restrict__ esize, uint64_t n,
                                                       uint64_t* __restrict__ pc) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride)
    pc[e] = esize[e] / kPiece + (esize[e] % kPiece != 0);
}

// pstart: the exclusive scan of the piece counts, pstart[n] = pieces.  base: n_base device pointers.
__global__ __launch_bounds__(kBlock) void zc_rp_copy(const uint64_t* __restrict__ pstart, uint64_t n, uint64_t pieces,
                                                     const uint32_t* __restrict__ slot,
                                                     const uint64_t* __restrict__ eoff,
                                                     const uint64_t* __restrict__ esize,
                                                     const uint64_t* __restrict__ dst,
                                                     const uint8_t* const* __restrict__ base, uint32_t n_base,
                                                     uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t q = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); q < pieces; q += waves) {
    // the entry of piece q: pstart[lo] <= q < pstart[hi]; bound: 32 halvings, n < 2^32
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (pstart[mid] <= q)
        lo = mid;
      else
        hi = mid;
    }
    const uint64_t at = (q - pstart[lo]) * kPiece, size = esize[lo];
    const uint32_t k = slot[lo];
    if (k >= n_base || at >= size) continue;  // neither happens on a plan restore_replay_validate let through
    zccopy::wave_copy(out + dst[lo] + at, base[k] + eoff[lo] + at, min(kPiece, size - at), lane);
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

struct SetDevice {
  int prev = -1;
  explicit SetDevice(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != d) (void)hipSetDevice(d);
  }
  ~SetDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
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
#define RCK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

}  // namespace

}  // namespace zc

// the index: device memory of its own, read-only once built, so any number of
// contexts may resolve against it
struct zc_chunk_index {
  int device = 0;
  uint64_t n_records = 0, n_bundles = 0, slots = 0, n_distinct = 0, n_flagged = 0;
  zc::Buf<uint64_t> idp, offp, bsize;
  zc::Buf<uint32_t> szp, bund, table;
  zc::Buf<uint8_t> bdup;
};

// a resolved backup: the counters and the used bundles on the host; the per-entry lists on the host
// (zc_restore_resolve) or in HBM (zc_restore_resolve_device, and a host plan's copy for its replays)
struct zc_restore_plan {
  uint64_t n_entries = 0, n_used = 0, length = 0, n_missing = 0, first_missing = 0, n_dup_used = 0, first_dup = 0;
  uint64_t bytes_total = 0;  // the BYTES entries' sizes: above 0, a replay reads the instruction stream's slot
  std::vector<uint32_t> used, slot;
  std::vector<uint64_t> used_size, off, size, dst;
  bool on_device = false;  // the host vectors of the per-entry lists are empty
  int device = 0;
  mutable std::mutex mu;          // guards a host plan's one upload
  mutable bool resident = false;  // d_* hold the lists
  mutable zc::Buf<uint32_t> d_slot;
  mutable zc::Buf<uint64_t> d_off, d_size, d_dst;
};

namespace zc {

struct ResolveScratch {
  Buf<uint64_t> ids, bf, run, tsum, keys, off64, eoff, esize, dst, slotof, used_size, pc, pstart, base;
  Buf<uint32_t> sizes, pairs, ins, bundle32, size32, ebund, slot, used;
  Buf<uint8_t> bused;
  Buf<RsDev> dev;
  hipEvent_t ev[2] = {};
  int cus = 0;
  ResolveTimes times{};
  ~ResolveScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

ResolveScratch* resolve_scratch_new() { return new ResolveScratch(); }
void resolve_scratch_free(ResolveScratch* s) { delete s; }
const ResolveTimes* resolve_times(const ResolveScratch* s) { return &s->times; }

namespace {

int first_use(ResolveScratch* s, hipStream_t st, std::string& err) {
  if (s->cus) return ZC_OK;
  int dev = 0, cus = 0;
  RCK(hipGetDevice(&dev));
  RCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  for (hipEvent_t& e : s->ev) RCK(hipEventCreate(&e));
  RCK(s->dev.ensure(1));
  s->cus = std::max(cus, 1);
  return ZC_OK;
}

int grid_for(const ResolveScratch* s, uint64_t items) {
  const uint64_t blocks = (items + kBlock - 1) / kBlock;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * 16));
}

// out[i] = the sum of src[0 .. i) for i < n (and out[n] with tail); *total on the device
template <class T>
int scan(ResolveScratch* s, const T* src, uint64_t n, uint64_t* out, bool tail, unsigned long long* d_total,
         hipStream_t st, std::string& err) {
  const uint32_t ntiles = (uint32_t)((n + kTile - 1) / kTile);  // n < 2^32
  if (!ntiles) return ZC_OK;  // the caller zeroed *d_total
  RCK(s->tsum.ensure(ntiles));
  const int gt = (int)std::min<uint64_t>(ntiles, (uint64_t)s->cus * 16);
  zcscan::zc_scan_tile_sums<T><<<gt, kBlock, 0, st>>>(src, n, ntiles, s->tsum.p);
  zcscan::zc_scan_tile_scan<<<1, kBlock, 0, st>>>(s->tsum.p, ntiles, d_total);
  zcscan::zc_scan_write<T><<<gt, kBlock, 0, st>>>(src, n, ntiles, s->tsum.p, out, tail ? 1 : 0);
  return ZC_OK;
}

RsDev fresh_dev() {
  RsDev h{};
  h.first_missing = h.first_dup = ~0ull;
  return h;
}

IndexView view_of(const zc_chunk_index* ix) {
  return IndexView{ix->table.p, ix->slots - 1, ix->idp.p, ix->bund.p, ix->offp.p, ix->szp.p, ix->bdup.p};
}

}  // namespace

int chunk_index_validate(bool host, const void* ids, const void* sizes, uint64_t N, const uint64_t* bundle_first,
                         uint64_t B, zc_chunk_index* const* out, std::string& err) {
  char msg[200];
  if (!out) return arg_error(err, "null index pointer");
  if (N >= kCountLimit || B >= kCountLimit) {
    snprintf(msg, sizeof msg, "%llu records, %llu bundles: each must stay below 2^32 - 1", (unsigned long long)N,
             (unsigned long long)B);
    return arg_error(err, msg);
  }
  if (N && (!ids || !sizes)) return arg_error(err, "null input array");
  if (!host) return ZC_OK;  // a set's bundle_first was made by zc_index_load
  // zc_gc_plan's rules; a NULL range array of no entries stands for {0}
  const uint64_t* first = bundle_first;
  if (!first) {
    if (B) return arg_error(err, "null input array");
    if (N == 0) return ZC_OK;
    snprintf(msg, sizeof msg, "bundle_first is empty but there are %llu records", (unsigned long long)N);
    return arg_error(err, msg);
  }
  if (first[0] != 0) {
    snprintf(msg, sizeof msg, "bundle_first[0] = %llu, not 0", (unsigned long long)first[0]);
    return arg_error(err, msg);
  }
  for (uint64_t k = 0; k < B; k++)
    if (first[k + 1] < first[k]) {
      snprintf(msg, sizeof msg, "bundle_first[%llu] = %llu is below bundle_first[%llu] = %llu",
               (unsigned long long)(k + 1), (unsigned long long)first[k + 1], (unsigned long long)k,
               (unsigned long long)first[k]);
      return arg_error(err, msg);
    }
  if (first[B] != N) {
    snprintf(msg, sizeof msg, "bundle_first ends at %llu, there are %llu records", (unsigned long long)first[B],
             (unsigned long long)N);
    return arg_error(err, msg);
  }
  return ZC_OK;
}

int chunk_index_build(ResolveScratch* s, int device, bool host, const void* ids, const void* sizes, uint64_t N,
                      const uint64_t* bundle_first, uint64_t B, zc_chunk_index** out, hipStream_t st,
                      std::string& err) {
  *out = nullptr;
  int rc = first_use(s, st, err);
  if (rc != ZC_OK) return rc;
  const char* tb = getenv("ZC_TEST_RESOLVE_BITS");
  const uint64_t slots = zcgc::capacity_for(N, tb ? atoi(tb) : 0);
  const uint64_t mask = slots - 1;
  zc_chunk_index* ix = new zc_chunk_index();
  struct Drop {
    zc_chunk_index* p;
    ~Drop() { delete p; }
  } drop{ix};
  ix->device = device;
  ix->n_records = N;
  ix->n_bundles = B;
  ix->slots = slots;
  RCK(ix->idp.ensure(3 * N));
  RCK(ix->offp.ensure(N));
  RCK(ix->szp.ensure(N));
  RCK(ix->bund.ensure(N));
  RCK(ix->table.ensure(slots));
  RCK(ix->bsize.ensure(B));
  RCK(ix->bdup.ensure(B));
  RCK(s->run.ensure(N + 1));
  RCK(s->pairs.ensure(N ? slots : 1));
  RCK(s->tsum.ensure((N + kTile - 1) / kTile));
  const uint64_t* d_ids = (const uint64_t*)ids;
  const uint32_t* d_sizes = (const uint32_t*)sizes;
  const uint64_t* d_bf = bundle_first;
  if (host) {
    RCK(s->ids.ensure(3 * N));
    RCK(s->sizes.ensure(N));
    RCK(s->bf.ensure(B + 1));
    if (N) {
      RCK(hipMemcpyAsync(s->ids.p, ids, 24 * N, hipMemcpyHostToDevice, st));
      RCK(hipMemcpyAsync(s->sizes.p, sizes, 4 * N, hipMemcpyHostToDevice, st));
    }
    if (B) RCK(hipMemcpyAsync(s->bf.p, bundle_first, 8 * (B + 1), hipMemcpyHostToDevice, st));
    d_ids = s->ids.p;
    d_sizes = s->sizes.p;
    d_bf = s->bf.p;
  }
  RsDev h = fresh_dev();
  RCK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
  RCK(hipMemsetAsync(ix->table.p, 0xff, 4 * slots, st));
  if (B) RCK(hipMemsetAsync(ix->bdup.p, 0, B, st));
  RCK(hipMemsetAsync(s->run.p, 0, 8, st));  // the run of no records is {0}
  RCK(hipEventRecord(s->ev[0], st));
  if (N) {  // N > 0 implies B > 0 (bundle_first ends at N)
    RCK(hipMemsetAsync(s->pairs.p, 0xff, 4 * slots, st));
    rc = scan<uint32_t>(s, d_sizes, N, s->run.p, true, &s->dev.p->total[0], st, err);
    if (rc != ZC_OK) return rc;
    const int gn = grid_for(s, N);
    zc_rs_place<<<gn, kBlock, 0, st>>>(d_ids, d_sizes, d_bf, (uint32_t)B, N, s->run.p, ix->idp.p, ix->szp.p,
                                       ix->offp.p, ix->bund.p);
    zc_rs_insert<<<gn, kBlock, 0, st>>>(ix->table.p, mask, ix->idp.p, N, s->dev.p);
    zc_rs_insert_pairs<<<gn, kBlock, 0, st>>>(s->pairs.p, mask, ix->idp.p, ix->bund.p, N, ix->bdup.p, s->dev.p);
  }
  if (B) {
    zc_rs_bundle_sizes<<<grid_for(s, B), kBlock, 0, st>>>(d_bf, B, s->run.p, ix->bsize.p);
    zc_rs_count<<<grid_for(s, std::max(slots, B)), kBlock, 0, st>>>(ix->table.p, slots, ix->bdup.p, B, s->dev.p);
  }
  RCK(hipGetLastError());
  RCK(hipEventRecord(s->ev[1], st));
  RCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  RCK(hipStreamSynchronize(st));
  float ms = 0;
  RCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->times.build_ms = ms;
  s->times.table_slots = slots;
  s->times.max_probe = h.max_probe;
  if (h.internal) {
    err = "a table has no free slot (internal error)";
    return ZC_ERR_STATE;
  }
  ix->n_distinct = h.n_distinct;
  ix->n_flagged = h.n_flagged;
  drop.p = nullptr;
  *out = ix;
  return ZC_OK;
}

void chunk_index_counts(const zc_chunk_index* ix, uint64_t* n_records, uint64_t* n_bundles, uint64_t* n_ids,
                        uint64_t* n_flagged) {
  if (n_records) *n_records = ix->n_records;
  if (n_bundles) *n_bundles = ix->n_bundles;
  if (n_ids) *n_ids = ix->n_distinct;
  if (n_flagged) *n_flagged = ix->n_flagged;
}

int chunk_index_device(const zc_chunk_index* ix) { return ix->device; }

int chunk_index_bundles(const zc_chunk_index* ix, uint64_t* payload_size, uint8_t* dup, std::string& err) {
  const uint64_t B = ix->n_bundles;
  if (!B) return ZC_OK;
  SetDevice g(ix->device);
  hipError_t e = hipSuccess;
  if (payload_size) e = hipMemcpy(payload_size, ix->bsize.p, 8 * B, hipMemcpyDeviceToHost);
  if (e == hipSuccess && dup) e = hipMemcpy(dup, ix->bdup.p, B, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    err = hipGetErrorString(e);
    return ZC_ERR_HIP;
  }
  return ZC_OK;
}

void chunk_index_destroy(zc_chunk_index* ix) {
  SetDevice g(ix->device);
  delete ix;
}

int chunk_index_lookup(ResolveScratch* s, const zc_chunk_index* ix, const uint8_t* ids, uint64_t n, uint32_t* bundle,
                       uint64_t* off, uint32_t* size, hipStream_t st, std::string& err) {
  int rc = first_use(s, st, err);
  if (rc != ZC_OK) return rc;
  s->times.resolve_ms = 0;
  s->times.table_slots = ix->slots;
  s->times.max_probe = 0;
  if (!n) return ZC_OK;
  RCK(s->keys.ensure(3 * n));
  RCK(s->bundle32.ensure(n));
  RCK(s->off64.ensure(n));
  RCK(s->size32.ensure(n));
  RsDev h = fresh_dev();
  RCK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
  RCK(hipMemcpyAsync(s->keys.p, ids, 24 * n, hipMemcpyHostToDevice, st));
  RCK(hipEventRecord(s->ev[0], st));
  zc_rs_lookup<<<grid_for(s, n), kBlock, 0, st>>>(view_of(ix), s->keys.p, n, s->bundle32.p, s->off64.p, s->size32.p,
                                                  s->dev.p);
  RCK(hipGetLastError());
  RCK(hipEventRecord(s->ev[1], st));
  RCK(hipMemcpyAsync(bundle, s->bundle32.p, 4 * n, hipMemcpyDeviceToHost, st));
  RCK(hipMemcpyAsync(off, s->off64.p, 8 * n, hipMemcpyDeviceToHost, st));
  RCK(hipMemcpyAsync(size, s->size32.p, 4 * n, hipMemcpyDeviceToHost, st));
  RCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  RCK(hipStreamSynchronize(st));
  float ms = 0;
  RCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->times.resolve_ms = ms;
  s->times.max_probe = h.max_probe;
  return ZC_OK;
}

int resolve_validate(const zc_instruction* ins, uint64_t n, uint64_t instr_bytes, zc_restore_plan* const* out,
                     uint64_t* bytes_total, std::string& err) {
  char msg[200];
  if (!out) return arg_error(err, "null plan pointer");
  if (n >= kCountLimit) {
    snprintf(msg, sizeof msg, "%llu entries: the count must stay below 2^32 - 1", (unsigned long long)n);
    return arg_error(err, msg);
  }
  if (n && !ins) return arg_error(err, "null instruction array");
  uint64_t total = 0;
  for (uint64_t e = 0; e < n; e++) {
    if (ins[e].kind == ZC_INSTR_CHUNK) continue;
    if (ins[e].kind != ZC_INSTR_BYTES) {
      snprintf(msg, sizeof msg, "entry %llu has kind %u, neither ZC_INSTR_CHUNK nor ZC_INSTR_BYTES",
               (unsigned long long)e, ins[e].kind);
      return arg_error(err, msg);
    }
    if (ins[e].data_off > instr_bytes || ins[e].size > instr_bytes - ins[e].data_off) {
      snprintf(msg, sizeof msg, "entry %llu: bytes [%llu, +%llu) run past the stream's %llu bytes",
               (unsigned long long)e, (unsigned long long)ins[e].data_off, (unsigned long long)ins[e].size,
               (unsigned long long)instr_bytes);
      return arg_error(err, msg);
    }
    if (total + ins[e].size < total) {
      snprintf(msg, sizeof msg, "the stream's length passes 2^64 at entry %llu", (unsigned long long)e);
      return arg_error(err, msg);
    }
    total += ins[e].size;
  }
  *bytes_total = total;
  return ZC_OK;
}

int resolve_device_validate(const zc_instr_set* set, int index_device, zc_restore_plan* const* out, const uint32_t** d_ins,
                            uint64_t* n, uint64_t* bytes_total, std::string& err) {
  if (!out) return arg_error(err, "null plan pointer");
  if (!set) return arg_error(err, "null instruction set");
  int device = 0;
  instr_set_view(set, &device, d_ins, n, bytes_total);
  if (device != index_device) return arg_error(err, "the instruction set lives on another device than the index");
  return ZC_OK;
}

// d_ins: a zc_instr_set's entries in HBM (ins is NULL then): nothing per entry is
// uploaded, and the plan keeps its per-entry lists where the kernels wrote them
int restore_resolve(ResolveScratch* s, const zc_chunk_index* ix, const zc_instruction* ins, const uint32_t* d_ins,
                    uint64_t n, uint64_t bytes_total, zc_restore_plan** out, hipStream_t st, std::string& err) {
  *out = nullptr;
  int rc = first_use(s, st, err);
  if (rc != ZC_OK) return rc;
  s->times.resolve_ms = 0;
  s->times.table_slots = ix->slots;
  s->times.max_probe = 0;
  zc_restore_plan* pl = new zc_restore_plan();
  struct Drop {
    zc_restore_plan* p;
    ~Drop() { delete p; }
  } drop{pl};
  pl->n_entries = n;
  pl->bytes_total = bytes_total;
  pl->device = ix->device;
  pl->on_device = d_ins != nullptr;
  if (n) {
    const uint64_t B = ix->n_bundles;
    uint32_t* d_slot = nullptr;
    uint64_t *d_off = nullptr, *d_size = nullptr, *d_dst = nullptr;
    if (d_ins) {
      RCK(pl->d_slot.ensure(n));
      RCK(pl->d_off.ensure(n));
      RCK(pl->d_size.ensure(n));
      RCK(pl->d_dst.ensure(n));
      d_slot = pl->d_slot.p, d_off = pl->d_off.p, d_size = pl->d_size.p, d_dst = pl->d_dst.p;
      pl->resident = true;
    } else {
      RCK(s->ins.ensure(12 * n));
      RCK(s->eoff.ensure(n));
      RCK(s->esize.ensure(n));
      RCK(s->dst.ensure(n));
      RCK(s->slot.ensure(n));
      d_slot = s->slot.p, d_off = s->eoff.p, d_size = s->esize.p, d_dst = s->dst.p;
    }
    RCK(s->ebund.ensure(n));
    RCK(s->bused.ensure(B));
    RCK(s->slotof.ensure(B));
    RCK(s->used.ensure(B));
    RCK(s->used_size.ensure(B));
    RCK(s->tsum.ensure((std::max(n, B) + kTile - 1) / kTile));  // both scans' tiles: no buffer is made mid-stream
    RsDev h = fresh_dev();
    RCK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (!d_ins) {
      RCK(hipMemcpyAsync(s->ins.p, ins, 48 * n, hipMemcpyHostToDevice, st));
      d_ins = s->ins.p;
    }
    if (B) RCK(hipMemsetAsync(s->bused.p, 0, B, st));
    RCK(hipEventRecord(s->ev[0], st));
    const int gn = grid_for(s, n);
    zc_rs_probe<<<gn, kBlock, 0, st>>>(view_of(ix), d_ins, n, s->ebund.p, d_off, d_size, s->bused.p, s->dev.p);
    rc = scan<uint8_t>(s, s->bused.p, B, s->slotof.p, false, &s->dev.p->total[0], st, err);
    if (rc != ZC_OK) return rc;
    rc = scan<uint64_t>(s, d_size, n, d_dst, false, &s->dev.p->total[1], st, err);
    if (rc != ZC_OK) return rc;
    if (B)
      zc_rs_used<<<grid_for(s, B), kBlock, 0, st>>>(s->bused.p, s->slotof.p, ix->bsize.p, B, s->used.p,
                                                    s->used_size.p);
    zc_rs_slots<<<gn, kBlock, 0, st>>>(s->ebund.p, s->slotof.p, n, s->dev.p, d_slot);
    RCK(hipGetLastError());
    RCK(hipEventRecord(s->ev[1], st));
    if (!pl->on_device) {
      pl->slot.resize(n);
      pl->off.resize(n);
      pl->size.resize(n);
      pl->dst.resize(n);
      RCK(hipMemcpyAsync(pl->slot.data(), d_slot, 4 * n, hipMemcpyDeviceToHost, st));
      RCK(hipMemcpyAsync(pl->off.data(), d_off, 8 * n, hipMemcpyDeviceToHost, st));
      RCK(hipMemcpyAsync(pl->size.data(), d_size, 8 * n, hipMemcpyDeviceToHost, st));
      RCK(hipMemcpyAsync(pl->dst.data(), d_dst, 8 * n, hipMemcpyDeviceToHost, st));
    }
    RCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
    RCK(hipStreamSynchronize(st));
    float ms = 0;
    RCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.resolve_ms = ms;
    s->times.max_probe = h.max_probe;
    const uint64_t n_used = h.total[0];
    if (n_used > B) {
      err = "more used bundles than bundles (internal error)";
      return ZC_ERR_STATE;
    }
    // the chunk sizes alone stay below 2^64 (fewer than 2^32 entries of fewer
    // than 2^32 bytes), so they are the device's sum, taken modulo 2^64, less the bytes runs
    const uint64_t chunk_total = h.total[1] - bytes_total;
    if (chunk_total + bytes_total < chunk_total) return arg_error(err, "the stream's length passes 2^64");
    pl->length = h.total[1];
    pl->n_used = n_used;
    pl->n_missing = h.n_missing;
    pl->first_missing = h.n_missing ? h.first_missing : 0;
    pl->n_dup_used = h.n_dup_used;
    pl->first_dup = h.n_dup_used ? h.first_dup : 0;
    pl->used.resize(n_used);
    pl->used_size.resize(n_used);
    if (n_used) {
      RCK(hipMemcpyAsync(pl->used.data(), s->used.p, 4 * n_used, hipMemcpyDeviceToHost, st));
      RCK(hipMemcpyAsync(pl->used_size.data(), s->used_size.p, 8 * n_used, hipMemcpyDeviceToHost, st));
      RCK(hipStreamSynchronize(st));
    }
  }
  drop.p = nullptr;
  *out = pl;
  return ZC_OK;
}

void restore_plan_counts(const zc_restore_plan* pl, uint64_t* n_entries, uint64_t* n_used, uint64_t* length,
                         uint64_t* n_missing, uint64_t* first_missing, uint64_t* n_dup_used, uint64_t* first_dup) {
  if (n_entries) *n_entries = pl->n_entries;
  if (n_used) *n_used = pl->n_used;
  if (length) *length = pl->length;
  if (n_missing) *n_missing = pl->n_missing;
  if (first_missing) *first_missing = pl->first_missing;
  if (n_dup_used) *n_dup_used = pl->n_dup_used;
  if (first_dup) *first_dup = pl->first_dup;
}

namespace {

// count entries from `first` of a device plan's lists to host arrays (NULL skips)
int plan_download(const zc_restore_plan* pl, uint64_t first, uint64_t count, uint32_t* slot, uint64_t* off,
                  uint64_t* size, uint64_t* dst, std::string& err) {
  SetDevice g(pl->device);
  hipError_t e = hipSuccess;
  if (slot) e = hipMemcpy(slot, pl->d_slot.p + first, 4 * count, hipMemcpyDeviceToHost);
  if (e == hipSuccess && off) e = hipMemcpy(off, pl->d_off.p + first, 8 * count, hipMemcpyDeviceToHost);
  if (e == hipSuccess && size) e = hipMemcpy(size, pl->d_size.p + first, 8 * count, hipMemcpyDeviceToHost);
  if (e == hipSuccess && dst) e = hipMemcpy(dst, pl->d_dst.p + first, 8 * count, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    err = hipGetErrorString(e);
    return ZC_ERR_HIP;
  }
  return ZC_OK;
}

}  // namespace

void restore_plan_used(const zc_restore_plan* pl, uint32_t* used, uint64_t* used_size) {
  const size_t u = pl->n_used;
  if (used && u) memcpy(used, pl->used.data(), 4 * u);
  if (used_size && u) memcpy(used_size, pl->used_size.data(), 8 * u);
}

int restore_plan_fetch(const zc_restore_plan* pl, uint32_t* used, uint64_t* used_size, uint32_t* slot, uint64_t* off,
                       uint64_t* size, uint64_t* dst, std::string& err) {
  const size_t n = pl->n_entries;
  restore_plan_used(pl, used, used_size);
  if (!n) return ZC_OK;
  if (pl->on_device) return plan_download(pl, 0, n, slot, off, size, dst, err);  // on demand: the plan keeps no host copy
  if (slot) memcpy(slot, pl->slot.data(), 4 * n);
  if (off) memcpy(off, pl->off.data(), 8 * n);
  if (size) memcpy(size, pl->size.data(), 8 * n);
  if (dst) memcpy(dst, pl->dst.data(), 8 * n);
  return ZC_OK;
}

int restore_plan_entry(const zc_restore_plan* pl, uint64_t e, uint32_t* slot, uint64_t* off, uint64_t* size,
                       uint64_t* dst, std::string& err) {
  if (e >= pl->n_entries) {
    char msg[120];
    snprintf(msg, sizeof msg, "entry %llu of %llu", (unsigned long long)e, (unsigned long long)pl->n_entries);
    return arg_error(err, msg);
  }
  if (pl->on_device) return plan_download(pl, e, 1, slot, off, size, dst, err);
  if (slot) *slot = pl->slot[e];
  if (off) *off = pl->off[e];
  if (size) *size = pl->size[e];
  if (dst) *dst = pl->dst[e];
  return ZC_OK;
}

void restore_plan_destroy(zc_restore_plan* pl) {
  SetDevice g(pl->device);
  delete pl;
}

int replay_validate(const zc_restore_plan* pl, int ctx_device, const void* const* slot_base, size_t n_slots,
                    const void* d_out, uint64_t out_cap, std::string& err) {
  char msg[200];
  if (!pl) return arg_error(err, "null plan");
  if (pl->n_missing) {
    snprintf(msg, sizeof msg, "the plan has %llu entries whose chunk id is missing (the first is entry %llu)",
             (unsigned long long)pl->n_missing, (unsigned long long)pl->first_missing);
    return arg_error(err, msg);
  }
  if (pl->n_dup_used) {
    snprintf(msg, sizeof msg, "the plan uses a bundle that holds a chunk id twice (%llu entries, the first is %llu)",
             (unsigned long long)pl->n_dup_used, (unsigned long long)pl->first_dup);
    return arg_error(err, msg);
  }
  if (n_slots != pl->n_used + 1) {
    snprintf(msg, sizeof msg, "%llu slots, the plan has %llu used bundles and the instruction stream",
             (unsigned long long)n_slots, (unsigned long long)pl->n_used);
    return arg_error(err, msg);
  }
  if (!slot_base) return arg_error(err, "null slot array");
  for (uint64_t k = 0; k < pl->n_used; k++)
    if (!slot_base[k] && pl->used_size[k]) {
      snprintf(msg, sizeof msg, "slot %llu (bundle %u) has no payload", (unsigned long long)k, pl->used[k]);
      return arg_error(err, msg);
    }
  if (pl->bytes_total && !slot_base[pl->n_used])
    return arg_error(err, "the instruction stream's slot is null and the plan has bytes_to_emit runs");
  if (pl->length > out_cap) {
    snprintf(msg, sizeof msg, "%llu bytes to restore, room for %llu", (unsigned long long)pl->length,
             (unsigned long long)out_cap);
    return arg_error(err, msg);
  }
  if (pl->length && !d_out) return arg_error(err, "null output");
  if (ctx_device >= 0 && pl->n_entries && pl->device != ctx_device)
    return arg_error(err, "the plan lives on another device than the context");
  return ZC_OK;
}

int restore_replay(ResolveScratch* s, const zc_restore_plan* pl, const void* const* slot_base, size_t n_slots,
                   void* d_out, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  int rc = first_use(s, st, err);
  if (rc != ZC_OK) return rc;
  const uint64_t n = pl->n_entries;
  if (!n || !pl->length) return ZC_OK;
  RCK(s->pc.ensure(n));
  RCK(s->pstart.ensure(n + 1));
  RCK(s->base.ensure(n_slots));
  RCK(s->tsum.ensure((n + kTile - 1) / kTile));
  {
    std::lock_guard<std::mutex> lock(pl->mu);
    if (!pl->resident) {  // a host-made plan: its lists go up once and stay
      RCK(pl->d_slot.ensure(n));
      RCK(pl->d_off.ensure(n));
      RCK(pl->d_size.ensure(n));
      RCK(pl->d_dst.ensure(n));
      RCK(hipMemcpyAsync(pl->d_slot.p, pl->slot.data(), 4 * n, hipMemcpyHostToDevice, st));
      RCK(hipMemcpyAsync(pl->d_off.p, pl->off.data(), 8 * n, hipMemcpyHostToDevice, st));
      RCK(hipMemcpyAsync(pl->d_size.p, pl->size.data(), 8 * n, hipMemcpyHostToDevice, st));
      RCK(hipMemcpyAsync(pl->d_dst.p, pl->dst.data(), 8 * n, hipMemcpyHostToDevice, st));
      RCK(hipStreamSynchronize(st));
      pl->resident = true;
    }
  }
  // after the work queued on the legacy default stream so far (the payloads' decode, the stream's replay)
  RCK(hipEventRecord(ev_in, nullptr));
  RCK(hipStreamWaitEvent(st, ev_in, 0));
  RsDev h = fresh_dev();
  RCK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
  RCK(hipMemcpyAsync(s->base.p, slot_base, 8 * n_slots, hipMemcpyHostToDevice, st));
  RCK(hipEventRecord(s->ev[0], st));
  zc_rp_pieces<<<grid_for(s, n), kBlock, 0, st>>>(pl->d_size.p, n, s->pc.p);
  rc = scan<uint64_t>(s, s->pc.p, n, s->pstart.p, true, &s->dev.p->total[1], st, err);
  if (rc != ZC_OK) return rc;
  RCK(hipGetLastError());
  // the piece count is the one word that comes back: it sizes the copy's grid
  RCK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  RCK(hipStreamSynchronize(st));
  const uint64_t pieces = h.total[1];
  if (pieces) {
    const uint64_t blocks = (pieces + kBlock / 64 - 1) / (kBlock / 64);
    const int grid = (int)std::min<uint64_t>(blocks, (uint64_t)s->cus * 64);
    zc_rp_copy<<<grid, kBlock, 0, st>>>(s->pstart.p, n, pieces, pl->d_slot.p, pl->d_off.p, pl->d_size.p, pl->d_dst.p,
                                        (const uint8_t* const*)s->base.p, (uint32_t)n_slots, (uint8_t*)d_out);
    RCK(hipGetLastError());
  }
  RCK(hipEventRecord(s->ev[1], st));
  RCK(hipStreamSynchronize(st));
  float ms = 0;
  RCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->times.replay_ms = ms;
  s->times.replay_pieces = pieces;
  return ZC_OK;
}

}  // namespace zc
