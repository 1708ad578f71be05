// zc_index.hip -- a repository's index files read on the GPU: decrypt, check,
// parse.  ChunkIndex::loadIndex (chunk_index.cc:26-79) reads every index file
// through IndexFile::Reader (index_file.cc:44-76): an AES-128-CBC stream with
// an Adler-32 around length-prefixed protobuf messages.  Here the files of a
// whole repository go through in one call and come out as the flat arrays
// zc_gc_input, Restorer and Adopter take.  zc_index_core.h is the format and
// the walkers; this file is their schedule.
//
//   decrypt   zc_aes.hip's CBC decrypt kernel, every file a chain (with a key)
//   frame     zc_index_frame_kernel    a wave per file: header to header through
//                                      an LDS tile; per bundle its id and where
//                                      its BundleInfo lies, per file its status,
//                                      bundle count and the stored Adler-32
//   adler     zc_lzo.hip's Adler-32 kernel over every framed file
//   records   zc_index_gather_kernel   the framed files' bundles, dense
//             zc_index_records_kernel<false, *> count: records and status per BundleInfo
//             zc_index_sums / _scan / _apply   exclusive scan of the counts
//             zc_index_records_kernel<true, *>  write: ids and sizes, dense, in reading order
//
// The record kernels take a list of BundleInfo extents, so the same pair
// serves unsealed bundle files (zc_bundle_info_parse).  Each pass is two
// launches: the short extents a lane each, the long ones a wave each: uniform
// hops from record to record through an LDS tile, then a lane per record for
// its fields.
//
// Every loop keeps the trip bound of its core loop or a count the host
// computed; every store is checked against a capacity the host computed, and
// a failed check sets a flag the host turns into ZC_ERR_STATE; no kernel
// waits on another wave, spins, or ends on a data value alone.  Waves of one
// workgroup share nothing but the launch: each has its own LDS tile and there
// is no workgroup barrier.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_index_core.h"

namespace zc {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// The LDS tile of a wave and the length from which a BundleInfo gets a whole
// wave: DESIGN 4.12 has the sweep of tools/index_rate.py they are read off;
// ZC_TEST_INDEX_TILE / ZC_TEST_INDEX_WAVE_MIN replace them in tests.
constexpr uint32_t kTileDefault = 4096;
constexpr uint32_t kTileMin = 128;  // > 15 + kHopLook + kRecordLook: a staged tile always holds the next record
constexpr uint32_t kTileMax = 16384;
constexpr uint32_t kWaveMinDefault = 2048;
constexpr uint32_t kScanTile = 1024;  // counts per workgroup of the scan

static_assert(kTileMin >= 16 + zcidx::kHopLook + zcidx::kRecordLook, "tile too small for one record");

struct FileDesc {
  uint64_t addr;  // absolute device address of the plaintext
  uint64_t size;
  uint64_t slot_first;  // its bundles' slots are [slot_first, slot_first + slot_cap)
  uint64_t slot_cap;
};
struct FileOut {
  int32_t status;  // zcidx::k*; kOk: the frames read cleanly up to the stored Adler-32
  uint32_t stored;
  uint64_t n_bundles;
  uint64_t adler_pos;
};
struct Ext {
  uint64_t addr;  // absolute device address of a BundleInfo's bytes
  uint32_t len;
  uint32_t pad;
};
struct IndexDev {
  uint32_t internal;  // bit 0: a bundle beyond its file's slots; bit 1: a record beyond its bundle's count or the arrays
  uint32_t pad;
};

__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// A wave's tile over the bytes [0, n) at g: tile byte t is byte lo + t.  lo
// keeps the tile's start 16-byte aligned in memory, so it may lie before g;
// such bytes, and those from n on, are never loaded.
struct Tile {
  const uint8_t* g;
  uint64_t n;
  uint8_t* lds;
  uint32_t bytes;
  int64_t lo;
  uint64_t hi;  // bytes [max(lo, 0), hi) are staged
  // all 64 lanes, uniformly: stage the tile that holds byte `at` (at < n)
  __device__ void stage(uint64_t at, uint32_t lane) {
    wave_lds_sync();  // the reads of the old tile are done
    const uintptr_t base = (uintptr_t)g;
    lo = (int64_t)at - (int64_t)((base + at) & 15);
    const uint64_t top = (uint64_t)(lo + (int64_t)bytes);
    hi = top < n ? top : n;
    const uint32_t chunks = (uint32_t)((hi - lo + 15) / 16);  // <= bytes / 16
    for (uint32_t c = lane; c < chunks; c += 64) {
      const int64_t rel = lo + 16 * (int64_t)c;
      uint4 v;
      if (rel >= 0 && (uint64_t)rel + 16 <= n) {
        v = *reinterpret_cast<const uint4*>(g + rel);
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int k = 0; k < 16; ++k) {
          const int64_t r = rel + k;
          if (r >= 0 && (uint64_t)r < n) w[k >> 2] |= (uint32_t)g[r] << (8 * (k & 3));
        }
        v = uint4{w[0], w[1], w[2], w[3]};
      }
      *reinterpret_cast<uint4*>(lds + 16 * c) = v;
    }
    wave_lds_sync();
  }
  __device__ bool holds(uint64_t a, uint64_t b) const { return (int64_t)a >= lo && b <= hi; }
};

// the frame walker's source: every lane asks for the same byte; a byte outside
// the tile brings the tile that holds it
struct UniformSrc {
  Tile* t;
  uint32_t lane;
  __device__ uint32_t byte(uint64_t i) const {
    if (!t->holds(i, i + 1)) t->stage(i, lane);
    return __builtin_amdgcn_readfirstlane((uint32_t)t->lds[(int64_t)i - t->lo]);
  }
};
// bytes the caller knows to be staged: the same for every lane, or a lane's own
struct StagedUniform {
  const Tile* t;
  __device__ uint32_t byte(uint64_t i) const {
    return __builtin_amdgcn_readfirstlane((uint32_t)t->lds[(int64_t)i - t->lo]);
  }
};
struct StagedLane {
  const Tile* t;
  __device__ uint32_t byte(uint64_t i) const { return t->lds[(int64_t)i - t->lo]; }
};

// a lane's own source over [0, n) at g: the aligned 16 bytes around the last
// byte asked for are kept in registers
struct WordSrc {
  const uint8_t* g;
  uint64_t n;
  mutable uintptr_t cur;  // the address of w's bytes (16-byte aligned), 1: none
  mutable uint32_t w[4];
  __device__ uint32_t byte(uint64_t i) const {
    const uintptr_t a = (uintptr_t)g + i, c = a & ~(uintptr_t)15;
    if (c != cur) {
      const uintptr_t first = (uintptr_t)g, last = first + n;
      if (c >= first && c + 16 <= last) {
        const uint4 v = *reinterpret_cast<const uint4*>(c);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
      } else {
        w[0] = w[1] = w[2] = w[3] = 0;
        for (int k = 0; k < 16; ++k)
          if (c + k >= first && c + k < last)
            w[k >> 2] |= (uint32_t) * reinterpret_cast<const uint8_t*>(c + k) << (8 * (k & 3));
      }
      cur = c;
    }
    const uint32_t j = (uint32_t)(a & 15), q = j >> 2;
    const uint32_t word = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
    return (word >> (8 * (j & 3))) & 0xff;
  }
};

template <class In>
__device__ inline uint64_t load_le64(const In& in, uint64_t off) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v |= (uint64_t)in.byte(off + k) << (8 * k);
  return v;
}

// ---- frames: a wave per file ----

__global__ __launch_bounds__(kBlock) void zc_index_frame_kernel(const FileDesc* __restrict__ files, uint32_t n,
                                                                int keyed, uint32_t tile_bytes,
                                                                FileOut* __restrict__ out, Ext* __restrict__ ext,
                                                                uint64_t* __restrict__ bid, IndexDev* dev) {
  extern __shared__ uint4 lds_all[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t waves = gridDim.x * kWaves;
  for (uint32_t fi = blockIdx.x * kWaves + wave; fi < n; fi += waves) {
    const FileDesc fd = files[fi];
    Tile tile{reinterpret_cast<const uint8_t*>((uintptr_t)fd.addr), fd.size,
              reinterpret_cast<uint8_t*>(lds_all) + (size_t)wave * tile_bytes, tile_bytes, 0, 0};
    const UniformSrc in{&tile, lane};
    zcidx::Frame f;
    FileOut o{};
    int rc = zcidx::frame_open(in, fd.size, keyed != 0, &f);
    if (rc == zcidx::kOk) {
      const uint64_t bound = zcidx::max_bundles(f.end - f.pos) + 1;  // and the terminator
      uint64_t b = 0;
      rc = zcidx::kTruncated;  // a walk that ran out of trips ran out of bytes
      for (uint64_t trip = 0; trip < bound; ++trip) {
        uint64_t id_off = 0, info_off = 0;
        uint32_t info_len = 0;
        const int r = zcidx::frame_next(in, &f, &id_off, &info_off, &info_len);
        if (r != zcidx::kFrameBundle) {
          rc = r;
          break;
        }
        if (b >= fd.slot_cap) {  // the host's bound: never
          if (lane == 0) atomicOr(&dev->internal, 1u);
          break;
        }
        const uint64_t i0 = load_le64(in, id_off), i1 = load_le64(in, id_off + 8), i2 = load_le64(in, id_off + 16);
        if (lane == 0) {
          const uint64_t s = fd.slot_first + b;
          ext[s] = Ext{fd.addr + info_off, info_len, 0};
          bid[3 * s] = i0;
          bid[3 * s + 1] = i1;
          bid[3 * s + 2] = i2;
        }
        ++b;
      }
      if (rc == zcidx::kFrameEnd) {
        rc = zcidx::kOk;
        o.adler_pos = f.pos;
        for (int k = 0; k < 4; ++k) o.stored |= in.byte(f.pos + k) << (8 * k);
      }
      o.n_bundles = b;
    }
    o.status = rc;
    if (lane == 0) out[fi] = o;
  }
}

// ---- the framed files' bundles, dense ----

// dense bundle j belongs to the file f with dfirst[f] <= j < dfirst[f + 1]
// and is its bundle j - dfirst[f]
__global__ __launch_bounds__(kBlock) void zc_index_gather_kernel(const uint64_t* __restrict__ dfirst, uint32_t nfiles,
                                                                 const uint64_t* __restrict__ slot_first,
                                                                 const Ext* __restrict__ ext,
                                                                 const uint64_t* __restrict__ bid, uint64_t nb,
                                                                 Ext* __restrict__ dext, uint64_t* __restrict__ dbid,
                                                                 uint32_t* __restrict__ file_of,
                                                                 uint32_t* __restrict__ kin) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nb; j += stride) {
    uint32_t lo = 0, hi = nfiles;  // the answer is in [lo, hi): dfirst[nfiles] = nb > j
    for (int it = 0; it < 33 && hi - lo > 1; it++) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (dfirst[mid] <= j)
        lo = mid;
      else
        hi = mid;
    }
    const uint64_t k = j - dfirst[lo], s = slot_first[lo] + k;
    dext[j] = ext[s];
    dbid[3 * j] = bid[3 * s];
    dbid[3 * j + 1] = bid[3 * s + 1];
    dbid[3 * j + 2] = bid[3 * s + 2];
    file_of[j] = lo;
    kin[j] = (uint32_t)(k < 0xffffffffull ? k : 0xffffffffull);
  }
}

// ---- records ----

struct RecOut {
  uint64_t* ids;    // 3 words per record
  uint32_t* sizes;
  uint64_t cap;     // records the arrays hold
};

// record `at` of the arrays, if it is bundle-record k < cnt
template <class In>
__device__ inline void store_record(const In& in, const RecOut& o, uint64_t at, uint32_t k, uint32_t cnt,
                                    uint64_t id_off, uint32_t size, IndexDev* dev) {
  if (k >= cnt || at >= o.cap) {
    atomicOr(&dev->internal, 2u);
    return;
  }
  o.ids[3 * at] = load_le64(in, id_off);
  o.ids[3 * at + 1] = load_le64(in, id_off + 8);
  o.ids[3 * at + 2] = load_le64(in, id_off + 16);
  o.sizes[at] = size;
}

struct CountSink {
  __device__ void operator()(uint32_t, uint64_t, uint32_t) const {}
};
struct WriteSink {
  const WordSrc* in;
  RecOut o;
  uint64_t first;
  uint32_t cnt;
  IndexDev* dev;
  __device__ void operator()(uint32_t k, uint64_t id_off, uint32_t size) const {
    store_record(*in, o, first + k, k, cnt, id_off, size, dev);
  }
};

// One long BundleInfo with the whole wave.  Returns its status; *count = the
// records before the first failure.  WRITE: record k goes to first + k.
template <bool WRITE>
__device__ inline int wave_records(Tile& tile, uint32_t lane, uint32_t len, const RecOut& o, uint64_t first,
                                   uint32_t cnt, IndexDev* dev, uint32_t* count) {
  const uint64_t end = len;
  const uint64_t look = zcidx::kHopLook + zcidx::kRecordLook;
  uint64_t pos = 0;
  uint32_t k = 0;
  int status = zcidx::kOk;
  // a trip that stages nothing reads a record (two bytes at least); one that
  // stages is followed by one that reads: len + 2 trips at most
  const uint64_t bound = (uint64_t)len + 2;
  for (uint64_t trip = 0; trip < bound && pos < end && status == zcidx::kOk; ++trip) {
    if (!tile.holds(pos, pos + look < end ? pos + look : end)) tile.stage(pos, lane);
    const StagedUniform uni{&tile};
    uint64_t my_body = 0;
    uint32_t my_len = 0, nb = 0;
    int hop_rc = zcidx::kOk;
    for (uint32_t j = 0; j < 64 && pos < end; ++j) {
      if (!tile.holds(pos, pos + look < end ? pos + look : end)) break;
      uint64_t p = pos, body = 0;
      uint32_t blen = 0;
      hop_rc = zcidx::record_hop(uni, p, end, &body, &blen);
      if (hop_rc != zcidx::kOk) break;
      if (lane == j) {
        my_body = body;
        my_len = blen;
      }
      pos = p;
      ++nb;
    }
    const StagedLane mine{&tile};
    uint64_t id_off = 0;
    uint32_t size = 0;
    int rc = zcidx::kOk;
    if (lane < nb) rc = zcidx::record_body(mine, my_body, my_len, &id_off, &size);
    const unsigned long long bad = __ballot(rc != zcidx::kOk);
    uint32_t good = nb;
    if (bad) {
      good = (uint32_t)__builtin_ctzll(bad);
      status = __shfl(rc, (int)good, 64);
    } else if (hop_rc != zcidx::kOk) {
      status = hop_rc;
    }
    if (WRITE && lane < good) store_record(mine, o, first + k + lane, k + lane, cnt, id_off, size, dev);
    k += good;
  }
  *count = k;
  return status;
}

// LONG false: a wave owns 64 consecutive extents and walks the short ones, a
// lane each.  LONG true: a wave per extent, for the long ones alone, so that
// no two of them wait for one wave.
template <bool WRITE, bool LONG>
__global__ __launch_bounds__(kBlock) void zc_index_records_kernel(const Ext* __restrict__ ext, uint64_t nb,
                                                                  uint32_t wave_min, uint32_t tile_bytes,
                                                                  uint32_t* __restrict__ cnt,
                                                                  uint8_t* __restrict__ est,
                                                                  const uint64_t* __restrict__ bf, RecOut o,
                                                                  IndexDev* dev) {
  extern __shared__ uint4 lds_all[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t groups = (nb + 63) / 64, waves = (uint64_t)gridDim.x * kWaves;
  if (LONG) {
    for (uint64_t e = (uint64_t)blockIdx.x * kWaves + wave; e < nb; e += waves) {
      const Ext x = ext[e];  // every lane the same
      if (x.len < wave_min) continue;
      uint32_t want = 0;
      uint64_t first = 0;
      if (WRITE) {
        if (est[e] != zcidx::kOk) continue;
        want = cnt[e];
        first = bf[e];
      }
      Tile tile{reinterpret_cast<const uint8_t*>((uintptr_t)x.addr), x.len,
                reinterpret_cast<uint8_t*>(lds_all) + (size_t)wave * tile_bytes, tile_bytes, 0, 0};
      uint32_t count = 0;
      const int rc = wave_records<WRITE>(tile, lane, x.len, o, first, want, dev, &count);
      if (lane == 0) {
        if (WRITE) {
          if (rc != zcidx::kOk || count != want) atomicOr(&dev->internal, 2u);
        } else {
          cnt[e] = rc == zcidx::kOk ? count : 0;
          est[e] = (uint8_t)rc;
        }
      }
    }
    return;
  }
  for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < groups; g += waves) {
    const uint64_t e = g * 64 + lane;
    const bool have = e < nb;
    Ext x{0, 0, 0};
    if (have) x = ext[e];
    uint32_t want = 0;
    uint64_t first = 0;
    bool walk = have;
    if (WRITE && have) {
      walk = est[e] == zcidx::kOk;
      want = cnt[e];
      first = bf[e];
    }
    const bool is_long = walk && x.len >= wave_min;
    if (walk && !is_long) {
      const WordSrc in{reinterpret_cast<const uint8_t*>((uintptr_t)x.addr), x.len, 1, {0, 0, 0, 0}};
      uint32_t count = 0;
      int rc;
      if (WRITE) {
        WriteSink sink{&in, o, first, want, dev};
        rc = zcidx::walk_records(in, 0, x.len, sink, &count);
        if (rc != zcidx::kOk || count != want) atomicOr(&dev->internal, 2u);
      } else {
        CountSink sink;
        rc = zcidx::walk_records(in, 0, x.len, sink, &count);
        cnt[e] = rc == zcidx::kOk ? count : 0;
        est[e] = (uint8_t)rc;
      }
    }
  }
}

// per file, the first bundle whose BundleInfo did not read cleanly: the
// smallest (bundle in file << 8 | status)
__global__ __launch_bounds__(kBlock) void zc_index_first_bad_kernel(const uint8_t* __restrict__ est,
                                                                    const uint32_t* __restrict__ file_of,
                                                                    const uint32_t* __restrict__ kin, uint64_t nb,
                                                                    unsigned long long* __restrict__ first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nb; j += stride)
    if (est[j] != zcidx::kOk) atomicMin(&first_bad[file_of[j]], (unsigned long long)kin[j] << 8 | est[j]);
}

// ---- exclusive scan of the counts: bf[j] = sum of cnt[0 .. j), bf[nb] = the total ----

__device__ inline uint64_t block_sum(uint64_t v, uint64_t* ls) {
  const uint32_t t = threadIdx.x;
  ls[t] = v;
  __syncthreads();
  for (uint32_t d = kBlock / 2; d >= 1; d >>= 1) {
    if (t < d) ls[t] += ls[t + d];
    __syncthreads();
  }
  const uint64_t s = ls[0];
  __syncthreads();
  return s;
}
// exclusive prefix of v over the block's threads
__device__ inline uint64_t block_prefix(uint64_t v, uint64_t* ls) {
  const uint32_t t = threadIdx.x;
  ls[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    const uint64_t a = t >= d ? ls[t - d] : 0;
    __syncthreads();
    ls[t] += a;
    __syncthreads();
  }
  const uint64_t r = ls[t] - v;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kBlock) void zc_index_sums_kernel(const uint32_t* __restrict__ cnt, uint64_t nb,
                                                               uint32_t ntiles, uint64_t* __restrict__ tsum) {
  __shared__ uint64_t ls[kBlock];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kScanTile + threadIdx.x * (kScanTile / kBlock);
    uint64_t v = 0;
    for (uint32_t k = 0; k < kScanTile / kBlock; k++)
      if (base + k < nb) v += cnt[base + k];
    const uint64_t s = block_sum(v, ls);
    if (threadIdx.x == 0) tsum[tile] = s;
  }
}
// one workgroup: the tiles' sums to exclusive prefixes, 256 at a time
__global__ __launch_bounds__(kBlock) void zc_index_scan_kernel(uint64_t* __restrict__ tsum, uint32_t ntiles,
                                                               uint64_t* __restrict__ total) {
  __shared__ uint64_t ls[kBlock];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < ntiles; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < ntiles ? tsum[i] : 0;
    const uint64_t p = block_prefix(v, ls);
    const uint64_t s = block_sum(v, ls);
    if (i < ntiles) tsum[i] = carry + p;
    carry += s;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(kBlock) void zc_index_apply_kernel(const uint32_t* __restrict__ cnt, uint64_t nb,
                                                                uint32_t ntiles, const uint64_t* __restrict__ tsum,
                                                                uint64_t* __restrict__ bf) {
  __shared__ uint64_t ls[kBlock];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kScanTile + threadIdx.x * (kScanTile / kBlock);
    uint64_t v = 0;
    for (uint32_t k = 0; k < kScanTile / kBlock; k++)
      if (base + k < nb) v += cnt[base + k];
    uint64_t at = tsum[tile] + block_prefix(v, ls);
    for (uint32_t k = 0; k < kScanTile / kBlock; k++)
      if (base + k < nb) {
        bf[base + k] = at;
        at += cnt[base + k];
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

int arg_error(std::string& err, const std::string& msg) {
  err = msg;
  return ZC_ERR_ARG;
}
int hip_error(std::string& err, hipError_t e, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  err = hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZC_ERR_NOMEM : ZC_ERR_HIP;
}
#define ICK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

uint32_t env_u32(const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) {
  const char* e = getenv(name);
  if (!e || !*e) return dflt;
  const unsigned long v = strtoul(e, nullptr, 10);
  return (uint32_t)std::min<unsigned long>(std::max<unsigned long>(v, lo), hi);
}

}  // namespace

struct IndexScratch {
  Buf<uint8_t> plain, up;  // the decrypted files; the host forms' upload
  Buf<FileDesc> fdesc;
  Buf<FileOut> fout;
  Buf<Ext> ext, dext;
  Buf<uint64_t> bid, dfirst, slot_first, tsum, total;
  Buf<uint32_t> file_of, kin, cnt;
  Buf<uint8_t> est;
  Buf<unsigned long long> first_bad;
  Buf<IndexDev> dev;
  hipEvent_t ev[6] = {};
  int cus = 0;
  IndexTimes times{};
  ~IndexScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

IndexScratch* index_scratch_new() { return new IndexScratch(); }
void index_scratch_free(IndexScratch* s) { delete s; }
const IndexTimes* index_times(const IndexScratch* s) { return &s->times; }

}  // namespace zc

// the loaded arrays: device memory of their own, so a set outlives the
// scratch of the call that made it
struct zc_index_set {
  int device = 0;
  uint64_t n_files = 0, n_bundles = 0, n_records = 0;
  zc::Buf<uint64_t> ids, bundle_ids, bundle_first;
  zc::Buf<uint32_t> sizes;
  std::vector<uint64_t> index_first;
  std::vector<int32_t> status;
};

namespace zc {

namespace {

struct Tuning {
  uint32_t tile, wave_min;
  size_t lds;
};
Tuning tuning() {
  Tuning t;
  t.tile = env_u32("ZC_TEST_INDEX_TILE", kTileDefault, kTileMin, kTileMax) / 16 * 16;
  t.wave_min = env_u32("ZC_TEST_INDEX_WAVE_MIN", kWaveMinDefault, 1, 0xffffffffu);
  t.lds = (size_t)t.tile * kWaves;
  return t;
}

int first_use(IndexScratch* s, hipStream_t st, std::string& err) {
  if (s->cus) return ZC_OK;
  int dev = 0, cus = 0;
  ICK(hipGetDevice(&dev));
  ICK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  for (hipEvent_t& e : s->ev) ICK(hipEventCreate(&e));
  s->cus = std::max(cus, 1);
  return ZC_OK;
}

int grid_items(const IndexScratch* s, uint64_t items) {
  const uint64_t blocks = (items + kBlock - 1) / kBlock;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * 16));
}
int grid_waves(const IndexScratch* s, uint64_t wave_items) {
  const uint64_t blocks = (wave_items + kWaves - 1) / kWaves;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * 8));
}

// count pass over dext[0 .. nb): cnt and est
void launch_count(IndexScratch* s, uint64_t nb, const Tuning& t, hipStream_t st) {
  hipLaunchKernelGGL((zc_index_records_kernel<false, false>), dim3(grid_waves(s, (nb + 63) / 64)), dim3(kBlock), 0,
                     st, s->dext.p, nb, t.wave_min, t.tile, s->cnt.p, s->est.p, (const uint64_t*)nullptr,
                     RecOut{nullptr, nullptr, 0}, s->dev.p);
  hipLaunchKernelGGL((zc_index_records_kernel<false, true>), dim3(grid_waves(s, nb)), dim3(kBlock), t.lds, st,
                     s->dext.p, nb, t.wave_min, t.tile, s->cnt.p, s->est.p, (const uint64_t*)nullptr,
                     RecOut{nullptr, nullptr, 0}, s->dev.p);
}
// cnt[0 .. nb) -> bf[0 .. nb], the total also in s->total
void launch_scan(IndexScratch* s, uint64_t nb, uint64_t* bf, hipStream_t st) {
  const uint32_t ntiles = (uint32_t)((nb + kScanTile - 1) / kScanTile);
  const int g = (int)std::max<uint32_t>(1, std::min<uint32_t>(ntiles, (uint32_t)s->cus * 16));
  hipLaunchKernelGGL(zc_index_sums_kernel, dim3(g), dim3(kBlock), 0, st, s->cnt.p, nb, ntiles, s->tsum.p);
  hipLaunchKernelGGL(zc_index_scan_kernel, dim3(1), dim3(kBlock), 0, st, s->tsum.p, ntiles, s->total.p);
  hipLaunchKernelGGL(zc_index_apply_kernel, dim3(g), dim3(kBlock), 0, st, s->cnt.p, nb, ntiles, s->tsum.p, bf);
}
void launch_write(IndexScratch* s, uint64_t nb, const Tuning& t, const uint64_t* bf, uint64_t* ids, uint32_t* sizes,
                  uint64_t cap, hipStream_t st) {
  hipLaunchKernelGGL((zc_index_records_kernel<true, false>), dim3(grid_waves(s, (nb + 63) / 64)), dim3(kBlock), 0,
                     st, s->dext.p, nb, t.wave_min, t.tile, s->cnt.p, s->est.p, bf, RecOut{ids, sizes, cap}, s->dev.p);
  hipLaunchKernelGGL((zc_index_records_kernel<true, true>), dim3(grid_waves(s, nb)), dim3(kBlock), t.lds, st,
                     s->dext.p, nb, t.wave_min, t.tile, s->cnt.p, s->est.p, bf, RecOut{ids, sizes, cap}, s->dev.p);
}

int ensure_records(IndexScratch* s, uint64_t nb, hipStream_t st, std::string& err) {
  ICK(s->cnt.ensure(nb));
  ICK(s->est.ensure(nb));
  ICK(s->tsum.ensure((nb + kScanTile - 1) / kScanTile));
  ICK(s->total.ensure(1));
  ICK(s->dev.ensure(1));
  return ZC_OK;
}

int order_after_default(hipEvent_t ev_in, hipStream_t st, std::string& err) {
  if (!ev_in) return ZC_OK;
  ICK(hipEventRecord(ev_in, nullptr));
  ICK(hipStreamWaitEvent(st, ev_in, 0));
  return ZC_OK;
}

}  // namespace

int index_validate(const uint8_t* key, bool host, const void* files, const uint64_t* file_off,
                   const uint64_t* file_size, size_t n, zc_index_set** set, std::string& err) {
  if (!set) return arg_error(err, "null set pointer");
  if (n && (!files || !file_off || !file_size)) return arg_error(err, "null pointer");
  if (n > 0x7fffffffull) return arg_error(err, "more than 2^31 files");
  if (key && !host && ((uintptr_t)files & 15)) return arg_error(err, "a base pointer is not 16-byte aligned");
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (file " + std::to_string(i) + ")";
    if (key && file_off[i] % 16) return arg_error(err, "an offset that is not 16-byte aligned" + at);
    const uint64_t a = (uint64_t)(uintptr_t)files + file_off[i];
    if (a + file_size[i] < a) return arg_error(err, "an extent wraps the address space" + at);
  }
  return ZC_OK;
}

int index_load(IndexScratch* s, AesScratch* aes, LzoScratch* lz, bool host, const uint8_t* key, const void* files,
               const uint64_t* file_off, const uint64_t* file_size, size_t n, zc_index_set** out, hipEvent_t ev_in,
               hipStream_t st, std::string& err) {
  const auto t_call = Clock::now();
  const bool keyed = key != nullptr;
  const Tuning tune = tuning();
  s->times = IndexTimes{};
  int rc = first_use(s, st, err);
  if (rc) return rc;
  std::unique_ptr<zc_index_set> set(new zc_index_set());
  ICK(hipGetDevice(&set->device));
  set->n_files = n;
  set->index_first.assign(n + 1, 0);
  set->status.assign(n, zcidx::kOk);
  if (!n) {
    *out = set.release();
    s->times.total_ms = ms_between(t_call, Clock::now());
    return ZC_OK;
  }
  // where the bytes lie
  const uint8_t* d_files = (const uint8_t*)files;
  uint64_t f_lo = 0;
  if (host) {
    uint64_t hi = 0;
    f_lo = ~0ull;
    for (size_t i = 0; i < n; i++)
      if (file_size[i]) {
        f_lo = std::min(f_lo, file_off[i]);
        hi = std::max(hi, file_off[i] + file_size[i]);
      }
    if (f_lo > hi) f_lo = hi = 0;
    f_lo &= ~15ull;  // keeps every offset's alignment
    ICK(s->up.ensure(hi - f_lo));
    if (hi > f_lo) ICK(hipMemcpyAsync(s->up.p, (const uint8_t*)files + f_lo, hi - f_lo, hipMemcpyHostToDevice, st));
    d_files = s->up.p;
  } else {
    rc = order_after_default(ev_in, st, err);
    if (rc) return rc;
  }
  // ---- decrypt: every file of a legal size is one chain from the zero IV ----
  ICK(hipEventRecord(s->ev[0], st));
  std::vector<FileDesc> fd(n);
  std::vector<uint64_t> slot_first(n + 1, 0);
  if (keyed) {
    std::vector<uint64_t> in_off, len, out_off;
    uint64_t pos = 0;
    for (size_t i = 0; i < n; i++) {
      fd[i].addr = pos;  // an offset until the buffer is made
      if (file_size[i] && file_size[i] % 16 == 0) {
        in_off.push_back(file_off[i] - f_lo);
        len.push_back(file_size[i]);
        out_off.push_back(pos);
        pos += file_size[i];
      }
    }
    ICK(s->plain.ensure(pos));
    for (size_t i = 0; i < n; i++) fd[i].addr += (uint64_t)(uintptr_t)s->plain.p;
    if (!len.empty()) {
      rc = aes_cbc(aes, true, false, key, d_files, in_off.data(), len.data(), len.size(), nullptr, s->plain.p,
                   out_off.data(), nullptr, st, err);
      if (rc) return rc;
    }
  } else {
    for (size_t i = 0; i < n; i++) fd[i].addr = (uint64_t)(uintptr_t)d_files + file_off[i] - f_lo;
  }
  for (size_t i = 0; i < n; i++) {
    fd[i].size = file_size[i];
    fd[i].slot_first = slot_first[i];
    fd[i].slot_cap = zcidx::max_bundles(file_size[i]);
    slot_first[i + 1] = slot_first[i] + fd[i].slot_cap;
  }
  const uint64_t slots = slot_first[n];
  // ---- frames ----
  ICK(s->fdesc.ensure(n));
  ICK(s->fout.ensure(n));
  ICK(s->ext.ensure(slots));
  ICK(s->bid.ensure(3 * slots));
  ICK(s->slot_first.ensure(n + 1));
  ICK(s->dfirst.ensure(n + 1));
  ICK(s->first_bad.ensure(n));
  ICK(s->dev.ensure(1));
  const IndexDev zero{};
  ICK(hipMemcpyAsync(s->fdesc.p, fd.data(), n * sizeof(FileDesc), hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(s->slot_first.p, slot_first.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(s->dev.p, &zero, sizeof zero, hipMemcpyHostToDevice, st));
  ICK(hipEventRecord(s->ev[1], st));
  hipLaunchKernelGGL(zc_index_frame_kernel, dim3(grid_waves(s, n)), dim3(kBlock), tune.lds, st, s->fdesc.p,
                     (uint32_t)n, keyed ? 1 : 0, tune.tile, s->fout.p, s->ext.p, s->bid.p, s->dev.p);
  ICK(hipGetLastError());
  ICK(hipEventRecord(s->ev[2], st));
  std::vector<FileOut> fo(n);
  IndexDev h{};
  ICK(hipMemcpyAsync(fo.data(), s->fout.p, n * sizeof(FileOut), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  if (h.internal) {
    err = "a file framed more bundles than its bytes can hold (internal error)";
    return ZC_ERR_STATE;
  }
  for (size_t i = 0; i < n; i++) {
    set->status[i] = fo[i].status;
    if (fo[i].n_bundles > fd[i].slot_cap) {
      err = "a bundle count over its file's bound (internal error)";
      return ZC_ERR_STATE;
    }
  }
  // ---- the Adler-32 of every framed file ----
  ICK(hipEventRecord(s->ev[3], st));
  {
    std::vector<uint64_t> aoff, alen;
    std::vector<size_t> who;
    const uint64_t base = keyed ? (uint64_t)(uintptr_t)s->plain.p : (uint64_t)(uintptr_t)d_files;
    for (size_t i = 0; i < n; i++)
      if (fo[i].status == zcidx::kOk) {
        who.push_back(i);
        aoff.push_back(fd[i].addr - base);
        alen.push_back(fo[i].adler_pos);
      }
    std::vector<uint32_t> ad(who.size());
    ICK(lzo_adler32(lz, (const uint8_t*)(uintptr_t)base, aoff.data(), alen.data(), who.size(), ad.data(), st));
    for (size_t k = 0; k < who.size(); k++)
      if (ad[k] != fo[who[k]].stored) set->status[who[k]] = zcidx::kBadAdler;
  }
  ICK(hipEventRecord(s->ev[4], st));
  // ---- records: every framed bundle dense, counted -- also those a file
  // framed before its walk failed, since a bad record in one of them is met
  // first; then a second round over the good files alone, if any was bad ----
  uint64_t B = 0;
  for (int round = 0; round < 2; round++) {
    std::vector<uint64_t> dfirst(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
      const bool in = round == 0 || set->status[i] == zcidx::kOk;
      dfirst[i + 1] = dfirst[i] + (in ? fo[i].n_bundles : 0);
    }
    B = dfirst[n];
    if (B >= 0xffffffffull) return arg_error(err, "2^32 - 1 bundles or more");
    rc = ensure_records(s, B, st, err);
    if (rc) return rc;
    ICK(s->dext.ensure(B));
    ICK(set->bundle_ids.ensure(3 * B));
    ICK(s->file_of.ensure(B));
    ICK(s->kin.ensure(B));
    bool again = false;
    if (B) {
      ICK(hipMemcpyAsync(s->dfirst.p, dfirst.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
      ICK(hipMemsetAsync(s->first_bad.p, 0xff, n * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(zc_index_gather_kernel, dim3(grid_items(s, B)), dim3(kBlock), 0, st, s->dfirst.p,
                         (uint32_t)n, s->slot_first.p, s->ext.p, s->bid.p, B, s->dext.p, set->bundle_ids.p,
                         s->file_of.p, s->kin.p);
      launch_count(s, B, tune, st);
      hipLaunchKernelGGL(zc_index_first_bad_kernel, dim3(grid_items(s, B)), dim3(kBlock), 0, st, s->est.p,
                         s->file_of.p, s->kin.p, B, s->first_bad.p);
      ICK(hipGetLastError());
      std::vector<unsigned long long> fb(n);
      ICK(hipMemcpyAsync(fb.data(), s->first_bad.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      ICK(hipStreamSynchronize(st));
      for (size_t i = 0; i < n; i++)
        if (fb[i] != ~0ull) {
          if (round == 1) {
            err = "a bundle read cleanly once and not twice (internal error)";
            return ZC_ERR_STATE;
          }
          // a bad record comes before the Adler-32, and before whatever ended the frame walk
          set->status[i] = (int32_t)(fb[i] & 0xff);
        }
    }
    for (size_t i = 0; i < n && !again; i++) again = fo[i].n_bundles && set->status[i] != zcidx::kOk;
    if (round == 0 && !again) {
      set->index_first = dfirst;
      break;
    }
    if (round == 1) set->index_first = dfirst;
  }
  set->n_bundles = B;
  // ---- scan, write ----
  ICK(set->bundle_first.ensure(B + 1));
  uint64_t N = 0;
  if (B) {
    launch_scan(s, B, set->bundle_first.p, st);
    ICK(hipGetLastError());
    ICK(hipMemcpyAsync(&N, s->total.p, 8, hipMemcpyDeviceToHost, st));
    ICK(hipStreamSynchronize(st));
    uint64_t bound = 0;
    for (size_t i = 0; i < n; i++) bound += zcidx::max_records(file_size[i]);
    if (N > bound) {
      err = "more records than the files' bytes can hold (internal error)";
      return ZC_ERR_STATE;
    }
  }
  if (N >= 0xffffffffull) return arg_error(err, "2^32 - 1 records or more");
  ICK(hipMemcpyAsync(set->bundle_first.p + B, &N, 8, hipMemcpyHostToDevice, st));  // N lives past the sync below
  set->n_records = N;
  ICK(set->ids.ensure(3 * N));
  ICK(set->sizes.ensure(N));
  if (N) {
    launch_write(s, B, tune, set->bundle_first.p, set->ids.p, set->sizes.p, N, st);
    ICK(hipGetLastError());
  }
  ICK(hipEventRecord(s->ev[5], st));
  ICK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  if (h.internal) {
    err = "the write pass did not repeat the count pass (internal error)";
    return ZC_ERR_STATE;
  }
  float ms = 0;
  ICK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->times.decrypt_ms = ms;
  ICK(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
  s->times.frame_ms = ms;
  ICK(hipEventElapsedTime(&ms, s->ev[3], s->ev[4]));
  s->times.adler_ms = ms;
  ICK(hipEventElapsedTime(&ms, s->ev[4], s->ev[5]));
  s->times.records_ms = ms;
  s->times.total_ms = ms_between(t_call, Clock::now());
  *out = set.release();
  return ZC_OK;
}

int info_validate(bool host, const void* plain, const uint64_t* info_off, const uint64_t* info_len, size_t n,
                  const uint64_t* bundle_first, const uint8_t* status, const uint64_t* n_records, std::string& err) {
  if (!n_records) return arg_error(err, "null n_records");
  if (n && (!plain || !info_off || !info_len || !bundle_first || !status)) return arg_error(err, "null pointer");
  if (n >= 0xffffffffull) return arg_error(err, "2^32 - 1 bundles or more");
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (bundle " + std::to_string(i) + ")";
    if (info_len[i] > 0xffffffffull) return arg_error(err, "a BundleInfo of 2^32 bytes or more" + at);
    const uint64_t a = (uint64_t)(uintptr_t)plain + info_off[i];
    if (a + info_len[i] < a) return arg_error(err, "an extent wraps the address space" + at);
  }
  return ZC_OK;
}

int info_parse(IndexScratch* s, bool host, const void* plain, const uint64_t* info_off, const uint64_t* info_len,
               size_t n, uint8_t* ids, uint32_t* sizes, uint64_t cap, uint64_t* bundle_first, uint8_t* status,
               uint64_t* n_records, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  const auto t_call = Clock::now();
  const Tuning tune = tuning();
  s->times = IndexTimes{};
  *n_records = 0;
  if (!n) return ZC_OK;
  int rc = first_use(s, st, err);
  if (rc) return rc;
  const uint8_t* d_plain = (const uint8_t*)plain;
  uint64_t lo = 0;
  if (host) {
    uint64_t hi = 0;
    lo = ~0ull;
    for (size_t i = 0; i < n; i++)
      if (info_len[i]) {
        lo = std::min(lo, info_off[i]);
        hi = std::max(hi, info_off[i] + info_len[i]);
      }
    if (lo > hi) lo = hi = 0;
    ICK(s->up.ensure(hi - lo));
    if (hi > lo) ICK(hipMemcpyAsync(s->up.p, (const uint8_t*)plain + lo, hi - lo, hipMemcpyHostToDevice, st));
    d_plain = s->up.p;
  } else {
    rc = order_after_default(ev_in, st, err);
    if (rc) return rc;
  }
  std::vector<Ext> ext(n);
  uint64_t bound = 0;
  for (size_t i = 0; i < n; i++) {
    ext[i] = Ext{info_len[i] ? (uint64_t)(uintptr_t)d_plain + info_off[i] - lo : 0, (uint32_t)info_len[i], 0};
    bound += zcidx::max_records(info_len[i]);
  }
  rc = ensure_records(s, n, st, err);
  if (rc) return rc;
  ICK(s->dext.ensure(n));
  ICK(s->dfirst.ensure(n + 1));  // the scan's output
  const IndexDev zero{};
  ICK(hipMemcpyAsync(s->dext.p, ext.data(), n * sizeof(Ext), hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(s->dev.p, &zero, sizeof zero, hipMemcpyHostToDevice, st));
  ICK(hipEventRecord(s->ev[4], st));
  launch_count(s, n, tune, st);
  launch_scan(s, n, s->dfirst.p, st);
  ICK(hipGetLastError());
  uint64_t N = 0;
  ICK(hipMemcpyAsync(&N, s->total.p, 8, hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(status, s->est.p, n, hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(bundle_first, s->dfirst.p, n * 8, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  bundle_first[n] = N;
  *n_records = N;
  if (N > bound) {
    err = "more records than the bytes can hold (internal error)";
    return ZC_ERR_STATE;
  }
  if (N > cap) {
    char msg[120];
    snprintf(msg, sizeof msg, "%llu records, room for %llu", (unsigned long long)N, (unsigned long long)cap);
    return arg_error(err, msg);
  }
  if (N) {
    if (!ids || !sizes) return arg_error(err, "null record arrays");
    // the record arrays of this call: the decrypt buffer's room, unused here
    ICK(s->plain.ensure(28 * N + 8));
    uint64_t* d_ids = reinterpret_cast<uint64_t*>(s->plain.p);
    uint32_t* d_sizes = reinterpret_cast<uint32_t*>(s->plain.p + 24 * N);
    launch_write(s, n, tune, s->dfirst.p, d_ids, d_sizes, N, st);
    ICK(hipGetLastError());
    ICK(hipEventRecord(s->ev[5], st));
    IndexDev h{};
    ICK(hipMemcpyAsync(ids, d_ids, 24 * N, hipMemcpyDeviceToHost, st));
    ICK(hipMemcpyAsync(sizes, d_sizes, 4 * N, hipMemcpyDeviceToHost, st));
    ICK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
    ICK(hipStreamSynchronize(st));
    if (h.internal) {
      err = "the write pass did not repeat the count pass (internal error)";
      return ZC_ERR_STATE;
    }
  } else {
    ICK(hipEventRecord(s->ev[5], st));
    ICK(hipStreamSynchronize(st));
  }
  float ms = 0;
  ICK(hipEventElapsedTime(&ms, s->ev[4], s->ev[5]));
  s->times.records_ms = ms;
  s->times.total_ms = ms_between(t_call, Clock::now());
  return ZC_OK;
}

// ---- the set ----

namespace {
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
}  // namespace

void index_set_counts(const zc_index_set* set, uint64_t* n_files, uint64_t* n_bundles, uint64_t* n_records) {
  if (n_files) *n_files = set->n_files;
  if (n_bundles) *n_bundles = set->n_bundles;
  if (n_records) *n_records = set->n_records;
}

int index_set_fetch(const zc_index_set* set, uint8_t* ids, uint32_t* sizes, uint64_t* bundle_first,
                    uint8_t* bundle_ids, uint64_t* index_first, int32_t* status, std::string& err) {
  const uint64_t N = set->n_records, B = set->n_bundles, I = set->n_files;
  if (index_first) memcpy(index_first, set->index_first.data(), 8 * (I + 1));
  if (status && I) memcpy(status, set->status.data(), 4 * I);
  if (!I) {
    if (bundle_first) bundle_first[0] = 0;
    return ZC_OK;
  }
  SetDevice g(set->device);
  hipError_t e = hipSuccess;
  if (e == hipSuccess && ids && N) e = hipMemcpy(ids, set->ids.p, 24 * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && sizes && N) e = hipMemcpy(sizes, set->sizes.p, 4 * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && bundle_first) e = hipMemcpy(bundle_first, set->bundle_first.p, 8 * (B + 1), hipMemcpyDeviceToHost);
  if (e == hipSuccess && bundle_ids && B) e = hipMemcpy(bundle_ids, set->bundle_ids.p, 24 * B, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    err = hipGetErrorString(e);
    return ZC_ERR_HIP;
  }
  return ZC_OK;
}

void index_set_device(const zc_index_set* set, const void** d_ids, const void** d_sizes) {
  if (d_ids) *d_ids = set->n_records ? set->ids.p : nullptr;
  if (d_sizes) *d_sizes = set->n_records ? set->sizes.p : nullptr;
}

void index_set_arrays(const zc_index_set* set, int* device, const void** d_ids, const void** d_sizes,
                      const uint64_t** d_bundle_first) {
  *device = set->device;
  *d_ids = set->ids.p;
  *d_sizes = set->sizes.p;
  *d_bundle_first = set->bundle_first.p;
}

void index_set_destroy(zc_index_set* set) {
  SetDevice g(set->device);
  delete set;
}

// ---- the writer (host only) ----

namespace {
void put_varint(uint8_t*& p, uint32_t v) {
  for (int k = 0; k < 4 && v >= 0x80; ++k) {
    *p++ = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  *p++ = (uint8_t)v;
}
}  // namespace

int index_serialize(const uint8_t* ids, const uint32_t* sizes, const uint64_t* bundle_first,
                    const uint8_t* bundle_ids, uint64_t n_bundles, uint8_t* out, uint64_t cap, uint64_t* n_out,
                    std::string& err) {
  if (!n_out) return arg_error(err, "null n_out");
  if (n_bundles && (!bundle_first || !bundle_ids)) return arg_error(err, "null pointer");
  const uint64_t N = n_bundles ? bundle_first[n_bundles] : 0;
  if (N && (!ids || !sizes)) return arg_error(err, "null record arrays");
  if (n_bundles && bundle_first[0] != 0) return arg_error(err, "bundle_first[0] is not 0");
  uint64_t total = 3 + 1;  // FileHeader, the terminator
  std::vector<uint32_t> info_len(n_bundles);
  for (uint64_t b = 0; b < n_bundles; b++)  // before any record is read: every range lies inside [0, N]
    if (bundle_first[b + 1] < bundle_first[b]) return arg_error(err, "bundle_first decreases");
  for (uint64_t b = 0; b < n_bundles; b++) {
    uint64_t len = 0;
    for (uint64_t r = bundle_first[b]; r < bundle_first[b + 1]; r++) len += 2 + zcidx::record_len(sizes[r]);
    if (len > 0xffffffffull) return arg_error(err, "a BundleInfo of 2^32 bytes or more");
    info_len[b] = (uint32_t)len;
    total += 1 + 26 + zcidx::varint_len((uint32_t)len) + len;
  }
  *n_out = total;
  if (total > cap) {
    char msg[120];
    snprintf(msg, sizeof msg, "%llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    return arg_error(err, msg);
  }
  if (!out) return arg_error(err, "null output");
  uint8_t* p = out;
  *p++ = 2;
  *p++ = 0x08;
  *p++ = 1;
  for (uint64_t b = 0; b < n_bundles; b++) {
    *p++ = 26;
    *p++ = 0x0A;
    *p++ = 24;
    memcpy(p, bundle_ids + 24 * b, 24);
    p += 24;
    put_varint(p, info_len[b]);
    for (uint64_t r = bundle_first[b]; r < bundle_first[b + 1]; r++) {
      *p++ = 0x0A;
      *p++ = (uint8_t)zcidx::record_len(sizes[r]);
      *p++ = 0x0A;
      *p++ = 24;
      memcpy(p, ids + 24 * r, 24);
      p += 24;
      *p++ = 0x10;
      put_varint(p, sizes[r]);
    }
  }
  *p++ = 0;
  if ((uint64_t)(p - out) != total) {
    err = "the serialized size differs from the computed one (internal error)";
    return ZC_ERR_STATE;
  }
  return ZC_OK;
}

static_assert(ZC_INDEX_OK == zcidx::kOk && ZC_INDEX_BAD_SIZE == zcidx::kBadSize &&
                  ZC_INDEX_BAD_PADDING == zcidx::kBadPadding && ZC_INDEX_TRUNCATED == zcidx::kTruncated &&
                  ZC_INDEX_BAD_VERSION == zcidx::kBadVersion && ZC_INDEX_BAD_MESSAGE == zcidx::kBadMessage &&
                  ZC_INDEX_BAD_BUNDLE_ID == zcidx::kBadBundleId && ZC_INDEX_BAD_CHUNK_ID == zcidx::kBadChunkId &&
                  ZC_INDEX_BAD_ADLER == zcidx::kBadAdler,
              "index status codes");

}  // namespace zc
