// zc_instr.hip -- a BackupInstruction stream that lies in HBM, parsed there
// (zc_instr_core.h has the steps and their definitions; the host parser,
// zc_parse_instructions, is the reference):
//
//   zc_in_exits   a workgroup per tile of T positions: hop of every position
//                 into LDS, log2 T rounds of pointer doubling between two LDS
//                 buffers, the exits to HBM (4 bytes a position)
//   zc_in_chain   one lane from position 0 over the exits, tile to tile: each
//                 tile's first true message start, the only serial part
//   zc_in_count   a lane per tile: its true messages parsed, entries, messages
//                 and BYTES sizes counted, the smallest error kept
//   zc_in_scan    one workgroup: the tiles' entry counts to their places
//   zc_in_write   a lane per tile: the same walk, the 48-byte records written
//
// Every loop bound is a count the host fixed before the launch or follows from
// p < hop(p) and tile end <= exit(p) (zc_instr_core.h); every kernel is
// grid-stride; no kernel waits on another wave or workgroup, spins, or ends on
// a data value other than those two strictly growing positions.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_instr_core.h"

static_assert(sizeof(zc_instruction) == 48, "zc_instruction is written as twelve 32-bit words");
static_assert(ZC_INSTR_CHUNK == 0 && ZC_INSTR_BYTES == 1, "entry kinds (zcin::tile_walk)");

namespace zc {

namespace {

constexpr int kBlock = 256;
constexpr uint64_t kCountLimit = 0xffffffffull;

// what the kernels report, one copy on the device
struct InDev {
  unsigned long long error;  // zcin::err_key of the first error, or kNoError
  unsigned long long messages, bytes, entries;
  uint32_t chain_hops, pad;
};

// T: the tile, a power of two; rounds = log2 T; lds: two buffers of T words
__global__ __launch_bounds__(kBlock) void zc_in_exits(const uint8_t* __restrict__ d, uint32_t n, uint32_t T,
                                                      uint32_t rounds, uint32_t tiles, uint32_t* __restrict__ exits) {
  extern __shared__ uint32_t lds[];
  uint32_t* a = lds;
  uint32_t* b = lds + T;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // bound: tiles
    const uint32_t base = tile * T;                                    // tiles * T < n + T < 2^32 + T: see instr_parse
    const uint32_t cnt = min(T, n - base), end = base + cnt;
    for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) a[i] = zcin::hop_at(d, n, (uint64_t)base + i);
    __syncthreads();
    for (uint32_t r = 0; r < rounds; r++) {  // bound: rounds
      for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
        const uint32_t v = a[i];
        b[i] = v < end ? a[v - base] : v;  // base + i < v: v - base indexes the tile
      }
      __syncthreads();
      uint32_t* t = a;
      a = b;
      b = t;
    }
    for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) exits[base + i] = a[i];
    __syncthreads();  // a is the next tile's hop buffer
  }
}

// entry: kNone everywhere before the launch
__global__ __launch_bounds__(64) void zc_in_chain(const uint32_t* __restrict__ exits, uint32_t n, uint32_t shift,
                                                  uint32_t tiles, uint32_t* __restrict__ entry, InDev* dev) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t p = 0, hops = 0;
  // bound: tiles -- exits[p] is at or beyond the end of p's tile, so p's tile grows with every step
  for (uint32_t k = 0; k < tiles && p < n; k++) {
    entry[p >> shift] = p;
    hops++;
    const uint32_t x = exits[p];
    if (x == zcin::kBad) break;  // a length error on the chain: that tile's walk reports it
    p = x;
  }
  dev->chain_hops = hops;
}

__global__ __launch_bounds__(64) void zc_in_count(const uint8_t* __restrict__ d, uint32_t n, uint32_t T,
                                                  uint32_t tiles, const uint32_t* __restrict__ entry,
                                                  uint32_t* __restrict__ cnt, InDev* dev) {
  const uint32_t stride = gridDim.x * 64;
  for (uint32_t t = blockIdx.x * 64 + threadIdx.x; t < tiles; t += stride) {  // bound: tiles
    const uint32_t e = entry[t];
    uint32_t entries = 0;
    if (e != zcin::kNone) {
      const uint64_t end = min((uint64_t)n, ((uint64_t)t + 1) * T);
      const zcin::TileSum s = zcin::tile_walk(d, n, e, end, nullptr);
      entries = s.entries;
      if (s.messages) atomicAdd(&dev->messages, (unsigned long long)s.messages);
      if (s.bytes) atomicAdd(&dev->bytes, (unsigned long long)s.bytes);
      if (s.error != zcin::kNoError) atomicMin(&dev->error, (unsigned long long)s.error);
    }
    cnt[t] = entries;
  }
}

// one workgroup: place[t] = the entries of the tiles in front of t, 256 tiles a round
__global__ __launch_bounds__(kBlock) void zc_in_scan(const uint32_t* __restrict__ cnt, uint32_t tiles,
                                                     uint64_t* __restrict__ place, InDev* dev) {
  __shared__ uint64_t ls[kBlock / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += kBlock) {  // bound: ceil(tiles / 256)
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < tiles ? cnt[i] : 0;
    uint64_t inc = v;
    for (int k = 1; k < 64; k <<= 1) {
      const uint64_t up = __shfl_up((unsigned long long)inc, k, 64);
      if ((int)lane >= k) inc += up;
    }
    if (lane == 63) ls[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t w = 0; w < kBlock / 64; w++) {
      if (w < wave) before += ls[w];
      all += ls[w];
    }
    __syncthreads();  // ls is the next round's
    if (i < tiles) place[i] = carry + before + inc - v;
    carry += all;
  }
  if (threadIdx.x == 0) dev->entries = carry;
}

// ins: room for the entries zc_in_scan counted
__global__ __launch_bounds__(64) void zc_in_write(const uint8_t* __restrict__ d, uint32_t n, uint32_t T,
                                                  uint32_t tiles, const uint32_t* __restrict__ entry,
                                                  const uint32_t* __restrict__ cnt,
                                                  const uint64_t* __restrict__ place, uint32_t* __restrict__ ins) {
  const uint32_t stride = gridDim.x * 64;
  for (uint32_t t = blockIdx.x * 64 + threadIdx.x; t < tiles; t += stride) {  // bound: tiles
    const uint32_t e = entry[t];
    if (e == zcin::kNone || !cnt[t]) continue;
    const uint64_t end = min((uint64_t)n, ((uint64_t)t + 1) * T);
    // the walk zc_in_count made over the same bytes: cnt[t] records from place[t] on
    (void)zcin::tile_walk(d, n, e, end, ins + 12 * place[t]);
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

int hip_error(std::string& err, hipError_t e, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  err = hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZC_ERR_NOMEM : ZC_ERR_HIP;
}
#define ICK(x)                                           \
  do {                                                   \
    hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return hip_error(err, e_, st); \
  } while (0)

}  // namespace

}  // namespace zc

// the parsed stream: device memory of its own, read-only once made
struct zc_instr_set {
  int device = 0;
  uint64_t n_entries = 0, n_messages = 0, bytes_total = 0;
  zc::Buf<uint32_t> ins;  // twelve words an entry
};

namespace zc {

struct InstrScratch {
  Buf<uint32_t> exits, entry, cnt;
  Buf<uint64_t> place;
  Buf<InDev> dev;
  hipEvent_t ev[6] = {};
  int cus = 0;
  InstrTimes times{};
  ~InstrScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

InstrScratch* instr_scratch_new() { return new InstrScratch(); }
void instr_scratch_free(InstrScratch* s) { delete s; }
const InstrTimes* instr_times(const InstrScratch* s) { return &s->times; }

int instr_validate(const void* d_data, uint64_t n, zc_instr_set* const* out, std::string& err) {
  char msg[160];
  if (!out) {
    err = "null set pointer";
    return ZC_ERR_ARG;
  }
  if (n >= zcin::kSizeLimit) {
    snprintf(msg, sizeof msg, "a stream of %llu bytes: the size must stay below 2^32 - 1", (unsigned long long)n);
    err = msg;
    return ZC_ERR_ARG;
  }
  if (n && !d_data) {
    err = "null stream pointer";
    return ZC_ERR_ARG;
  }
  return ZC_OK;
}

int instr_parse(InstrScratch* s, int device, const void* d_data, uint64_t n64, zc_instr_set** out, hipEvent_t ev_in,
                hipStream_t st, std::string& err) {
  *out = nullptr;
  s->times = InstrTimes{};
  zc_instr_set* set = new zc_instr_set();
  struct Drop {
    zc_instr_set* p;
    ~Drop() { delete p; }
  } drop{set};
  set->device = device;
  if (!n64 || !d_data) {  // no stream: no entries, no device work
    drop.p = nullptr;
    *out = set;
    return ZC_OK;
  }
  if (!s->cus) {
    int cus = 0;
    ICK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    for (hipEvent_t& e : s->ev) ICK(hipEventCreate(&e));
    ICK(s->dev.ensure(1));
    s->cus = std::max(cus, 1);
  }
  const uint32_t n = (uint32_t)n64;  // below 2^32 - 1 (instr_validate)
  const uint32_t T = zcin::tile_for(getenv("ZC_TEST_INSTR_TILE")), shift = zcin::log2_of(T);
  const uint32_t tiles = (uint32_t)((n64 + T - 1) / T);  // the last tile's base, (tiles - 1) * T, is below n
  const uint8_t* d = (const uint8_t*)d_data;
  ICK(s->exits.ensure(n));
  ICK(s->entry.ensure(tiles));
  ICK(s->cnt.ensure(tiles));
  ICK(s->place.ensure(tiles));
  // after the work queued on the legacy default stream so far
  ICK(hipEventRecord(ev_in, nullptr));
  ICK(hipStreamWaitEvent(st, ev_in, 0));
  InDev h{};
  h.error = zcin::kNoError;
  ICK(hipMemcpyAsync(s->dev.p, &h, sizeof h, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(s->entry.p, 0xff, 4 * (size_t)tiles, st));  // kNone: no tile keeps an earlier call's entry
  const int lane_grid = (int)std::max<uint32_t>(1, std::min<uint32_t>((tiles + 63) / 64, (uint32_t)s->cus * 16));
  ICK(hipEventRecord(s->ev[0], st));
  zc_in_exits<<<(int)std::min<uint32_t>(tiles, (uint32_t)s->cus * 8), kBlock, 8 * (size_t)T, st>>>(
      d, n, T, shift, tiles, s->exits.p);
  ICK(hipEventRecord(s->ev[1], st));
  zc_in_chain<<<1, 64, 0, st>>>(s->exits.p, n, shift, tiles, s->entry.p, s->dev.p);
  ICK(hipEventRecord(s->ev[2], st));
  zc_in_count<<<lane_grid, 64, 0, st>>>(d, n, T, tiles, s->entry.p, s->cnt.p, s->dev.p);
  zc_in_scan<<<1, kBlock, 0, st>>>(s->cnt.p, tiles, s->place.p, s->dev.p);
  ICK(hipGetLastError());
  ICK(hipEventRecord(s->ev[3], st));
  ICK(hipMemcpyAsync(&h, s->dev.p, sizeof h, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  float ms[4] = {};
  ICK(hipEventElapsedTime(&ms[0], s->ev[0], s->ev[1]));
  ICK(hipEventElapsedTime(&ms[1], s->ev[1], s->ev[2]));
  ICK(hipEventElapsedTime(&ms[2], s->ev[2], s->ev[3]));
  s->times.exit_ms = ms[0];  // hop is the exit kernel's first step: it has no time of its own
  s->times.chain_ms = ms[1];
  s->times.emit_ms = ms[2];
  s->times.tiles = tiles;
  s->times.chain_hops = h.chain_hops;
  if (h.error != zcin::kNoError) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s at byte %llu", zcin::err_text((uint32_t)(h.error & 0xff)),
             (unsigned long long)(h.error >> 8));
    err = msg;
    return ZC_ERR_ARG;
  }
  if (h.entries >= kCountLimit) {
    char msg[160];
    snprintf(msg, sizeof msg, "%llu entries: the count must stay below 2^32 - 1", (unsigned long long)h.entries);
    err = msg;
    return ZC_ERR_ARG;
  }
  set->n_entries = h.entries;
  set->n_messages = h.messages;
  set->bytes_total = h.bytes;
  if (h.entries) {
    ICK(set->ins.ensure(12 * (size_t)h.entries));
    ICK(hipEventRecord(s->ev[4], st));
    zc_in_write<<<lane_grid, 64, 0, st>>>(d, n, T, tiles, s->entry.p, s->cnt.p, s->place.p, set->ins.p);
    ICK(hipGetLastError());
    ICK(hipEventRecord(s->ev[5], st));
    ICK(hipStreamSynchronize(st));
    ICK(hipEventElapsedTime(&ms[3], s->ev[4], s->ev[5]));
    s->times.emit_ms += ms[3];
  }
  drop.p = nullptr;
  *out = set;
  return ZC_OK;
}

void instr_set_counts(const zc_instr_set* set, uint64_t* n_entries, uint64_t* n_messages, uint64_t* bytes_total) {
  if (n_entries) *n_entries = set->n_entries;
  if (n_messages) *n_messages = set->n_messages;
  if (bytes_total) *bytes_total = set->bytes_total;
}

void instr_set_view(const zc_instr_set* set, int* device, const uint32_t** d_ins, uint64_t* n_entries,
                    uint64_t* bytes_total) {
  *device = set->device;
  *d_ins = set->ins.p;
  *n_entries = set->n_entries;
  *bytes_total = set->bytes_total;
}

int instr_set_fetch(const zc_instr_set* set, uint64_t first, uint64_t count, zc_instruction* out, std::string& err) {
  char msg[160];
  if (first > set->n_entries || count > set->n_entries - first) {
    snprintf(msg, sizeof msg, "entries [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)count,
             (unsigned long long)set->n_entries);
    err = msg;
    return ZC_ERR_ARG;
  }
  if (!count) return ZC_OK;
  if (!out) {
    err = "null output array";
    return ZC_ERR_ARG;
  }
  SetDevice g(set->device);
  const hipError_t e = hipMemcpy(out, set->ins.p + 12 * first, 48 * count, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    err = hipGetErrorString(e);
    return ZC_ERR_HIP;
  }
  return ZC_OK;
}

void instr_set_destroy(zc_instr_set* set) {
  SetDevice g(set->device);
  delete set;
}

}  // namespace zc
