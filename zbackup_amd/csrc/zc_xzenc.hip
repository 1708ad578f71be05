// zc_xzenc.hip -- LZMA bundles written on the GPU.  Bundle::Creator compresses a
// bundle's payload with lzma_easy_encoder(6, LZMA_CHECK_CRC64)
// (compression.cc:78-97); here the payloads of a whole backup go through in one
// call and the xz streams land in HBM, where zc_bundle_seal reads them.
// zc_xzenc_core.h is the format, the match rule and the parse; this file is
// their schedule.
//
//   check   zc_xzenc_check_kernel   a wave per payload: zc_xz_check_kernel's 64
//           slices, producing the CRC32 / CRC64 instead of comparing it.
//   match   zc_xzenc_match_kernel   a wave per payload, a lane per position, 64
//           positions a step: the lanes read the wave's hash table (positions
//           of earlier steps only), pick their candidates (zcxzenc::pick), store
//           them, and only then enter their own positions with an atomic
//           maximum, so a candidate depends on the payload alone.  An entry is
//           generation << 32 | position + 1: a wave's next payload, and the
//           next call, raise the generation instead of clearing the table.
//   code    zc_xzenc_code_kernel    a wave per payload.  The walk's state is
//           wave-uniform (scalar registers), the probabilities lie in the
//           wave's LDS region as the decode kernel lays them out, a match is
//           measured by the 64 lanes at once (the four rep distances in one
//           step, 16 lanes each), and the stream's bytes are stored 64 at a time.
//
// Every loop is the core's: one trip count fixed before the walk, constant
// counts, or sizes bounded by a chunk.  No wave waits on another, there is no
// workgroup barrier in the match and code kernels and no spin; the waves of a
// workgroup share nothing but the launch.  All stores are ordinary vector
// stores; the only atomics are the table's maxima.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_xz_core.h"
#include "zc_xz_dev.h"
#include "zc_xzenc_core.h"

namespace zc {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kBlocksPerCu = 2;  // 4 waves * 15,984 bytes of LDS a block: two blocks, eight waves a CU
constexpr uint64_t kTableEntries = 1ull << zcxzenc::kHashBits;

struct EncDesc {
  uint64_t pay_addr, pay_size;  // absolute device address of the payload
  uint64_t out_addr, out_cap;
  uint64_t cand_off;            // the payload's candidates (zcxzenc::pick's packing) begin at cand + cand_off
  uint64_t check;               // the payload's check value (the check kernel's)
};

// ---- the payload's check ----

__global__ __launch_bounds__(kBlock) void zc_xzenc_check_kernel(EncDesc* __restrict__ desc, uint32_t n,
                                                                uint32_t check_id) {
  __shared__ uint64_t t64[256];
  __shared__ uint32_t t32[256];
  t64[threadIdx.x] = zcxz::crc64_entry(threadIdx.x);
  t32[threadIdx.x] = zcxz::crc32_entry(threadIdx.x);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t waves = gridDim.x * kWaves;
  for (uint32_t i = blockIdx.x * kWaves + wave; i < n; i += waves) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>((uintptr_t)desc[i].pay_addr);
    const uint64_t size = desc[i].pay_size;
    uint64_t got;
    if (check_id == zcxz::kCheckCrc64)
      got = zcxz::crc64_finish_raw(wave_raw_crc<uint64_t>(p, size, t64, zcxz::kPoly64, lane), size);
    else
      got = zcxz::crc32_finish_raw(wave_raw_crc<uint32_t>(p, size, t32, zcxz::kPoly32, lane), size);
    if (lane == 0) desc[i].check = got;
  }
}

// ---- match finding ----

// a lane's own view of the payload
struct LaneSrc {
  const uint8_t* p;
  __device__ __forceinline__ uint32_t byte(uint64_t i) const { return p[i]; }
  __device__ __forceinline__ uint32_t word(uint64_t i) const {
    uint32_t w;
    __builtin_memcpy(&w, p + i, 4);
    return w;
  }
  __device__ __forceinline__ uint32_t match_len(uint64_t at, uint32_t d, uint32_t limit) const {
    uint32_t k = 0;
    bool same = true;
    for (; same && k + 4 <= limit;) {  // limit <= kNice
      same = word(at + k) == word(at + k - d);
      if (same) k += 4;
    }
    for (; k < limit && p[at + k] == p[at + k - d];) ++k;
    return k;
  }
};

// payload first + j for j < count, a wave each; a wave's table is the slot of its
// place in the grid, and its t-th payload of the launch runs under generation gen0 + t
__global__ __launch_bounds__(kBlock) void zc_xzenc_match_kernel(const EncDesc* __restrict__ desc, uint32_t first,
                                                                uint32_t count, uint64_t* __restrict__ tables,
                                                                uint32_t gen0, uint32_t* __restrict__ cand) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t waves = gridDim.x * kWaves;
  const uint32_t slot = blockIdx.x * kWaves + wave;
  uint64_t* table = tables + (uint64_t)slot * kTableEntries;
  uint32_t gen = gen0;
  for (uint32_t j = slot; j < count; j += waves, ++gen) {
    const EncDesc x = desc[first + j];
    const uint64_t n = x.pay_size;
    const LaneSrc in{reinterpret_cast<const uint8_t*>((uintptr_t)x.pay_addr)};
    uint32_t* c = cand + x.cand_off;
    const uint64_t tag = (uint64_t)gen << 32;
    for (uint64_t g = 0; g < n; g += 64) {
      const uint64_t p = g + lane;
      const bool valid = p + 4 <= n;
      uint64_t* e = table;
      uint32_t d = 0;
      if (valid) {
        e = table + zcxzenc::hash4(in.word(p));
        const uint64_t v = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t t1 = (v >> 32) == gen ? (v & 0xffffffffull) : 0;
        d = zcxzenc::pick(in, n, p, t1);
      }
      if (p < n) c[p] = d;
      // Every lane has its table entry (pick() used it) before any lane of this step enters
      // a position; the next step reads what this one entered.  The table is read and written
      // at the L2 only (an atomic load, an atomic maximum; no line of it lives in the CU's L1),
      // so ordering within the wave is all that is needed: the maxima are done when the
      // wave's memory counters are at zero.  No cache is written back or invalidated here.
      __builtin_amdgcn_wave_barrier();
      if (valid) __hip_atomic_fetch_max(e, tag | (p + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- coding ----

// the walk's view: every lane asks for the same thing, the answers are wave-uniform
// The bytes at p - 1 and p and the candidates come from two 64-entry windows held a lane
// each in registers, so the walk's steady state asks memory only for what lies behind p.
struct WaveSrc {
  const uint8_t* p;
  const uint32_t* c;
  uint64_t n;
  uint32_t lane;
  mutable uint64_t bw, cw;   // the windows hold bytes [bw, bw + 64) and candidates [cw, cw + 64); far away: none
  mutable uint32_t bv, cv;   // lane k: byte bw + k, candidate cw + k (0 from n on)
  __device__ __forceinline__ uint32_t byte(uint64_t i) const {
    if (i - bw >= 64) {      // also when bw > i
      bw = i > 0 ? i - 1 : 0;  // the walk asks for p, then for p - 1
      const uint64_t at = bw + lane;
      bv = at < n ? (uint32_t)p[at] : 0;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)bv, (int)(uint32_t)(i - bw));
  }
  __device__ __forceinline__ uint32_t back_byte(uint64_t i) const {
    return __builtin_amdgcn_readfirstlane((uint32_t)p[i]);
  }
  __device__ __forceinline__ uint32_t cand(uint64_t i) const {
    if (i - cw >= 64) {
      cw = i;
      const uint64_t at = cw + lane;
      cv = at < n ? c[at] : 0;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)cv, (int)(uint32_t)(i - cw));
  }
  // 64 bytes a step, a lane each; limit <= 273: five steps at most
  __device__ __forceinline__ uint32_t match_len(uint64_t at, uint32_t d, uint32_t limit) const {
    uint32_t len = limit;
    bool open = true;
    for (uint32_t k0 = 0; open && k0 < limit; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool eq = k < limit && p[at + k] == p[at + k - d];
      const uint64_t differ = ~__ballot(eq);  // a lane at or past limit counts as a difference
      if (differ != 0) {
        len = k0 + (uint32_t)__builtin_ctzll(differ);
        open = false;
      }
    }
    return len;
  }
  // the four rep distances in one step: 16 lanes and 16 bytes each, longer matches by match_len
  __device__ __forceinline__ void rep_lens(uint64_t at, const uint32_t* d, uint32_t limit, uint32_t* l) const {
    const uint32_t r = lane >> 4, k = lane & 15;
    const uint32_t dr = r == 0 ? d[0] : r == 1 ? d[1] : r == 2 ? d[2] : d[3];
    const bool eq = (uint64_t)dr <= at && k < limit && p[at + k] == p[at + k - dr];
    const uint64_t same = __ballot(eq);
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t m = (uint32_t)(same >> (16 * q)) & 0xffffu;
      uint32_t len = (uint32_t)__builtin_ctz(~m | 0x10000u);
      if (len == 16 && limit > 16) len = 16 + match_len(at + 16, d[q], limit - 16);
      l[q] = len;
    }
  }
};

// The probabilities in the wave's LDS region with the encoder's batch on top: lane k
// reads and updates the k-th probability of a symbol's batch, the walk then takes them
// from the lanes in order.  A wave's LDS operations complete in order, so a later batch
// (another lane, the same address) reads what this one wrote.  ZC_XZENC_PLAIN_BITS builds
// the plain form instead (DESIGN 4.14 has both rates).
struct EncProbs : LdsProbs {
#ifdef ZC_XZENC_PLAIN_BITS
  static constexpr bool kBatched = false;
#else
  static constexpr bool kBatched = true;
#endif
  using Vec = uint32_t;
  template <class F>
  __device__ __forceinline__ Vec gather_update(uint32_t count, uint32_t bits, F idx_of) {
    uint32_t v = 0;
    if (lane < count) {
      const uint32_t i = idx_of(lane);
      v = p[i];
      p[i] = (uint16_t)((bits >> lane) & 1 ? v - (v >> 5) : v + ((2048 - v) >> 5));
    }
    return v;
  }
  __device__ __forceinline__ uint32_t vec_get(Vec v, uint32_t k) const {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k);
  }
};

// The stream in global memory.  The walk's bytes are held back in a 64-byte window, a lane
// each, and stored together when a byte falls outside it: a store per byte would stand in
// front of every load of the walk (a wave's loads and stores complete in one order), and the
// walk loads at every symbol.  A stored chunk is copied by all lanes.
struct StreamOut {
  uint8_t* out;
  const uint8_t* pay;
  uint32_t lane;
  uint64_t wb;    // the window holds stream bytes [wb, wb + 64)
  uint64_t held;  // bit k: lane k holds byte wb + k
  uint32_t v;
  __device__ __forceinline__ void flush() {
    if ((held >> lane) & 1) out[wb + lane] = (uint8_t)v;
    held = 0;
  }
  __device__ __forceinline__ void put(uint64_t pos, uint32_t b) {
    if (pos - wb >= 64) {  // also when pos < wb
      flush();
      wb = pos;
    }
    const uint32_t k = (uint32_t)(pos - wb);
    if (lane == k) v = b;
    held |= 1ull << k;
  }
  __device__ __forceinline__ void stored(uint64_t pos, uint64_t src, uint32_t len) {  // len <= 65,536
    // the bytes of the chunk's LZMA form are in memory before other lanes write over them
    flush();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (uint32_t k = lane; k < len; k += 64) out[pos + k] = pay[src + k];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  __device__ __forceinline__ void finish() { flush(); }
};

__global__ __launch_bounds__(kBlock) void zc_xzenc_code_kernel(const EncDesc* __restrict__ desc, uint32_t first,
                                                               uint32_t count, const uint32_t* __restrict__ cand,
                                                               uint32_t check_id,
                                                               zcxzenc::EncResult* __restrict__ res) {
  constexpr uint32_t kWaveBytes = probs_bytes(zcxz::kProbsCommon);
  __shared__ uint4 lds_all[kWaves * kWaveBytes / 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * kWaves;
  uint8_t* mine = reinterpret_cast<uint8_t*>(lds_all) + (size_t)wave * kWaveBytes;
  for (uint32_t j = blockIdx.x * kWaves + wave; j < count; j += waves) {
    const EncDesc x = desc[first + j];
    const uint64_t pay_addr = uniform64(x.pay_addr), n = uniform64(x.pay_size);
    const uint64_t out_addr = uniform64(x.out_addr), out_cap = uniform64(x.out_cap);
    const uint64_t cand_off = uniform64(x.cand_off), check = uniform64(x.check);
    const uint8_t* pay = reinterpret_cast<const uint8_t*>((uintptr_t)pay_addr);
    const WaveSrc in{pay, cand + cand_off, n, lane, 1ull << 62, 1ull << 62, 0, 0};
    EncProbs probs{{reinterpret_cast<uint16_t*>(mine), zcxz::kProbsCommon, lane}};
    StreamOut out{reinterpret_cast<uint8_t*>((uintptr_t)out_addr), pay, lane, 0, 0, 0};
    zcxzenc::NoCount cnt;
    const zcxzenc::EncResult r = zcxzenc::encode(in, n, out_cap, check_id, check, probs, out, cnt);
    if (lane == 0) res[first + j] = r;
    wave_lds_sync();  // the next payload's probabilities reuse the region
  }
}

}  // namespace

struct XzEncScratch {
  Buf<uint8_t> up, down;  // the host forms' payloads and streams
  Buf<EncDesc> desc;
  Buf<zcxzenc::EncResult> res;
  Buf<uint64_t> tables;   // a table per wave of the match kernel's grid
  Buf<uint32_t> cand;     // a distance per payload byte of a batch
  uint32_t gen0 = 0;      // the generation a fresh, regrown or just-cleared table starts from (0; tests: ZC_TEST_XZENC_GEN0)
  uint32_t gen = 0;       // the last generation handed out
  hipEvent_t ev[2] = {};
  int cus = 0;
  XzEncTimes times{};
  uint64_t max_rounds = 0;  // the largest count of rounds a launch of the last call took
  ~XzEncScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

XzEncScratch* xzenc_scratch_new() {
  XzEncScratch* s = new XzEncScratch();
  // (ZC_TEST_XZENC_GEN0: tests start the 32-bit generation near its end, which a context
  // otherwise reaches after some 2^32 launches' rounds; used only inside [0, 0xfffffffe])
  const char* tg = getenv("ZC_TEST_XZENC_GEN0");
  char* end = nullptr;
  const unsigned long long tgv = tg ? strtoull(tg, &end, 10) : 0;
  if (tg && end != tg && *end == 0 && *tg != '-' && tgv <= 0xfffffffeull) s->gen = s->gen0 = (uint32_t)tgv;
  return s;
}
void xzenc_scratch_free(XzEncScratch* s) { delete s; }
const XzEncTimes* xzenc_times(const XzEncScratch* s) { return &s->times; }

void xzenc_schedule(const XzEncScratch* s, uint64_t* batches, uint64_t* max_rounds, uint32_t* generation) {
  *batches = s->times.batches;
  *max_rounds = s->max_rounds;
  *generation = s->gen;
}

uint64_t xzenc_capacity(uint64_t n) { return zcxzenc::capacity(n); }

int xzenc_validate(const void* pay, const uint64_t* pay_off, const uint64_t* pay_size, size_t n, const void* out,
                   const uint64_t* out_off, const uint64_t* out_cap, uint32_t check, const zc_xz_enc_result* res,
                   std::string& err) {
  if (check != zcxz::kCheckNone && check != zcxz::kCheckCrc32 && check != zcxz::kCheckCrc64)
    return arg_error(err, "check id " + std::to_string(check) + " (0, 1 or 4)");
  if (!n) return ZC_OK;
  if (!pay || !pay_off || !pay_size || !out || !out_off || !out_cap || !res) return arg_error(err, "null pointer");
  if (n > 0x7fffffffull) return arg_error(err, "more than 2^31 bundles");
  struct Span {
    uint64_t lo, hi;
    size_t i;
    bool is_out;
  };
  std::vector<Span> spans;
  spans.reserve(2 * n);
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (bundle " + std::to_string(i) + ")";
    if (pay_size[i] > zcxzenc::kMaxPayload) return arg_error(err, "a payload of more than 64 MiB" + at);
    const uint64_t a = (uint64_t)(uintptr_t)pay + pay_off[i], b = (uint64_t)(uintptr_t)out + out_off[i];
    if (a < pay_off[i] || a + pay_size[i] < a) return arg_error(err, "a payload extent wraps the address space" + at);
    if (b < out_off[i] || b + out_cap[i] < b) return arg_error(err, "an output extent wraps the address space" + at);
    if (out_cap[i] >> 40) return arg_error(err, "an extent of 2^40 bytes or more" + at);
    if (pay_size[i]) spans.push_back(Span{a, a + pay_size[i], i, false});
    if (out_cap[i]) spans.push_back(Span{b, b + out_cap[i], i, true});
  }
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
  uint64_t out_hi = 0, pay_hi = 0;  // where the output ranges and the payloads seen so far end
  size_t out_i = 0, pay_i = 0;
  for (const Span& s : spans) {
    if (s.is_out) {
      if (s.lo < out_hi)
        return arg_error(err, "the output ranges of bundles " + std::to_string(out_i) + " and " + std::to_string(s.i) +
                                  " overlap");
      if (s.lo < pay_hi)
        return arg_error(err, "the output range of bundle " + std::to_string(s.i) + " touches the payload of bundle " +
                                  std::to_string(pay_i));
      if (s.hi > out_hi) out_hi = s.hi, out_i = s.i;
    } else {
      if (s.lo < out_hi)
        return arg_error(err, "the output range of bundle " + std::to_string(out_i) + " touches the payload of bundle " +
                                  std::to_string(s.i));
      if (s.hi > pay_hi) pay_hi = s.hi, pay_i = s.i;
    }
  }
  return ZC_OK;
}

int xzenc_encode(XzEncScratch* s, bool host, const void* pay, const uint64_t* pay_off, const uint64_t* pay_size,
                 size_t n, void* out, const uint64_t* out_off, const uint64_t* out_cap, uint32_t check,
                 zc_xz_enc_result* res, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  const auto t_call = Clock::now();
  s->times = XzEncTimes{};
  s->max_rounds = 0;
  if (!n) return ZC_OK;
  if (!s->cus) {
    int dev = 0, cus = 0;
    XCK(hipGetDevice(&dev));
    XCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (hipEvent_t& e : s->ev) XCK(hipEventCreate(&e));
    s->cus = std::max(cus, 1);
  }
  // where the bytes lie
  const uint8_t* d_pay = (const uint8_t*)pay;
  uint8_t* d_out = (uint8_t*)out;
  uint64_t p_lo = 0, o_lo = 0, o_hi = 0;
  if (host) {
    uint64_t hi = 0;
    p_lo = o_lo = ~0ull;
    for (size_t i = 0; i < n; i++) {
      if (pay_size[i]) {
        p_lo = std::min(p_lo, pay_off[i]);
        hi = std::max(hi, pay_off[i] + pay_size[i]);
      }
      if (out_cap[i]) {
        o_lo = std::min(o_lo, out_off[i]);
        o_hi = std::max(o_hi, out_off[i] + out_cap[i]);
      }
    }
    if (p_lo > hi) p_lo = hi = 0;
    if (o_lo > o_hi) o_lo = o_hi = 0;
    p_lo &= ~15ull;
    XCK(s->up.ensure(hi - p_lo));
    XCK(s->down.ensure(o_hi - o_lo));
    if (hi > p_lo) XCK(hipMemcpyAsync(s->up.p, (const uint8_t*)pay + p_lo, hi - p_lo, hipMemcpyHostToDevice, st));
    d_pay = s->up.p;
    d_out = s->down.p;
  } else if (ev_in) {
    XCK(hipEventRecord(ev_in, nullptr));
    XCK(hipStreamWaitEvent(st, ev_in, 0));
  }
  // ---- batches: consecutive payloads whose candidates fit the pool ----
  size_t free_b = 0, total_b = 0;
  XCK(hipMemGetInfo(&free_b, &total_b));
  uint64_t largest = 1;
  for (size_t i = 0; i < n; i++) largest = std::max(largest, pay_size[i]);
  // four bytes of candidates per payload byte: at most a quarter of the free memory and 8 GiB,
  // and at least the largest payload's
  // (ZC_TEST_XZENC_POOL=<bytes> stands for the second term: tests cut a small call into batches)
  uint64_t room = std::min<uint64_t>((uint64_t)free_b / 16, 2ull << 30);
  if (const char* tp = getenv("ZC_TEST_XZENC_POOL")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(tp, &end, 10);
    if (end != tp && *end == 0 && *tp != '-' && v >= 1) room = v;
  }
  const uint64_t pool = std::max<uint64_t>(largest, room);
  std::vector<EncDesc> desc(n);
  std::vector<size_t> batch_end;
  uint64_t in_batch = 0, most = 0;
  for (size_t i = 0; i < n; i++) {
    if (in_batch != 0 && in_batch + pay_size[i] > pool) {
      batch_end.push_back(i);
      in_batch = 0;
    }
    desc[i] = EncDesc{(uint64_t)(uintptr_t)d_pay + pay_off[i] - p_lo, pay_size[i],
                      (uint64_t)(uintptr_t)d_out + out_off[i] - o_lo, out_cap[i], in_batch, 0};
    in_batch += pay_size[i];
    most = std::max(most, in_batch);
  }
  batch_end.push_back(n);
  const auto grid = [&](size_t items) {
    const uint64_t blocks = (items + kWaves - 1) / kWaves;
    return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * kBlocksPerCu)));
  };
  size_t widest = 0;
  for (size_t b = 0, lo = 0; b < batch_end.size(); lo = batch_end[b++]) widest = std::max(widest, batch_end[b] - lo);
  const uint64_t slots = (uint64_t)grid(widest).x * kWaves;
  if (slots * kTableEntries > s->tables.cap || !s->tables.p) {
    XCK(s->tables.ensure(slots * kTableEntries));
    XCK(hipMemsetAsync(s->tables.p, 0, slots * kTableEntries * sizeof(uint64_t), st));  // generation 0: no entry
    s->gen = s->gen0;
  }
  XCK(s->cand.ensure(most));
  XCK(s->desc.ensure(n));
  XCK(s->res.ensure(n));
  XCK(hipMemcpyAsync(s->desc.p, desc.data(), n * sizeof(EncDesc), hipMemcpyHostToDevice, st));
  float ms = 0;
  // ---- the payloads' checks ----
  if (check != zcxz::kCheckNone) {
    XCK(hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(zc_xzenc_check_kernel, grid(n), dim3(kBlock), 0, st, s->desc.p, (uint32_t)n, check);
    XCK(hipGetLastError());
    XCK(hipEventRecord(s->ev[1], st));
    XCK(hipEventSynchronize(s->ev[1]));
    XCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.check_ms = ms;
  }
  // ---- candidates, then the streams, a batch at a time ----
  for (size_t b = 0, lo = 0; b < batch_end.size(); lo = batch_end[b++]) {
    const size_t count = batch_end[b] - lo;
    const dim3 g = grid(count);
    const uint64_t rounds = (count + (uint64_t)g.x * kWaves - 1) / ((uint64_t)g.x * kWaves);
    if ((uint64_t)s->gen + rounds >= 0xffffffffull) {  // the generations are used up: start over on a clear table
      XCK(hipMemsetAsync(s->tables.p, 0, s->tables.cap * sizeof(uint64_t), st));
      s->gen = 0;
    }
    XCK(hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(zc_xzenc_match_kernel, g, dim3(kBlock), 0, st, (const EncDesc*)s->desc.p, (uint32_t)lo,
                       (uint32_t)count, s->tables.p, s->gen + 1, s->cand.p);
    XCK(hipGetLastError());
    s->gen += (uint32_t)rounds;
    s->max_rounds = std::max(s->max_rounds, rounds);
    XCK(hipEventRecord(s->ev[1], st));
    XCK(hipEventSynchronize(s->ev[1]));
    XCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.match_ms += ms;
    XCK(hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(zc_xzenc_code_kernel, g, dim3(kBlock), 0, st, (const EncDesc*)s->desc.p, (uint32_t)lo,
                       (uint32_t)count, (const uint32_t*)s->cand.p, check, s->res.p);
    XCK(hipGetLastError());
    XCK(hipEventRecord(s->ev[1], st));
    XCK(hipEventSynchronize(s->ev[1]));
    XCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.code_ms += ms;
  }
  s->times.batches = batch_end.size();
  std::vector<zcxzenc::EncResult> r(n);
  XCK(hipMemcpyAsync(r.data(), s->res.p, n * sizeof(zcxzenc::EncResult), hipMemcpyDeviceToHost, st));
  XCK(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++) {
    if (r[i].status != zcxz::kOk && r[i].status != zcxz::kOutput) {
      err = "a bundle's status is neither OK nor E_OUTPUT (internal error)";
      return ZC_ERR_STATE;
    }
    if (r[i].status == zcxz::kOk && r[i].size > out_cap[i]) {
      err = "a stream longer than its room (internal error)";
      return ZC_ERR_STATE;
    }
    res[i].status = r[i].status;
    res[i].info = (check & 15) | (r[i].stored << 8);
    res[i].size = r[i].status == zcxz::kOk ? r[i].size : 0;
  }
  if (host) {
    for (size_t i = 0; i < n; i++)
      if (res[i].size)
        XCK(hipMemcpyAsync((uint8_t*)out + out_off[i], s->down.p + (out_off[i] - o_lo), res[i].size,
                           hipMemcpyDeviceToHost, st));
    XCK(hipStreamSynchronize(st));
  }
  s->times.total_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_call).count();
  return ZC_OK;
}

static_assert(sizeof(zcxzenc::EncResult) == 16 && sizeof(zc_xz_enc_result) == 16, "the result records");

}  // namespace zc
