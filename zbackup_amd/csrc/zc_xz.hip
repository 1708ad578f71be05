// zc_xz.hip -- LZMA bundles decoded on the GPU.  Bundle::Reader (bundle.cc:179-216)
// runs a bundle's body through lzma_stream_decoder (compression.cc:99-107); here
// the bodies of a whole restore or adoption go through in one call and the
// payloads land in HBM, where Restorer, IndexedRestorer and Adopter read them.
// zc_xz_core.h is the format and the walk; this file is its schedule.
//
//   decode   zc_xz_decode_kernel<probabilities>   a wave per bundle.  The
//            walk's state is wave-uniform: every lane runs the same walk, and
//            what it reads (input bytes and probabilities from the wave's LDS
//            region, bytes of the output written so far) comes through
//            readfirstlane, so its branches are scalar.  The compressed bytes
//            pass through an LDS window the 64 lanes refill together; the
//            output in global memory is the dictionary: a literal is stored
//            by one lane, a match is copied by the lanes in steps of 64 from
//            the periodic source out[p - dist + k % dist], all of it below p.
//            Two compiled forms by LDS room: the common one for lc + lp <= 3
//            (every liblzma preset) and the wide one for lc + lp = 4, which
//            the host launches for exactly the bundles the common form marked.
//   check    zc_xz_check_kernel   a wave per decoded block: 64 slices, a table
//            CRC each, combined with one x^(8 slice) operator, compared with
//            the stored CRC32 / CRC64.
//
// Every loop of the decode kernel is the core's: one trip count fixed before
// the walk, constant counts, or sizes the walk validated.  No wave waits on
// another, there is no workgroup barrier in the decode kernel and no spin; the
// waves of a workgroup share nothing but the launch.
#include <hip/hip_runtime.h>

#include <stdio.h>
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

namespace zc {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kWindow = 2048;  // the input window of a wave, bytes

struct XzDesc {
  uint64_t in_addr, in_size;  // absolute device address of the stream
  uint64_t out_addr, out_cap;
};

// A wave's window over the bytes [0, n) at g (zc_index.hip's Tile, restated):
// window byte t is byte lo + t.  lo keeps the window's start 16-byte aligned
// in memory, so it may lie before g; such bytes, and those from n on, are
// never loaded.  All 64 lanes, uniformly: stage the window that holds byte
// `at` (at < n); returns lo.  One copy of this code, called: the walk reads
// bytes in some sixty places.
__device__ __noinline__ int64_t stage_window(const uint8_t* g, uint64_t n, uint8_t* lds, uint32_t bytes, uint64_t at,
                                             uint32_t lane) {
  wave_lds_sync();  // the reads of the old window are done
  const uintptr_t base = (uintptr_t)g;
  const int64_t lo = (int64_t)at - (int64_t)((base + at) & 15);
  const uint64_t top = (uint64_t)(lo + (int64_t)bytes);
  const uint64_t hi = top < n ? top : n;
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
  return lo;
}
struct Tile {
  const uint8_t* g;
  uint64_t n;
  uint8_t* lds;
  uint32_t bytes;
  int64_t lo;
  uint64_t hi;  // bytes [max(lo, 0), hi) are staged
  __device__ __forceinline__ void stage(uint64_t at, uint32_t lane) {
    lo = (int64_t)uniform64((uint64_t)stage_window(g, n, lds, bytes, at, lane));
    const uint64_t top = (uint64_t)(lo + (int64_t)bytes);
    hi = top < n ? top : n;
  }
  __device__ __forceinline__ bool holds(uint64_t a, uint64_t b) const { return (int64_t)a >= lo && b <= hi; }
};

// the walk's source: every lane asks for the same byte; a byte outside the
// window brings the window that holds it
struct UniformSrc {
  Tile* t;
  uint32_t lane;
  __device__ __forceinline__ uint32_t byte(uint64_t i) const {
    if (!t->holds(i, i + 1)) t->stage(i, lane);
    return __builtin_amdgcn_readfirstlane((uint32_t)t->lds[(int64_t)i - t->lo]);
  }
};

// The sink: the output in global memory is the dictionary.  The walk hands it
// only validated ops (zc_xz_core.h), and every source byte of a read lies
// below the write position.  A wavefront-scope fence stands between the stores
// of earlier symbols (other lanes') and each load.
struct GlobalOut {
  uint8_t* out;
  const uint8_t* in;
  uint32_t lane;
  __device__ __forceinline__ void lit(uint64_t pos, uint32_t b) {
    if (lane == 0) out[pos] = (uint8_t)b;
  }
  __device__ __forceinline__ uint32_t get(uint64_t pos) const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    return __builtin_amdgcn_readfirstlane((uint32_t)out[pos]);
  }
  __device__ __forceinline__ void copy(uint64_t pos, uint32_t dist, uint32_t len) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const uint8_t* src = out + (pos - dist);
    uint8_t* dst = out + pos;
    if (dist >= 64) {
      // a step's 64 bytes lie inside one period or across one wrap: k0 mod dist is
      // carried along, no division
      uint32_t r0 = 0;  // k0 mod dist
      for (uint32_t k0 = 0; k0 < len; k0 += 64) {  // len <= 273: five steps at most
        const uint32_t k = k0 + lane, r = r0 + lane;
        if (k < len) dst[k] = src[r >= dist ? r - dist : r];
        r0 += 64;
        if (r0 >= dist) r0 -= dist;
      }
    } else {
      for (uint32_t k0 = 0; k0 < len; k0 += 64) {
        const uint32_t k = k0 + lane;
        if (k < len) dst[k] = src[k % dist];
      }
    }
  }
  __device__ __forceinline__ void stored(uint64_t src, uint64_t pos, uint32_t len) {  // len <= 65,536
    for (uint32_t k = lane; k < len; k += 64) out[pos + k] = in[src + k];
  }
};

// bundle list[j] (list null: bundle j) for j < n, a wave each
template <uint32_t PROBS>
__global__ __launch_bounds__(kBlock) void zc_xz_decode_kernel(const XzDesc* __restrict__ desc,
                                                              const uint32_t* __restrict__ list, uint32_t n,
                                                              zcxz::Result* __restrict__ res) {
  constexpr uint32_t kWaveBytes = probs_bytes(PROBS) + kWindow;
  __shared__ uint4 lds_all[kWaves * kWaveBytes / 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * kWaves;
  uint8_t* mine = reinterpret_cast<uint8_t*>(lds_all) + (size_t)wave * kWaveBytes;
  for (uint32_t j = blockIdx.x * kWaves + wave; j < n; j += waves) {
    const uint32_t i = list ? __builtin_amdgcn_readfirstlane(list[j]) : j;
    const XzDesc x = desc[i];
    const uint64_t in_addr = uniform64(x.in_addr), in_size = uniform64(x.in_size);
    const uint64_t out_addr = uniform64(x.out_addr), out_cap = uniform64(x.out_cap);
    const uint8_t* in_p = reinterpret_cast<const uint8_t*>((uintptr_t)in_addr);
    Tile tile{in_p, in_size, mine + probs_bytes(PROBS), kWindow, 0, 0};
    const UniformSrc in{&tile, lane};
    LdsProbs probs{reinterpret_cast<uint16_t*>(mine), PROBS, lane};
    GlobalOut out{reinterpret_cast<uint8_t*>((uintptr_t)out_addr), in_p, lane};
    const zcxz::Result r = zcxz::decode(in, in_size, out_cap, probs, out);
    if (lane == 0) res[i] = r;
    wave_lds_sync();  // the next bundle's window and probabilities reuse the region
  }
}

// ---- the payload's check ----

// bundle list[j] for j < n: status kOk, check id 1 or 4, decoded > 0 (the host's choice)
__global__ __launch_bounds__(kBlock) void zc_xz_check_kernel(const XzDesc* __restrict__ desc,
                                                             const uint32_t* __restrict__ list, uint32_t n,
                                                             zcxz::Result* __restrict__ res) {
  __shared__ uint64_t t64[256];
  __shared__ uint32_t t32[256];
  t64[threadIdx.x] = zcxz::crc64_entry(threadIdx.x);
  t32[threadIdx.x] = zcxz::crc32_entry(threadIdx.x);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t waves = gridDim.x * kWaves;
  for (uint32_t j = blockIdx.x * kWaves + wave; j < n; j += waves) {
    const uint32_t i = list[j];
    const zcxz::Result r = res[i];
    const uint8_t* p = reinterpret_cast<const uint8_t*>((uintptr_t)desc[i].out_addr);
    uint64_t got;
    if (r.check_id == zcxz::kCheckCrc64)
      got = zcxz::crc64_finish_raw(wave_raw_crc<uint64_t>(p, r.decoded, t64, zcxz::kPoly64, lane), r.decoded);
    else
      got = zcxz::crc32_finish_raw(wave_raw_crc<uint32_t>(p, r.decoded, t32, zcxz::kPoly32, lane), r.decoded);
    if (lane == 0 && got != r.stored) res[i].status = zcxz::kCheck;
  }
}

}  // namespace

struct XzScratch {
  Buf<uint8_t> up, down;  // the host forms' streams and payloads
  Buf<XzDesc> desc;
  Buf<uint32_t> list;
  Buf<zcxz::Result> res;
  hipEvent_t ev[6] = {};
  int cus = 0;
  XzTimes times{};
  ~XzScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

XzScratch* xz_scratch_new() { return new XzScratch(); }
void xz_scratch_free(XzScratch* s) { delete s; }
const XzTimes* xz_times(const XzScratch* s) { return &s->times; }

int xz_validate(const void* in, const uint64_t* in_off, const uint64_t* in_size, size_t n, const void* out,
                const uint64_t* out_off, const uint64_t* out_cap, const zc_xz_result* res, std::string& err) {
  if (!n) return ZC_OK;
  if (!in || !in_off || !in_size || !out || !out_off || !out_cap || !res) return arg_error(err, "null pointer");
  if (n > 0x7fffffffull) return arg_error(err, "more than 2^31 bundles");
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (bundle " + std::to_string(i) + ")";
    const uint64_t a = (uint64_t)(uintptr_t)in + in_off[i], b = (uint64_t)(uintptr_t)out + out_off[i];
    if (a < in_off[i] || a + in_size[i] < a) return arg_error(err, "an input extent wraps the address space" + at);
    if (b < out_off[i] || b + out_cap[i] < b) return arg_error(err, "an output extent wraps the address space" + at);
    if (in_size[i] >> 40 || out_cap[i] >> 40) return arg_error(err, "an extent of 2^40 bytes or more" + at);
  }
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return out_off[a] < out_off[b]; });
  size_t last = n;  // the last range with room
  for (size_t k = 0; k < n; k++) {
    const size_t i = order[k];
    if (!out_cap[i]) continue;
    if (last != n && out_off[last] + out_cap[last] > out_off[i])
      return arg_error(err, "the output ranges of bundles " + std::to_string(last) + " and " + std::to_string(i) +
                                " overlap");
    last = i;
  }
  return ZC_OK;
}

int xz_decode(XzScratch* s, bool host, const void* in, const uint64_t* in_off, const uint64_t* in_size, size_t n,
              void* out, const uint64_t* out_off, const uint64_t* out_cap, zc_xz_result* res, hipEvent_t ev_in,
              hipStream_t st, std::string& err) {
  const auto t_call = Clock::now();
  s->times = XzTimes{};
  if (!n) return ZC_OK;
  if (!s->cus) {
    int dev = 0, cus = 0;
    XCK(hipGetDevice(&dev));
    XCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (hipEvent_t& e : s->ev) XCK(hipEventCreate(&e));
    s->cus = std::max(cus, 1);
  }
  // where the bytes lie
  const uint8_t* d_in = (const uint8_t*)in;
  uint8_t* d_out = (uint8_t*)out;
  uint64_t i_lo = 0, o_lo = 0, o_hi = 0;
  if (host) {
    uint64_t hi = 0;
    i_lo = o_lo = ~0ull;
    for (size_t i = 0; i < n; i++) {
      if (in_size[i]) {
        i_lo = std::min(i_lo, in_off[i]);
        hi = std::max(hi, in_off[i] + in_size[i]);
      }
      if (out_cap[i]) {
        o_lo = std::min(o_lo, out_off[i]);
        o_hi = std::max(o_hi, out_off[i] + out_cap[i]);
      }
    }
    if (i_lo > hi) i_lo = hi = 0;
    if (o_lo > o_hi) o_lo = o_hi = 0;
    i_lo &= ~15ull;
    XCK(s->up.ensure(hi - i_lo));
    XCK(s->down.ensure(o_hi - o_lo));
    if (hi > i_lo) XCK(hipMemcpyAsync(s->up.p, (const uint8_t*)in + i_lo, hi - i_lo, hipMemcpyHostToDevice, st));
    d_in = s->up.p;
    d_out = s->down.p;
  } else if (ev_in) {
    XCK(hipEventRecord(ev_in, nullptr));
    XCK(hipStreamWaitEvent(st, ev_in, 0));
  }
  std::vector<XzDesc> desc(n);
  for (size_t i = 0; i < n; i++)
    desc[i] = XzDesc{(uint64_t)(uintptr_t)d_in + in_off[i] - i_lo, in_size[i],
                     (uint64_t)(uintptr_t)d_out + out_off[i] - o_lo, out_cap[i]};
  XCK(s->desc.ensure(n));
  XCK(s->res.ensure(n));
  XCK(s->list.ensure(n));
  XCK(hipMemcpyAsync(s->desc.p, desc.data(), n * sizeof(XzDesc), hipMemcpyHostToDevice, st));
  const auto grid = [&](size_t items, int blocks_per_cu) {
    const uint64_t blocks = (items + kWaves - 1) / kWaves;
    return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)s->cus * blocks_per_cu)));
  };
  // ---- decode: the common form over all, the wide form over those that asked ----
  XCK(hipEventRecord(s->ev[0], st));
  hipLaunchKernelGGL((zc_xz_decode_kernel<zcxz::kProbsCommon>), grid(n, 8), dim3(kBlock), 0, st, s->desc.p,
                     (const uint32_t*)nullptr, (uint32_t)n, s->res.p);
  XCK(hipGetLastError());
  XCK(hipEventRecord(s->ev[1], st));
  std::vector<zcxz::Result> r(n);
  XCK(hipMemcpyAsync(r.data(), s->res.p, n * sizeof(zcxz::Result), hipMemcpyDeviceToHost, st));
  XCK(hipStreamSynchronize(st));
  std::vector<uint32_t> wide;
  for (size_t i = 0; i < n; i++)
    if (r[i].status == zcxz::kNeedWide) wide.push_back((uint32_t)i);
  XCK(hipEventRecord(s->ev[2], st));
  if (!wide.empty()) {
    XCK(hipMemcpyAsync(s->list.p, wide.data(), wide.size() * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((zc_xz_decode_kernel<zcxz::kProbsWide>), grid(wide.size(), 4), dim3(kBlock), 0, st, s->desc.p,
                       (const uint32_t*)s->list.p, (uint32_t)wide.size(), s->res.p);
    XCK(hipGetLastError());
    XCK(hipMemcpyAsync(r.data(), s->res.p, n * sizeof(zcxz::Result), hipMemcpyDeviceToHost, st));
    XCK(hipStreamSynchronize(st));
    for (uint32_t i : wide)
      if (r[i].status == zcxz::kNeedWide) {
        err = "the wide form asked for more probabilities (internal error)";
        return ZC_ERR_STATE;
      }
  }
  // ---- the payloads' checks ----
  XCK(hipEventRecord(s->ev[3], st));
  std::vector<uint32_t> chk;
  for (size_t i = 0; i < n; i++)
    if (r[i].status == zcxz::kOk && r[i].decoded && r[i].check_id != zcxz::kCheckNone) chk.push_back((uint32_t)i);
  if (!chk.empty()) {
    XCK(hipMemcpyAsync(s->list.p, chk.data(), chk.size() * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(zc_xz_check_kernel, grid(chk.size(), 8), dim3(kBlock), 0, st, s->desc.p,
                       (const uint32_t*)s->list.p, (uint32_t)chk.size(), s->res.p);
    XCK(hipGetLastError());
  }
  XCK(hipEventRecord(s->ev[4], st));
  if (!chk.empty()) XCK(hipMemcpyAsync(r.data(), s->res.p, n * sizeof(zcxz::Result), hipMemcpyDeviceToHost, st));
  XCK(hipStreamSynchronize(st));
  std::vector<bool> is_wide(n, false);
  for (uint32_t i : wide) is_wide[i] = true;
  for (size_t i = 0; i < n; i++) {
    if (r[i].decoded > out_cap[i]) {
      err = "a bundle decoded past its room (internal error)";
      return ZC_ERR_STATE;
    }
    res[i].status = r[i].status;
    res[i].info = (r[i].check_id & 15) | (is_wide[i] ? 0x100u : 0);
    res[i].decoded = r[i].decoded;
    res[i].consumed = r[i].status == zcxz::kOk ? r[i].consumed : 0;
  }
  if (host) {
    // the decoded bytes back, and nothing else: neighbours that are full go in one copy
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return out_off[a] < out_off[b]; });
    uint64_t run_off = 0, run_len = 0;
    for (size_t k = 0; k < n; k++) {
      const size_t i = order[k];
      if (!r[i].decoded) continue;
      if (run_len && out_off[i] == run_off + run_len) {
        run_len += r[i].decoded;
        continue;
      }
      if (run_len)
        XCK(hipMemcpyAsync((uint8_t*)out + run_off, s->down.p + (run_off - o_lo), run_len, hipMemcpyDeviceToHost, st));
      run_off = out_off[i];
      run_len = r[i].decoded;
    }
    if (run_len)
      XCK(hipMemcpyAsync((uint8_t*)out + run_off, s->down.p + (run_off - o_lo), run_len, hipMemcpyDeviceToHost, st));
    XCK(hipStreamSynchronize(st));
  }
  float ms = 0, ms2 = 0;
  XCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  XCK(hipEventElapsedTime(&ms2, s->ev[2], s->ev[3]));
  s->times.decode_ms = ms + (wide.empty() ? 0 : ms2);
  XCK(hipEventElapsedTime(&ms, s->ev[3], s->ev[4]));
  s->times.check_ms = ms;
  s->times.n_wide = wide.size();
  s->times.total_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_call).count();
  return ZC_OK;
}

static_assert(ZC_XZ_OK == zcxz::kOk && ZC_XZ_E_FORMAT == zcxz::kFormat && ZC_XZ_E_UNSUPPORTED == zcxz::kUnsupported &&
                  ZC_XZ_E_HEADER == zcxz::kHeader && ZC_XZ_E_DATA == zcxz::kData && ZC_XZ_E_INPUT == zcxz::kInput &&
                  ZC_XZ_E_OUTPUT == zcxz::kOutput && ZC_XZ_E_CHECK == zcxz::kCheck && ZC_XZ_E_BUDGET == zcxz::kBudget,
              "xz status codes");

}  // namespace zc
