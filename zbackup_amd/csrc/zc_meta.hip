// zc_meta.hip -- chunk metadata from bytes wherever they lie: adopting a
// repository the engine did not write.
//
// A repository written by stock zbackup is known by chunk id only; the record
// that lets an id take the anchor path (zc_chunk_meta) is a pure
// function of the chunk's bytes, so it can be computed from decoded bundle
// payloads: chunks back to back at arbitrary byte offsets, sizes 1..W, no scan
// laid over them.  zc_meta_core.h is the scalar definition.  Three launches:
//
//   zc_extent_meta_kernel  one wave per chunk: the rolling hash and the first
//                          content anchor from the bytes alone
//   zc_sha1_kernel         the existing lane-per-chunk SHA-1 (zc_kernels.hip)
//                          over the same extents
//   zc_meta_pack_kernel    the 48-byte records assembled in HBM and compared
//                          with the ids the bundles claim
//
// zc_extent_meta_kernel.  The wave reads the 16-byte-aligned pieces that cover
// the chunk, lane l pieces l, l + 64, ...: consecutive lanes read consecutive
// 16 bytes.  A piece that is not wholly inside the payload is read dword by
// dword, and only the dwords that hold a payload byte.  Bytes of a piece
// outside the chunk (before its first byte in the first piece, after its last
// in the last) are left out of the digest one by one.
//   Rolling hash: every lane keeps a Horner accumulator over its own pieces
// (x 257^1024 per wave step, 1008 of that before the piece and 16 inside it),
// which is then weighted by 257^(chunk bytes after the lane's last piece) and
// summed across the wave; 257^size joins at the end.
//   First anchor (size == W > 63 only): the anchor state is linear in the bytes
// and forgets everything older than 32 bytes, so the state before a piece is
// (G(piece - 2) << 8) + G(piece - 1) per 16-bit half, G(p) being the state p's
// own 16 bytes leave from zero.  Every lane computes its G, takes the two
// below it from lanes l - 1 and l - 2 (lanes 0 and 1: from lanes 62 and 63 of
// the step before), and tests its 16 positions.  Once a step has found an
// anchor the later steps skip this work (later pieces hold later positions);
// the loop itself runs on.
//
// Every loop's trip count is fixed from the chunk's offset and size before the
// loop; no kernel waits on another wave, spins, or ends on a data value.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_meta_core.h"

namespace zc {

namespace {

constexpr int kBlock = 256;            // 4 waves: 4 chunks per workgroup
constexpr int kWavesPerBlock = kBlock / 64;

static_assert(sizeof(zc_chunk_meta) == sizeof(zcmeta::Record) && sizeof(zc_seed) == sizeof(zcmeta::Expect),
              "zc_meta_core.h restates zchunk.h's records");
static_assert(ZC_META_BAD_SHA1 == zcmeta::kBadSha1 && ZC_META_BAD_ROLLING == zcmeta::kBadRolling &&
                  ZC_META_BAD_SIZE == zcmeta::kBadSize && ZC_META_NO_ANCHOR == zcmeta::kNoAnchor &&
                  ZC_ANCHOR_MIN_OFF == zcmeta::kAnchorMinOff,
              "zc_meta_core.h restates the constants");

// what zc_extent_meta_kernel leaves per chunk
struct ExtentMeta {
  uint64_t rolling;
  uint64_t fingerprint;
  uint32_t anchor;
  uint32_t gear;
};

// the dwords that hold a payload byte, as offsets from `data`: the payload's
// first byte rounded down, its end rounded up to a dword
struct PayloadSpan {
  uint64_t dw_lo, dw_hi;
};

// The 16-byte piece at offset a (a multiple of 16): one 16-byte load when all
// four dwords hold payload bytes, else the dwords that do (the others read 0)
__device__ __forceinline__ uint4 load_piece(const uint8_t* __restrict__ data, uint64_t a, const PayloadSpan& ps) {
  if (a >= ps.dw_lo && a + 16 <= ps.dw_hi) return *reinterpret_cast<const uint4*>(data + a);
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t d = a + 4 * k;
    w[k] = (d >= ps.dw_lo && d + 4 <= ps.dw_hi) ? *reinterpret_cast<const uint32_t*>(data + d) : 0u;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t piece_byte(const uint4& x, int k) {
  const uint32_t w = k < 4 ? x.x : k < 8 ? x.y : k < 12 ? x.z : x.w;
  return (w >> (8 * (k & 3))) & 0xFFu;
}

// four bytes of a dword in stream order as one Horner term: b0 257^3 + b1 257^2 + b2 257 + b3
__device__ __forceinline__ uint64_t horner4(uint32_t w) {
  return (uint64_t)(w & 0xFFu) * 16974593u + (((w >> 8) & 0xFFu) * 66049u + ((w >> 16) & 0xFFu) * 257u + (w >> 24));
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void zc_extent_meta_kernel(const uint8_t* __restrict__ data, PayloadSpan ps,
                                                                const uint64_t* __restrict__ off,
                                                                const uint32_t* __restrict__ size, uint32_t n,
                                                                uint32_t W, int32_t anchor_lo,
                                                                ExtentMeta* __restrict__ out) {
  const uint32_t chunk = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (chunk >= n) return;  // the whole wave
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t s = off[chunk];
  const uint32_t sz = size[chunk];
  const uint64_t e = s + sz;
  const uint64_t A = s & ~15ull;
  const uint64_t P = (e - A + 15) >> 4;     // pieces that cover the chunk
  const uint64_t T = (P + 63) >> 6;         // wave steps
  const bool anchors = sz == W && W > ZC_ANCHOR_MIN_OFF;

  const uint64_t m1008 = zcmeta::pow257(1008), m1024 = zcmeta::pow257(1024), m4 = 257ull * 257 * 257 * 257;
  uint64_t acc = 0;
  uint32_t best_q = ZC_NO_ANCHOR, best_g = 0;
  uint32_t carry62 = 0, carry63 = 0;  // G of the last two pieces of the step before
  bool found = false;                 // wave-uniform: a step has found an anchor

  for (uint64_t t = 0; t < T; ++t) {
    const uint64_t j = (t << 6) + lane;
    const bool have = j < P;
    const uint64_t a = A + (j << 4);
    uint4 x = make_uint4(0, 0, 0, 0);
    if (have) x = load_piece(data, a, ps);
    // bytes [lo, hi) of the piece are the chunk's
    const uint32_t lo = s > a ? (uint32_t)(s - a) : 0u;
    const uint32_t hi = e < a + 16 ? (uint32_t)(e - a) : 16u;
    if (have) {
      if (lo == 0 && hi == 16) {
        uint64_t h = horner4(x.x);
        h = h * m4 + horner4(x.y);
        h = h * m4 + horner4(x.z);
        h = h * m4 + horner4(x.w);
        acc = acc * m1024 + h;
      } else {
        acc *= m1008;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((uint32_t)k < hi) acc = acc * 257u + ((uint32_t)k >= lo ? piece_byte(x, k) : 0u);
      }
    }
    if (anchors && !found) {
      uint32_t G = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) G = zcmeta::gear_step(G, piece_byte(x, k));
      uint32_t g1 = __shfl_up(G, 1, 64), g2 = __shfl_up(G, 2, 64);
      if (lane == 0) {
        g1 = carry63;
        g2 = carry62;
      } else if (lane == 1) {
        g2 = carry63;
      }
      carry62 = __shfl(G, 62, 64);
      carry63 = __shfl(G, 63, 64);
      // both halves of g2 sixteen bytes on (eight steps each), plus g1, per half
      const uint32_t adv = (g2 << 8) & 0xFF00FF00u;
      uint32_t g = ((adv & 0xFFFF0000u) + (g1 & 0xFFFF0000u)) | ((adv + g1) & 0xFFFFu);
      const uint64_t q0 = a - s;  // position of the piece's first byte (only read where a + k >= s + 63)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        g = zcmeta::gear_step(g, piece_byte(x, k));
        const bool in = have && a + k >= s + ZC_ANCHOR_MIN_OFF && a + k < e;
        if (in && best_q == ZC_NO_ANCHOR && zcmeta::anchor_hit(g, anchor_lo)) {
          best_q = (uint32_t)(q0 + k);
          best_g = g;
        }
      }
      found = __any(best_q != ZC_NO_ANCHOR);
    }
  }

  // the lanes' accumulators, each moved up by the chunk bytes after its last piece
  uint64_t part = 0;
  if (lane < P) {
    const uint64_t jl = lane + (((P - 1 - lane) >> 6) << 6);
    const uint64_t end = std::min<uint64_t>(e, A + (jl << 4) + 16);
    part = acc * zcmeta::pow257((uint32_t)(e - end));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) part += shfl_xor64(part, m);
  // the first anchor: the smallest position any lane holds
  uint32_t q = best_q;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) q = min(q, (uint32_t)__shfl_xor(q, m, 64));
  const unsigned long long owner = __ballot(best_q == q);
  const uint32_t gq = __shfl(best_g, (int)__ffsll((long long)owner) - 1, 64);
  if (lane == 0) {
    ExtentMeta r;
    r.rolling = zcmeta::pow257(sz) + part;
    r.anchor = q;
    r.gear = 0;
    r.fingerprint = 0;
    if (q != ZC_NO_ANCHOR) {
      r.gear = gq;
      uint64_t f = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) f |= (uint64_t)data[s + q - 7 + k] << (8 * k);
      r.fingerprint = f;
    }
    out[chunk] = r;
  }
}

// The records in HBM, one thread per chunk; with expected ids, what differs
__global__ __launch_bounds__(kBlock) void zc_meta_pack_kernel(const ExtentMeta* __restrict__ em,
                                                              const uint8_t* __restrict__ sha20,
                                                              const uint32_t* __restrict__ size, uint32_t n,
                                                              uint32_t def, const zcmeta::Expect* __restrict__ expect,
                                                              zcmeta::Record* __restrict__ rec,
                                                              uint8_t* __restrict__ status,
                                                              unsigned long long* __restrict__ n_bad) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const ExtentMeta m = em[i];
  const zcmeta::Record r =
      zcmeta::make_record(sha20 + (uint64_t)i * 20, m.rolling, size[i], def, m.anchor, m.gear, m.fingerprint);
  rec[i] = r;
  uint32_t st = 0;
  if (expect) st = zcmeta::compare(r, expect[i]);
  status[i] = (uint8_t)st;
  if (st) atomicAdd(n_bad, 1ull);
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
#define MCK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

using Clock = std::chrono::steady_clock;

}  // namespace

struct MetaScratch {
  Buf<uint8_t> payload, sha, status;
  Buf<uint64_t> off;
  Buf<uint32_t> size;
  Buf<zcmeta::Expect> expect;
  Buf<ExtentMeta> em;
  Buf<zcmeta::Record> rec;
  Buf<unsigned long long> n_bad;
  hipEvent_t ev[3] = {};
  MetaTimes times{};
  ~MetaScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

MetaScratch* meta_scratch_new() { return new MetaScratch(); }
void meta_scratch_free(MetaScratch* s) { delete s; }
const MetaTimes* meta_times(const MetaScratch* s) { return &s->times; }

int meta_validate(const void* payload, uint64_t payload_bytes, const uint64_t* off, const uint32_t* size, size_t n,
                  const zc_seed* expect, const zc_chunk_meta* out, const uint8_t* status, const size_t* n_bad,
                  std::string& err) {
  if (!n) return ZC_OK;
  if (!payload || !off || !size || !out) return arg_error(err, "null payload, off, size or out with n > 0");
  if (expect && !status && !n_bad) return arg_error(err, "expected ids given, but neither status nor n_bad");
  if (n >= 0xFFFFFFFFull) return arg_error(err, "the chunk count must stay below 2^32 - 1");
  for (size_t i = 0; i < n; ++i) {
    if (size[i] == 0) return arg_error(err, "size[" + std::to_string(i) + "] is 0");
    if (off[i] > payload_bytes || size[i] > payload_bytes - off[i])
      return arg_error(err, "chunk " + std::to_string(i) + " [" + std::to_string(off[i]) + ", +" +
                                std::to_string(size[i]) + ") ends past the payload's " +
                                std::to_string(payload_bytes) + " bytes");
  }
  return ZC_OK;
}

int meta_compute(MetaScratch* s, bool host, const void* payload, uint64_t payload_bytes, const uint64_t* off,
                 const uint32_t* size, size_t n, uint32_t W, uint32_t def, const zc_seed* expect, zc_chunk_meta* out,
                 uint8_t* status, size_t* n_bad, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  s->times = MetaTimes{};
  const auto t0 = Clock::now();
  if (zcmeta::anchor_lo_for(W) != anchor_lo_for(W) || zcmeta::anchor_rate_inv(W) != anchor_rate_inv(W)) {
    err = "zc_meta_core.h and zc_device.h disagree on the anchor rate (internal error)";
    return ZC_ERR_STATE;
  }
  if (!s->ev[0])
    for (hipEvent_t& e : s->ev) MCK(hipEventCreate(&e));
  MCK(s->off.ensure(n));
  MCK(s->size.ensure(n));
  MCK(s->sha.ensure(20 * n));
  MCK(s->em.ensure(n));
  MCK(s->rec.ensure(n));
  MCK(s->status.ensure(n));
  MCK(s->n_bad.ensure(1));
  if (expect) MCK(s->expect.ensure(n));
  const uint8_t* d_pay = (const uint8_t*)payload;
  if (host) {
    MCK(s->payload.ensure(payload_bytes));
    MCK(hipMemcpyAsync(s->payload.p, payload, payload_bytes, hipMemcpyHostToDevice, st));
    d_pay = s->payload.p;
  } else if (ev_in) {
    MCK(hipEventRecord(ev_in, nullptr));  // after the caller's default-stream work
    MCK(hipStreamWaitEvent(st, ev_in, 0));
  }
  // the kernels address the payload from the 16-byte boundary at or below it
  const uint64_t shift = (uint64_t)(uintptr_t)d_pay & 15u;
  const uint8_t* data = d_pay - shift;
  std::vector<uint64_t> h_off(off, off + n);
  if (shift)
    for (uint64_t& o : h_off) o += shift;
  PayloadSpan ps;
  ps.dw_lo = shift & ~3ull;
  ps.dw_hi = (shift + payload_bytes + 3) & ~3ull;
  MCK(hipMemcpyAsync(s->off.p, h_off.data(), 8 * n, hipMemcpyHostToDevice, st));
  MCK(hipMemcpyAsync(s->size.p, size, 4 * n, hipMemcpyHostToDevice, st));
  if (expect) MCK(hipMemcpyAsync(s->expect.p, expect, sizeof(zc_seed) * n, hipMemcpyHostToDevice, st));
  MCK(hipMemsetAsync(s->n_bad.p, 0, sizeof(unsigned long long), st));
  MCK(hipEventRecord(s->ev[0], st));
  const uint32_t nn = (uint32_t)n;
  zc_extent_meta_kernel<<<(nn + kWavesPerBlock - 1) / kWavesPerBlock, kBlock, 0, st>>>(
      data, ps, s->off.p, s->size.p, nn, W, zcmeta::anchor_lo_for(W), s->em.p);
  MCK(hipGetLastError());
  MCK(hipEventRecord(s->ev[1], st));
  MCK(launch_sha1(data, s->off.p, s->size.p, nn, s->sha.p, st));
  MCK(hipEventRecord(s->ev[2], st));
  zc_meta_pack_kernel<<<(nn + kBlock - 1) / kBlock, kBlock, 0, st>>>(
      s->em.p, s->sha.p, s->size.p, nn, def, expect ? s->expect.p : nullptr, s->rec.p, s->status.p, s->n_bad.p);
  MCK(hipGetLastError());
  unsigned long long bad = 0;
  MCK(hipMemcpyAsync(out, s->rec.p, sizeof(zc_chunk_meta) * n, hipMemcpyDeviceToHost, st));
  if (status) MCK(hipMemcpyAsync(status, s->status.p, n, hipMemcpyDeviceToHost, st));
  MCK(hipMemcpyAsync(&bad, s->n_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
  MCK(hipStreamSynchronize(st));
  if (n_bad) *n_bad = (size_t)bad;
  float ms = 0;
  MCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->times.meta_ms = ms;
  MCK(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
  s->times.sha1_ms = ms;
  s->times.total_ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  return ZC_OK;
}

}  // namespace zc
