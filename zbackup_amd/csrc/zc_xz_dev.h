// What the xz decoder (zc_xz.hip) and the xz encoder (zc_xzenc.hip) share on
// the device and in their host paths: a wave's LDS ordering, the probabilities
// in a wave's LDS region, the sliced CRC of a wave, a growing device buffer and
// the host paths' error plumbing.  Included inside each file once; everything
// here is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "../../include/zchunk.h"
#include "zc_xz_core.h"

namespace zc {

namespace {

__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
__device__ inline uint64_t uniform64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// the probabilities in the wave's LDS region.  Every lane stores every update
// (the same value to the same address) and reads its own store back, so the
// walk needs no cross-lane ordering here; fill() does, its lanes write for
// each other.  A store by lane 0 alone is ordered as well (a wave's LDS
// operations complete in order) but was measured slower: switching lanes off
// and on around every store cost the 2 MiB text-like bundle 416 ms against
// 347 ms.
struct LdsProbs {
  uint16_t* p;
  uint32_t n, lane;
  __device__ __forceinline__ uint32_t cap() const { return n; }
  __device__ __forceinline__ uint32_t ld(uint32_t i) const { return __builtin_amdgcn_readfirstlane((uint32_t)p[i]); }
  __device__ __forceinline__ void st(uint32_t i, uint32_t v) { p[i] = (uint16_t)v; }
  __device__ __forceinline__ void fill(uint32_t count) {  // count <= n, both even
    wave_lds_sync();
    uint32_t* w = reinterpret_cast<uint32_t*>(p);
    for (uint32_t i = lane; i < count / 2; i += 64) w[i] = 0x04000400u;
    wave_lds_sync();
  }
};

constexpr uint32_t probs_bytes(uint32_t probs) { return (probs * 2 + 15) / 16 * 16; }

template <class T>
__device__ inline T shfl_down_t(T v, uint32_t d) {
  if (sizeof(T) == 8) {
    const uint32_t lo = __shfl_down((uint32_t)v, d, 64);
    const uint32_t hi = __shfl_down((uint32_t)((uint64_t)v >> 32), d, 64);
    return (T)((uint64_t)hi << 32 | lo);
  }
  return (T)__shfl_down((uint32_t)v, d, 64);
}

// The raw CRC (start 0, no final inversion) of p[0, n) by a wave: the bytes,
// zeros in front up to 64 equal slices, a slice per lane; lane 0 returns it.
template <class T>
__device__ inline T wave_raw_crc(const uint8_t* p, uint64_t n, const T* table, T poly, uint32_t lane) {
  // slices of a multiple of 16 bytes: the lanes' starts share their alignment, and the
  // bytes come in aligned 16-byte loads (a lane's 64-byte line serves four loads, not 64)
  const uint64_t slice = ((n + 63) / 64 + 15) & ~15ull, pad = slice * 64 - n;
  const uint64_t lo = (uint64_t)lane * slice, hi = lo + slice;
  const uint64_t b = lo < pad ? 0 : lo - pad, e = hi <= pad ? 0 : hi - pad;  // [b, e) of p; b >= e: none
  T raw = 0;
  uint64_t k = b;
  for (int h = 0; h < 15 && k < e && (((uintptr_t)(p + k)) & 15); ++h, ++k)
    raw = table[(uint32_t)(raw ^ p[k]) & 0xff] ^ (raw >> 8);
  if ((((uintptr_t)(p + k)) & 15) == 0) {
    for (; k + 16 <= e; k += 16) {  // bytes [k, k + 16) lie inside [b, e), 16-byte aligned
      const uint4 v = *reinterpret_cast<const uint4*>(p + k);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        raw = table[(uint32_t)(raw ^ ((w[j >> 2] >> (8 * (j & 3))) & 0xff)) & 0xff] ^ (raw >> 8);
    }
  }
  for (; k < e; ++k) raw = table[(uint32_t)(raw ^ p[k]) & 0xff] ^ (raw >> 8);
  T X = zcxz::gf_x8n<T>(slice, poly);  // a slice further: x^(8 slice)
  for (uint32_t s = 1; s < 64; s <<= 1) {
    const T right = shfl_down_t(raw, s);
    raw = zcxz::gf_mul(raw, X, poly) ^ right;
    X = zcxz::gf_mul(X, X, poly);
  }
  return raw;
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
#define XCK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

using Clock = std::chrono::steady_clock;

}  // namespace

}  // namespace zc
