// One wave's byte copy, shared by zc_lzo_copy_kernel (zc_lzo.hip) and
// zc_range_read_kernel (zc_range.hip): a head of bytes up to the destination's
// 16-byte alignment, 16-byte aligned stores (the source read unaligned), a byte
// tail.  Exactly the bytes [dst, dst + len) are written and exactly the bytes
// [src, src + len) are read; the lanes of the wave share one (src, dst, len).
// No cross-lane operation, no wait: every lane walks its own 16-byte slots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zccopy {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
  if (head > len) head = (uint32_t)len;
  if (lane < head) dst[lane] = src[lane];
  src += head;
  dst += head;
  len -= head;
  const uint64_t nv = len >> 4;
  uint64_t v = lane;
  // four 16-byte loads in flight per lane before their stores
  for (; v + 3 * 64 < nv; v += 4 * 64) {
    u32x4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_memcpy(&x[u], src + (v + u * 64) * 16, 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(x[u], reinterpret_cast<u32x4*>(dst + (v + u * 64) * 16));
  }
  for (; v < nv; v += 64) {
    u32x4 x;
    __builtin_memcpy(&x, src + v * 16, 16);
    __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst + v * 16));
  }
  const uint32_t t = (uint32_t)(len & 15);
  if (lane < t) dst[nv * 16 + lane] = src[nv * 16 + lane];
}

}  // namespace zccopy
