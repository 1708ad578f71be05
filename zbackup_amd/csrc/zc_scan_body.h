// The exclusive scan of a device array in three launches, shared by
// zc_resolve.hip (the records' sizes, the used flags, the entry sizes, the
// piece counts) and zc_ser.hip (the messages' lengths, the piece counts):
//
//   zc_scan_tile_sums   a workgroup per tile of kTile values: the tile's sum
//   zc_scan_tile_scan   one workgroup: the tiles' sums to exclusive prefixes
//   zc_scan_write       a workgroup per tile: out[i] = the sum of src[0 .. i)
//
// Every loop bound is a count the host fixed before the launch; the kernels are
// grid-stride; none waits on another wave or workgroup.  The kernels have
// internal linkage: each source that includes this header gets its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zcscan {

constexpr int kBlock = 256;
constexpr uint32_t kTileItems = 4;               // values per thread of a scan tile
constexpr uint32_t kTile = kBlock * kTileItems;  // values per tile

// exclusive prefix of v over the block's 256 threads (a shuffle scan per wave,
// the four waves' sums through LDS); *sum: the block's total
__device__ inline uint64_t block_prefix(uint64_t v, uint64_t* ls, uint64_t* sum) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up((unsigned long long)inc, d, 64);
    if ((int)lane >= d) inc += up;
  }
  if (lane == 63) ls[wave] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (uint32_t w = 0; w < kBlock / 64; w++) {
    if (w < wave) before += ls[w];
    all += ls[w];
  }
  __syncthreads();  // ls may be reused
  *sum = all;
  return before + inc - v;
}

template <class T>
__global__ __launch_bounds__(kBlock) void zc_scan_tile_sums(const T* __restrict__ src, uint64_t n, uint32_t ntiles,
                                                            uint64_t* __restrict__ tsum) {
  __shared__ uint64_t ls[kBlock / 64];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kTile + threadIdx.x * kTileItems;
    uint64_t v = 0;
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n) v += src[base + k];
    uint64_t sum;
    (void)block_prefix(v, ls, &sum);
    if (threadIdx.x == 0) tsum[tile] = sum;
  }
}

// one workgroup: the tiles' sums to exclusive prefixes, 256 at a time
static __global__ __launch_bounds__(kBlock) void zc_scan_tile_scan(uint64_t* __restrict__ tsum, uint32_t ntiles,
                                                                   unsigned long long* __restrict__ total) {
  __shared__ uint64_t ls[kBlock / 64];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < ntiles; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < ntiles ? tsum[i] : 0;
    uint64_t sum;
    const uint64_t pre = block_prefix(v, ls, &sum);
    if (i < ntiles) tsum[i] = carry + pre;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// out[i] = the sum of src[0 .. i); out[n] = the total (tail != 0)
template <class T>
__global__ __launch_bounds__(kBlock) void zc_scan_write(const T* __restrict__ src, uint64_t n, uint32_t ntiles,
                                                        const uint64_t* __restrict__ tsum,
                                                        uint64_t* __restrict__ out, int tail) {
  __shared__ uint64_t ls[kBlock / 64];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = (uint64_t)tile * kTile + threadIdx.x * kTileItems;
    uint64_t v = 0;
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n) v += src[base + k];
    uint64_t sum;
    uint64_t at = tsum[tile] + block_prefix(v, ls, &sum);
    for (uint32_t k = 0; k < kTileItems; k++)
      if (base + k < n) {
        out[base + k] = at;
        at += src[base + k];
        if (tail && base + k == n - 1) out[n] = at;
      }
  }
}

}  // namespace zcscan
