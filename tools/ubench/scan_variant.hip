// One variant of the product scan (zc_kernels.hip built with the -D ZC_*_CFG
// switches of zc_device.h / zc_kernels.hip and -Dzc=<namespace>), exported as
// the C entry SCAN_ENTRY for scan_geom_ab.hip.  Tooling only.
#include "../../zbackup_amd/csrc/zc_kernels.hip"
// claim: the variant's claim counter (a device word, zero before the first
// launch) and its value before this launch.  stamp: with -DZC_SCAN_STAMP_CFG=1,
// 8 words per wave of the launch (start clock, end clock, HW_ID, XCC_ID, tiles
// walked, global wave), or null; other builds ignore it.
extern "C" hipError_t SCAN_ENTRY(const uint8_t* d, uint64_t n, uint64_t ntiles, uint64_t* blk, uint32_t* base,
                                 uint32_t* cnt, uint32_t* rel, uint32_t* g, uint32_t wcap,
                                 unsigned long long* counters, uint32_t* claim, uint32_t claim_base,
                                 uint32_t* stamp) {
  // this variant's own tile geometry (the lane span sets the tile size)
  (void)ntiles;
  (void)wcap;
#if ZC_SCAN_STAMP_CFG
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(zc::g_scan_stamp), &stamp, sizeof(stamp));
  if (e != hipSuccess) return e;
#else
  (void)stamp;
#endif
  const zc::PoolOut po{base, cnt, rel, g, zc::wave_tile_cap(65536), 0};
  return zc::launch_scan_tiles(d, n, 0, n / zc::ZC_STILE, zc::anchor_lo_for(65536), blk, po, counters, 0,
                               zc::GridKeysOut{nullptr, nullptr, 0, 0}, nullptr, nullptr, 0, nullptr,
                               zc::ScanClaim{claim, claim_base});
}
