// A/B of scan variants, interleaved in one process: the product zc_scan_kernel
// built with different -D ZC_*_CFG switches (scan_variant.hip, one object per
// variant, tools/ubench/make_geom_ab.sh), 8 GiB of seeded random bytes.
// Compared across the variants (identical in every one): the span digests, the
// directory (base and count of every wave-tile) and the anchor pool (position
// and gear word of every anchor).  A variant named "(probe)" hashes the wrong
// bytes on purpose (timing only) and is left out of the comparison.
//
// After the timed rounds the stamped builds (-DZC_SCAN_STAMP_CFG=1) run once
// each: every wave leaves its start and end clock, its hardware ids and the
// number of wave-tiles it walked, and the tool prints per XCD, SE and CU the
// workgroups hosted, the mean and max end time and the mean wave lifetime over
// the launch time.  Tooling only.
//
//   scan_geom_ab [bytes [rounds [cu-table 0/1]]]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

typedef hipError_t (*ScanFn)(const uint8_t*, uint64_t, uint64_t, uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*,
                             uint32_t, unsigned long long*, uint32_t*, uint32_t, uint32_t*);
#define DECL(N) extern "C" hipError_t N(const uint8_t*, uint64_t, uint64_t, uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t, unsigned long long*, uint32_t*, uint32_t, uint32_t*);
DECL(scan_v_parent) DECL(scan_v_claim) DECL(scan_v_roll) DECL(scan_v_prod) DECL(scan_v_parent_stamp) DECL(scan_v_prod_stamp)
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__global__ void fill(uint8_t* d, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 8; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    ((uint64_t*)d)[i] = z ^ (z >> 31);
  }
}

constexpr uint32_t kStampWaves = 16384;  // room for every geometry built (8 words each)

struct V {
  const char* name;
  ScanFn f;
  bool stamp;
  uint64_t* blk = nullptr;
  uint32_t *dbase = nullptr, *dcnt = nullptr, *prel = nullptr, *pg = nullptr, *claim = nullptr;
  uint32_t claim_base = 0;
  std::vector<float> t;
  unsigned long long pool = 0;
};

// the stamps of one launch: per XCD, per SE and (cu_table) per CU
static void report(const char* name, const std::vector<uint32_t>& st, bool cu_table) {
  struct W { uint64_t t0, t1; uint32_t xcc, se, cu, tiles, gw; };
  std::vector<W> ws;
  for (uint32_t i = 0; i < kStampWaves; ++i) {
    const uint32_t* s = &st[8 * i];
    const uint64_t t0 = s[0] | ((uint64_t)s[1] << 32), t1 = s[2] | ((uint64_t)s[3] << 32);
    if (!t1) continue;
    // HW_ID: cu_id bits 11:8, sh_id 12, se_id 15:13; XCC_ID: bits 3:0
    ws.push_back(W{t0, t1, s[5] & 15u, (s[4] >> 13) & 7u, (s[4] >> 8) & 31u, s[6], s[7]});
  }
  if (ws.empty()) { printf("%s: no stamps\n", name); return; }
  uint64_t lo = ~0ull, hi = 0;
  uint32_t tmin = ~0u, tmax = 0;
  for (auto& w : ws) {
    lo = std::min(lo, w.t0); hi = std::max(hi, w.t1);
    if (w.tiles) { tmin = std::min(tmin, w.tiles); tmax = std::max(tmax, w.tiles); }
  }
  const double span = (double)(hi - lo);  // 100 MHz ticks
  printf("== stamps: %s: %zu waves, launch %.1f us, tiles per wave %u..%u\n", name, ws.size(), span / 100, tmin, tmax);
  struct Agg { std::map<uint32_t, int> wgs; double end = 0, life = 0, endmax = 0; int n = 0; };
  auto add = [&](Agg& a, const W& w) {
    a.wgs[w.gw / 4]++;
    a.end += (double)(w.t1 - lo); a.endmax = std::max(a.endmax, (double)(w.t1 - lo));
    a.life += (double)(w.t1 - w.t0); a.n++;
  };
  std::map<uint32_t, Agg> xcd;
  std::map<std::pair<uint32_t, uint32_t>, Agg> se;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, Agg> cu;
  Agg all;
  for (auto& w : ws) {
    add(all, w); add(xcd[w.xcc], w); add(se[{w.xcc, w.se}], w); add(cu[{w.xcc, w.se, w.cu}], w);
  }
  auto line = [&](const char* what, const Agg& a) {
    printf("%-14s wgs %4zu  end mean %7.1f us max %7.1f us  lifetime/launch %.4f\n", what, a.wgs.size(),
           a.end / a.n / 100, a.endmax / 100, a.life / a.n / span);
  };
  line("all", all);
  char b[64];
  for (auto& [k, a] : xcd) { snprintf(b, sizeof b, "xcd %u", k); line(b, a); }
  for (auto& [k, a] : se) { snprintf(b, sizeof b, "xcd %u se %u", k.first, k.second); line(b, a); }
  std::map<size_t, int> hist;
  for (auto& [k, a] : cu) hist[a.wgs.size()]++;
  printf("CUs seen %zu; workgroups per CU:", cu.size());
  for (auto& [k, c] : hist) printf("  %zu wgs on %d CUs", k, c);
  printf("\n");
  if (cu_table)
    for (auto& [k, a] : cu) {
      snprintf(b, sizeof b, "x%u s%u cu%2u", std::get<0>(k), std::get<1>(k), std::get<2>(k));
      line(b, a);
    }
}

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], 0, 0) : (8ull << 30);
  const int rounds = argc > 2 ? atoi(argv[2]) : 25;
  const bool cu_table = argc > 3 ? atoi(argv[3]) != 0 : true;
  // sized for the smallest geometry built (2 KiB lane spans: 128 KiB
  // wave-tiles, 128 pool entries each); each variant launches its own tiles
  const uint64_t ntiles = n / (2ull << 20), nwt = n / (128ull << 10), nblk = n / 1024;
  const uint32_t wcap = 2u * ((1u << 18) / 4096) + 64u;
  uint8_t* d; CK(hipMalloc(&d, n));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, d, n);
  std::vector<V> vs = {{"parent (static stride, re-prime all)", scan_v_parent, false},
                       {"claim only", scan_v_claim, false},
                       {"roll-on only", scan_v_roll, false},
                       {"product (claim + roll-on)", scan_v_prod, false},
                       {"parent, stamped", scan_v_parent_stamp, true},
                       {"product, stamped", scan_v_prod_stamp, true}};
  unsigned long long* cnt; uint32_t* stamp;
  CK(hipMalloc(&cnt, 64)); CK(hipMalloc(&stamp, kStampWaves * 32));
  for (auto& v : vs) {
    CK(hipMalloc(&v.blk, nblk * 8)); CK(hipMalloc(&v.dbase, nwt * 4)); CK(hipMalloc(&v.dcnt, nwt * 4));
    CK(hipMalloc(&v.prel, nwt * wcap * 4)); CK(hipMalloc(&v.pg, nwt * wcap * 4)); CK(hipMalloc(&v.claim, 4));
    CK(hipMemset(v.dbase, 0, nwt * 4)); CK(hipMemset(v.dcnt, 0, nwt * 4)); CK(hipMemset(v.claim, 0, 4));
  }
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  auto run = [&](V& v, uint32_t* st, float* ms) -> int {
    CK(hipMemset(cnt, 0, 64));
    CK(hipEventRecord(a));
    CK(v.f(d, n, ntiles, v.blk, v.dbase, v.dcnt, v.prel, v.pg, wcap, cnt, v.claim, v.claim_base, st));
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(ms, a, b));
    CK(hipMemcpy(&v.pool, cnt, 8, hipMemcpyDeviceToHost));  // CNT_POOL is counter 0
    CK(hipMemcpy(&v.claim_base, v.claim, 4, hipMemcpyDeviceToHost));  // the next launch's base
    return 0;
  };
  for (int r = 0; r < rounds; ++r)
    for (auto& v : vs) {
      if (v.stamp) continue;
      float ms;
      if (run(v, nullptr, &ms)) return 1;
      if (r) v.t.push_back(ms);
    }
  // the stamped builds: one warm launch without stamps, one with
  for (auto& v : vs) {
    if (!v.stamp) continue;
    float ms;
    if (run(v, nullptr, &ms)) return 1;
    CK(hipMemset(stamp, 0, kStampWaves * 32));
    if (run(v, stamp, &ms)) return 1;
    v.t.push_back(ms);
    std::vector<uint32_t> st(kStampWaves * 8);
    CK(hipMemcpy(st.data(), stamp, kStampWaves * 32, hipMemcpyDeviceToHost));
    report(v.name, st, cu_table);
  }
  std::vector<uint64_t> h0(nblk), h1(nblk);
  std::vector<uint32_t> b0(nwt), c0(nwt), r0(nwt * wcap), g0(nwt * wcap), b1(nwt), c1(nwt), r1(nwt * wcap), g1(nwt * wcap);
  CK(hipMemcpy(h0.data(), vs[0].blk, nblk * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(b0.data(), vs[0].dbase, nwt * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(c0.data(), vs[0].dcnt, nwt * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(r0.data(), vs[0].prel, nwt * wcap * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(g0.data(), vs[0].pg, nwt * wcap * 4, hipMemcpyDeviceToHost));
  bool same = true, dir_same = true, pool_same = true;
  for (auto& v : vs) {
    const bool probe = strstr(v.name, "(probe)") != nullptr;  // a timing probe hashes the wrong bytes
    CK(hipMemcpy(h1.data(), v.blk, nblk * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b1.data(), v.dbase, nwt * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(c1.data(), v.dcnt, nwt * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(r1.data(), v.prel, nwt * wcap * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g1.data(), v.pg, nwt * wcap * 4, hipMemcpyDeviceToHost));
    if (!probe) {
      same = same && h0 == h1;
      dir_same = dir_same && b0 == b1 && c0 == c1;
      // every stored anchor: the wave-tile's share [base, base + count)
      for (uint64_t t = 0; t < nwt && b0 == b1 && c0 == c1; ++t) {
        if (c0[t] == 0xFFFFFFFFu) continue;  // left for the exact rescan: nothing stored
        for (uint64_t i = b0[t]; i < (uint64_t)b0[t] + c0[t] && i < nwt * wcap; ++i)
          pool_same = pool_same && r0[i] == r1[i] && g0[i] == g1[i];
      }
    }
    std::sort(v.t.begin(), v.t.end());
    printf("%-38s median %7.3f ms  min %7.3f ms  %7.1f GB/s (min)  pool %llu%s\n", v.name, v.t[v.t.size() / 2], v.t[0],
           n / (v.t[0] * 1e6), v.pool, v.stamp ? "  (one stamped launch)" : "");
  }
  printf(same ? "span digests identical\n" : "SPAN DIGESTS DIFFER\n");
  printf(dir_same ? "directory identical\n" : "DIRECTORY DIFFERS\n");
  printf(pool_same ? "anchor pool identical\n" : "ANCHOR POOL DIFFERS\n");
  return same && dir_same && pool_same ? 0 : 2;
}
