// zc_aes.hip -- encrypted repositories: AES-128-CBC over bundle files on the
// GPU (Encryption::encrypt / decrypt, encryption.cc:17-95) and the file
// EncryptedFile::OutputStream / InputStream put around a bundle
// (encrypted_file.cc:20-392, bundle.cc:96-218).  The cipher is zc_aes_core.h.
//
//   zc_aes_cbc_enc4_kernel CBC encryption is one serial chain per file, so the
//                          parallelism is across the chains of a call and a
//                          chain's speed is the length of one block's dependent
//                          instruction chain.  Four lanes per chain, a state
//                          column each, the other columns' words fetched with
//                          DPP quad_perm: a quarter of the instructions per
//                          block.  Trip count = the chain's block count (fixed
//                          by the host).
//   zc_aes_cbc_enc_kernel  the lane-per-chain form it replaced (2.7x slower,
//                          DESIGN 4.8), behind ZC_AES_ENC=lane for comparison;
//                          ZC_AES_CPW sets its chains per wave.
//   zc_aes_cbc_dec_kernel  CBC decryption is parallel per block, P[i] =
//                          D(C[i]) ^ C[i-1]: a streaming kernel over a flat list
//                          of (chain, first block, block count) tiles of
//                          kAesTileBlocks blocks, a block per lane per step,
//                          16-byte loads and stores, grid-stride over the list.
//                          The block before a chain's first is the chain's IV.
//   zc_bundle_parse_kernel one lane per bundle file: the two varint32 lengths,
//                          the stored Adler-32s, the padding (parse_plain).
//
// Tables in LDS, replicated across the 32 banks a ds_read_b32 lane group sees:
// entry x of lane l sits at word x * 32 + (l & 31), so every lane reads its own
// bank whatever x is (lanes l and l + 32 are served in different LDS cycles):
// no bank conflicts, 32 KiB per table.  ZC_AES_TABLE=shared selects the plain
// 1 KiB layout for comparison (DESIGN 4.8 has both rates).
//
// Every loop bound below is a count the host computed from validated lengths;
// no kernel waits on another workgroup, spins, or ends on a data value.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_device.h"
#include "zc_aes_core.h"

namespace zc {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// blocks per decrypt tile (64 KiB): the unit of the tile list
constexpr uint32_t kAesTileBlocks = 4096;
constexpr int kEncAhead = 4;      // blocks a chain's lane reads ahead
constexpr uint32_t kRepl = 32;  // table replicas = banks of a ds_read_b32 lane group

struct AesRk {
  uint32_t w[zcaes::kRkWords];
  __host__ __device__ uint32_t operator[](int i) const { return w[i]; }
};
struct AesChain {
  uint64_t in, out;  // absolute device addresses, 16-byte aligned
  uint64_t nblk;
  uint64_t pad;
  uint32_t iv[4];
};
struct AesTile {
  uint32_t chain, nblk;
  uint64_t first;
};

template <bool REPL>
struct LdsLookup {
  const uint32_t* te_;
  const uint32_t* td_;
  const uint32_t* isb_;
  uint32_t col;  // lane & 31
  __device__ uint32_t at(const uint32_t* t, uint32_t x) const { return REPL ? t[x * kRepl + col] : t[x]; }
  __device__ uint32_t te(uint32_t x) const { return at(te_, x); }
  __device__ uint32_t td(uint32_t x) const { return at(td_, x); }
  __device__ uint32_t isb(uint32_t x) const { return at(isb_, x); }
};

template <bool REPL>
__device__ inline void fill_table(uint32_t* lds, const uint32_t* __restrict__ src) {
  constexpr uint32_t kWords = REPL ? 256 * kRepl : 256;
  for (uint32_t k = threadIdx.x; k < kWords; k += blockDim.x) lds[k] = src[REPL ? k / kRepl : k];
}

// wave w of the grid takes chains [w * cpw, (w + 1) * cpw), a lane each.  A
// lane reads its chain G blocks ahead (the next group's loads ride under this
// group's rounds): one block ahead did not cover a miss to HBM.
template <bool REPL, int G>
__global__ __launch_bounds__(256) void zc_aes_cbc_enc_kernel(const AesRk rk, const AesChain* __restrict__ chains,
                                                             uint32_t n, uint32_t cpw,
                                                             const uint32_t* __restrict__ te0) {
  __shared__ uint32_t lt[REPL ? 256 * kRepl : 256];
  fill_table<REPL>(lt, te0);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t ci = wave * cpw + lane;
  if (lane >= cpw || ci >= n) return;
  const AesChain c = chains[ci];
  const LdsLookup<REPL> t{lt, nullptr, nullptr, lane & 31};
  const u32x4* in = reinterpret_cast<const u32x4*>((uintptr_t)c.in);
  u32x4* out = reinterpret_cast<u32x4*>((uintptr_t)c.out);
  uint32_t prev[4] = {c.iv[0], c.iv[1], c.iv[2], c.iv[3]};
  auto block = [&](const u32x4 p, uint64_t i) {
    uint32_t s[4] = {p[0] ^ prev[0], p[1] ^ prev[1], p[2] ^ prev[2], p[3] ^ prev[3]};
    zcaes::encrypt_block(rk, t, s);
    u32x4 o;
    o[0] = prev[0] = s[0];
    o[1] = prev[1] = s[1];
    o[2] = prev[2] = s[2];
    o[3] = prev[3] = s[3];
    out[i] = o;
  };
  const uint64_t ngroups = c.nblk / G;  // whole groups, then a tail of < G blocks
  u32x4 next[G];
  if (ngroups) {
#pragma unroll
    for (int k = 0; k < G; ++k) next[k] = in[k];
  }
  for (uint64_t g = 0; g < ngroups; ++g) {
    u32x4 cur[G];
#pragma unroll
    for (int k = 0; k < G; ++k) cur[k] = next[k];
    if (g + 1 < ngroups) {
#pragma unroll
      for (int k = 0; k < G; ++k) next[k] = in[(g + 1) * G + k];
    }
#pragma unroll
    for (int k = 0; k < G; ++k) block(cur[k], g * G + k);
  }
  for (uint64_t i = ngroups * G; i < c.nblk; ++i) block(in[i], i);
}

// The same chains, four lanes per chain: lane j of a quad holds state column j
// and fetches the three other columns' words with DPP quad_perm moves, so a
// block's dependent chain is a quarter of the lane-per-chain kernel's vector
// instructions.  Quad q of the grid takes chain q; a quad is wholly active or
// wholly done (its four lanes share the trip count), which is what DPP needs.
// rk: the 44 round-key words in device memory (lane j keeps words 4 r + j).
template <bool REPL, int G>
__global__ __launch_bounds__(256) void zc_aes_cbc_enc4_kernel(const uint32_t* __restrict__ rk,
                                                              const AesChain* __restrict__ chains, uint32_t n,
                                                              const uint32_t* __restrict__ te0) {
  __shared__ uint32_t lt[REPL ? 256 * kRepl : 256];
  fill_table<REPL>(lt, te0);
  __syncthreads();
  const uint64_t ci = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 2;
  const uint32_t j = threadIdx.x & 3;
  if (ci >= n) return;
  const uint64_t c_in = chains[ci].in, c_out = chains[ci].out, nblk = chains[ci].nblk;
  const LdsLookup<REPL> t{lt, nullptr, nullptr, threadIdx.x & 31};
  const uint32_t* in = reinterpret_cast<const uint32_t*>((uintptr_t)c_in) + j;
  uint32_t* out = reinterpret_cast<uint32_t*>((uintptr_t)c_out) + j;
  uint32_t k[zcaes::kRounds + 1];
#pragma unroll
  for (int r = 0; r <= zcaes::kRounds; ++r) k[r] = rk[4 * r + j];
  uint32_t prev = chains[ci].iv[j];
  // lane i of a quad reads lane (i + 1) & 3, (i + 2) & 3, (i + 3) & 3
#define ZC_QUAD(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xf, 0xf, false))
  auto block = [&](uint32_t p, uint64_t i) {
    uint32_t a = p ^ prev ^ k[0];
#pragma unroll
    for (int r = 1; r < zcaes::kRounds; ++r) {
      const uint32_t w1 = ZC_QUAD(a, 0x39), w2 = ZC_QUAD(a, 0x4E), w3 = ZC_QUAD(a, 0x93);
      a = t.te(a & 0xff) ^ zcaes::rotl(t.te((w1 >> 8) & 0xff), 8) ^ zcaes::rotl(t.te((w2 >> 16) & 0xff), 16) ^
          zcaes::rotl(t.te(w3 >> 24), 24) ^ k[r];
    }
    const uint32_t w1 = ZC_QUAD(a, 0x39), w2 = ZC_QUAD(a, 0x4E), w3 = ZC_QUAD(a, 0x93);
    a = (((t.te(a & 0xff) >> 8) & 0xff) | (t.te((w1 >> 8) & 0xff) & 0xff00) | ((t.te((w2 >> 16) & 0xff) & 0xff00) << 8) |
         ((t.te(w3 >> 24) & 0xff00) << 16)) ^ k[zcaes::kRounds];
    prev = a;
    out[4 * i] = a;
  };
#undef ZC_QUAD
  const uint64_t ngroups = nblk / G;
  uint32_t next[G];
  if (ngroups) {
#pragma unroll
    for (int u = 0; u < G; ++u) next[u] = in[4 * u];
  }
  for (uint64_t g = 0; g < ngroups; ++g) {
    uint32_t cur[G];
#pragma unroll
    for (int u = 0; u < G; ++u) cur[u] = next[u];
    if (g + 1 < ngroups) {
#pragma unroll
      for (int u = 0; u < G; ++u) next[u] = in[4 * ((g + 1) * G + u)];
    }
#pragma unroll
    for (int u = 0; u < G; ++u) block(cur[u], g * G + u);
  }
  for (uint64_t i = ngroups * G; i < nblk; ++i) block(in[4 * i], i);
}

template <bool REPL>
__global__ __launch_bounds__(256) void zc_aes_cbc_dec_kernel(const AesRk dk, const AesChain* __restrict__ chains,
                                                             const AesTile* __restrict__ tiles, uint32_t ntiles,
                                                             const uint32_t* __restrict__ td0,
                                                             const uint32_t* __restrict__ isb) {
  __shared__ uint32_t ltd[REPL ? 256 * kRepl : 256];
  __shared__ uint32_t lis[REPL ? 256 * kRepl : 256];
  fill_table<REPL>(ltd, td0);
  fill_table<REPL>(lis, isb);
  __syncthreads();
  const LdsLookup<REPL> t{nullptr, ltd, lis, threadIdx.x & 31};
  for (uint32_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const AesTile tile = tiles[ti];
    const AesChain& c = chains[tile.chain];
    const u32x4* in = reinterpret_cast<const u32x4*>((uintptr_t)c.in);
    u32x4* out = reinterpret_cast<u32x4*>((uintptr_t)c.out);
    for (uint32_t k = threadIdx.x; k < tile.nblk; k += 256) {
      const uint64_t b = tile.first + k;  // < c.nblk by the host's construction
      const u32x4 x = in[b];
      u32x4 pv;
      if (b)
        pv = in[b - 1];  // the previous tile's last block for k == 0
      else
        pv = u32x4{c.iv[0], c.iv[1], c.iv[2], c.iv[3]};
      uint32_t s[4] = {x[0], x[1], x[2], x[3]};
      zcaes::decrypt_block(dk, t, s);
      u32x4 o{s[0] ^ pv[0], s[1] ^ pv[1], s[2] ^ pv[2], s[3] ^ pv[3]};
      __builtin_nontemporal_store(o, out + b);
    }
  }
}

struct FileDesc {
  uint64_t addr;  // absolute device address of the plaintext
  uint64_t size;
};
struct DevBytes {
  const uint8_t* p;
  __device__ uint32_t byte(uint64_t i) const { return p[i]; }
};
__global__ __launch_bounds__(64) void zc_bundle_parse_kernel(const FileDesc* __restrict__ files, uint32_t n,
                                                             int keyed, zcaes::Parsed* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const DevBytes in{reinterpret_cast<const uint8_t*>((uintptr_t)files[i].addr)};
  zcaes::Parsed p;
  zcaes::parse_plain(in, files[i].size, keyed != 0, &p);
  out[i] = p;
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
    cap = n;
    return hipSuccess;
  }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};

struct Ext {
  uint64_t a, b;  // [a, b)
  size_t i;
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
#define ACK(x)                                             \
  do {                                                     \
    hipError_t e_ = (x);                                   \
    if (e_ != hipSuccess) return hip_error(err, e_, st);   \
  } while (0)

// sorted by start; true when two extents share a byte (*at = the later one)
bool sort_and_find_overlap(std::vector<Ext>& v, size_t* at) {
  std::sort(v.begin(), v.end(), [](const Ext& x, const Ext& y) { return x.a < y.a; });
  for (size_t k = 1; k < v.size(); k++)
    if (v[k].a < v[k - 1].b) {
      *at = v[k].i;
      return true;
    }
  return false;
}
// outs: sorted and disjoint.  The first input that shares a byte with an
// output (other than, with same_ok, input i being exactly output i)
bool inputs_touch_outputs(const std::vector<Ext>& ins, const std::vector<Ext>& outs, bool same_ok, size_t* at) {
  for (const Ext& x : ins) {
    auto it = std::upper_bound(outs.begin(), outs.end(), x.a, [](uint64_t a, const Ext& o) { return a < o.b; });
    for (; it != outs.end() && it->a < x.b; ++it) {
      if (same_ok && it->i == x.i && it->a == x.a && it->b == x.b) continue;
      *at = x.i;
      return true;
    }
  }
  return false;
}

}  // namespace

struct AesScratch {
  zcaes::Tables tab;
  Buf<uint32_t> d_tab;  // te0, td0, isb: 256 words each
  bool tab_up = false;
  Buf<AesChain> chains;
  Buf<AesTile> tiles;
  Buf<uint32_t> d_rk;           // the round keys of the call in flight
  Buf<uint8_t> h_in, h_out;     // the host forms' device copies
  Buf<uint8_t> stage;           // seal: prefixes, Adler-32s, padding
  Buf<FileDesc> fdesc;
  Buf<zcaes::Parsed> parsed;
  int cus = 0;
  uint32_t form = 0;  // the CBC kernel last launched (ZC_AES_FORM_*), set where run_cbc launches
  bool form_set = false;
  AesScratch() { zcaes::make_tables(&tab); }
};

AesScratch* aes_scratch_new() { return new AesScratch(); }
void aes_scratch_free(AesScratch* s) { delete s; }
bool aes_last_form(const AesScratch* s, uint32_t* form) {
  if (!s || !s->form_set) return false;
  *form = s->form;
  return true;
}

namespace {

void set_form(AesScratch* s, uint32_t form) {
  s->form = form;
  s->form_set = true;
}

// A compiled form: the kernel with the word zc_aes_last_form reports for it.
// The word is made from the template arguments the kernel pointer is taken
// with, so it names the instantiation that is launched, whatever selected it.
template <class K>
struct Form {
  K kernel;
  uint32_t form;
};
template <bool REPL>
constexpr uint32_t table_bit() {
  return REPL ? 0u : (uint32_t)ZC_AES_FORM_PLAIN_TABLES;
}
template <bool REPL, int G>
constexpr auto enc4_form() {
  return Form<decltype(&zc_aes_cbc_enc4_kernel<REPL, G>)>{&zc_aes_cbc_enc4_kernel<REPL, G>, table_bit<REPL>()};
}
template <bool REPL, int G>
constexpr auto lane_form() {
  return Form<decltype(&zc_aes_cbc_enc_kernel<REPL, G>)>{
      &zc_aes_cbc_enc_kernel<REPL, G>,
      ZC_AES_FORM_LANE | table_bit<REPL>() | (G == 1 ? (uint32_t)ZC_AES_FORM_AHEAD_1 : 0u)};
}
template <bool REPL>
constexpr auto dec_form() {
  return Form<decltype(&zc_aes_cbc_dec_kernel<REPL>)>{&zc_aes_cbc_dec_kernel<REPL>,
                                                      ZC_AES_FORM_DECRYPT | table_bit<REPL>()};
}

bool shared_tables() {
  const char* e = getenv("ZC_AES_TABLE");
  return e && !strcmp(e, "shared");
}

// the chains of `list` (validated: 16-byte aligned addresses, nblk >= 1) through
// the kernel of one direction; returns after the stream has drained
int run_cbc(AesScratch* s, bool decrypt, const uint8_t* key, const std::vector<AesChain>& list, hipStream_t st,
            std::string& err) {
  if (list.empty()) return ZC_OK;
  if (list.size() > 0x7fffffffull) return arg_error(err, "more than 2^31 chains");
  if (!s->cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    ACK(hipGetDevice(&dev));
    ACK(hipGetDeviceProperties(&prop, dev));
    s->cus = std::max(1, prop.multiProcessorCount);
  }
  if (!s->tab_up) {
    ACK(s->d_tab.ensure(768));
    ACK(hipMemcpyAsync(s->d_tab.p, s->tab.te0, 1024, hipMemcpyHostToDevice, st));
    ACK(hipMemcpyAsync(s->d_tab.p + 256, s->tab.td0, 1024, hipMemcpyHostToDevice, st));
    ACK(hipMemcpyAsync(s->d_tab.p + 512, s->tab.isb, 1024, hipMemcpyHostToDevice, st));
    ACK(hipStreamSynchronize(st));
    s->tab_up = true;
  }
  AesRk rk;
  if (decrypt)
    zcaes::expand_decrypt_key(s->tab, key, rk.w);
  else
    zcaes::expand_encrypt_key(s->tab, key, rk.w);
  const uint32_t n = (uint32_t)list.size();
  ACK(s->chains.ensure(n));
  ACK(hipMemcpyAsync(s->chains.p, list.data(), n * sizeof(AesChain), hipMemcpyHostToDevice, st));
  const bool shared = shared_tables();
  if (!decrypt) {
    const char* mode = getenv("ZC_AES_ENC");  // measurements: "lane" = the lane-per-chain kernel
    if (!(mode && !strcmp(mode, "lane"))) {
      ACK(s->d_rk.ensure(zcaes::kRkWords));
      ACK(hipMemcpyAsync(s->d_rk.p, rk.w, sizeof rk.w, hipMemcpyHostToDevice, st));
      const dim3 grid((uint32_t)((4ull * n + 255) / 256)), block(256);
      const auto f = shared ? enc4_form<false, kEncAhead>() : enc4_form<true, kEncAhead>();
      hipLaunchKernelGGL(f.kernel, grid, block, 0, st, s->d_rk.p, s->chains.p, n, s->d_tab.p);
      ACK(hipGetLastError());
      set_form(s, f.form);
      ACK(hipStreamSynchronize(st));  // rk's host memory is reused
      return ZC_OK;
    }
    uint32_t cpw = 64;  // chains per wave: full waves measured best
    if (const char* e = getenv("ZC_AES_CPW")) {  // measurements: chains per wave
      const unsigned long v = strtoul(e, nullptr, 10);
      if (v >= 1 && v <= 64) cpw = (uint32_t)v;
    }
    const uint32_t waves = (n + cpw - 1) / cpw;
    const dim3 grid((waves + 3) / 4), block(256);
    const char* pf = getenv("ZC_AES_PREFETCH");  // measurements: "1" = one block ahead
    const bool one = pf && !strcmp(pf, "1");
    const auto f = shared ? (one ? lane_form<false, 1>() : lane_form<false, kEncAhead>())
                          : (one ? lane_form<true, 1>() : lane_form<true, kEncAhead>());
    hipLaunchKernelGGL(f.kernel, grid, block, 0, st, rk, s->chains.p, n, cpw, s->d_tab.p);
    ACK(hipGetLastError());
    set_form(s, f.form | cpw << ZC_AES_FORM_CPW_SHIFT);  // cpw: the launch's own argument
    ACK(hipStreamSynchronize(st));
    return ZC_OK;
  }
  std::vector<AesTile> tiles;
  for (uint32_t i = 0; i < n; i++)
    for (uint64_t f = 0; f < list[i].nblk; f += kAesTileBlocks)
      tiles.push_back(AesTile{i, (uint32_t)std::min<uint64_t>(kAesTileBlocks, list[i].nblk - f), f});
  if (tiles.size() > 0xffffffffull) return arg_error(err, "more than 2^32 tiles of 64 KiB");
  ACK(s->tiles.ensure(tiles.size()));
  ACK(hipMemcpyAsync(s->tiles.p, tiles.data(), tiles.size() * sizeof(AesTile), hipMemcpyHostToDevice, st));
  const uint32_t nt = (uint32_t)tiles.size();
  const dim3 grid(std::min<uint32_t>(nt, 2u * (uint32_t)s->cus)), block(256);
  const auto f = shared ? dec_form<false>() : dec_form<true>();
  hipLaunchKernelGGL(f.kernel, grid, block, 0, st, rk, s->chains.p, s->tiles.p, nt, s->d_tab.p + 256, s->d_tab.p + 512);
  ACK(hipGetLastError());
  set_form(s, f.form);
  ACK(hipStreamSynchronize(st));  // the lists' host memory is reused
  return ZC_OK;
}

int order_after_default(hipEvent_t ev_in, hipStream_t st, std::string& err) {
  if (!ev_in) return ZC_OK;
  ACK(hipEventRecord(ev_in, nullptr));
  ACK(hipStreamWaitEvent(st, ev_in, 0));
  return ZC_OK;
}

uint64_t lo_of(const uint64_t* off, size_t n) { return n ? *std::min_element(off, off + n) : 0; }

}  // namespace

int aes_cbc(AesScratch* s, bool decrypt, bool host, const uint8_t* key, const void* in, const uint64_t* in_off,
            const uint64_t* len, size_t n, const uint8_t* iv, void* out, const uint64_t* out_off, hipEvent_t ev_in,
            hipStream_t st, std::string& err) {
  if (!key) return arg_error(err, "null key");
  if (n && (!in || !in_off || !len || !out || !out_off)) return arg_error(err, "null pointer");
  if (!n) return ZC_OK;
  if (!host && (((uintptr_t)in | (uintptr_t)out) & 15)) return arg_error(err, "a base pointer is not 16-byte aligned");
  std::vector<Ext> ins(n), outs(n);
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (chain " + std::to_string(i) + ")";
    if (len[i] == 0) return arg_error(err, "a chain of 0 bytes" + at);
    if (len[i] % 16) return arg_error(err, "a length that is not a multiple of 16" + at);
    if ((in_off[i] | out_off[i]) % 16) return arg_error(err, "an offset that is not 16-byte aligned" + at);
    const uint64_t a = (uint64_t)(uintptr_t)in + in_off[i], o = (uint64_t)(uintptr_t)out + out_off[i];
    if (a + len[i] < a || o + len[i] < o) return arg_error(err, "an extent wraps the address space" + at);
    ins[i] = Ext{a, a + len[i], i};
    outs[i] = Ext{o, o + len[i], i};
  }
  size_t bad = 0;
  if (sort_and_find_overlap(outs, &bad))
    return arg_error(err, "output extents overlap (chain " + std::to_string(bad) + ")");
  if (inputs_touch_outputs(ins, outs, !decrypt, &bad))
    return arg_error(err, std::string(decrypt ? "an input extent overlaps an output extent: decryption reads its "
                                                "neighbours' ciphertext, so it cannot run in place"
                                              : "an input extent overlaps another chain's output extent") +
                              " (chain " + std::to_string(bad) + ")");
  const uint8_t* d_in = (const uint8_t*)in;
  uint8_t* d_out = (uint8_t*)out;
  uint64_t in_lo = 0, out_lo = 0;
  if (host) {
    in_lo = lo_of(in_off, n);
    out_lo = lo_of(out_off, n);
    uint64_t in_hi = 0, out_hi = 0;
    for (size_t i = 0; i < n; i++) {
      in_hi = std::max(in_hi, in_off[i] + len[i]);
      out_hi = std::max(out_hi, out_off[i] + len[i]);
    }
    ACK(s->h_in.ensure(in_hi - in_lo));
    ACK(s->h_out.ensure(out_hi - out_lo));
    ACK(hipMemcpyAsync(s->h_in.p, (const uint8_t*)in + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, st));
    d_in = s->h_in.p;
    d_out = s->h_out.p;
  } else {
    const int rc = order_after_default(ev_in, st, err);
    if (rc) return rc;
  }
  std::vector<AesChain> list(n);
  for (size_t i = 0; i < n; i++) {
    AesChain& c = list[i];
    c.in = (uint64_t)(uintptr_t)d_in + in_off[i] - in_lo;
    c.out = (uint64_t)(uintptr_t)d_out + out_off[i] - out_lo;
    c.nblk = len[i] / 16;
    c.pad = 0;
    if (iv)
      memcpy(c.iv, iv + 16 * i, 16);
    else
      memset(c.iv, 0, 16);
  }
  const int rc = run_cbc(s, decrypt, key, list, st, err);
  if (rc) return rc;
  if (host) {
    for (size_t i = 0; i < n; i++)
      ACK(hipMemcpyAsync((uint8_t*)out + out_off[i], s->h_out.p + (out_off[i] - out_lo), len[i],
                         hipMemcpyDeviceToHost, st));
    ACK(hipStreamSynchronize(st));
  }
  return ZC_OK;
}

int bundle_seal(AesScratch* s, LzoScratch* lz, bool host, const uint8_t* key, const void* prefix,
                const zc_bundle_file* files, size_t n, const void* body, void* files_out, uint64_t* file_size,
                hipEvent_t ev_in, hipStream_t st, std::string& err) {
  if (n && (!files || !files_out || !file_size)) return arg_error(err, "null pointer");
  if (!n) return ZC_OK;
  if (!host && ((uintptr_t)files_out & 15)) return arg_error(err, "d_files is not 16-byte aligned");
  const bool keyed = key != nullptr;
  std::vector<Ext> exts(n);
  uint64_t stage_bytes = 0, f_lo = ~0ull, f_hi = 0, b_lo = ~0ull, b_hi = 0;
  for (size_t i = 0; i < n; i++) {
    const zc_bundle_file& f = files[i];
    const std::string at = " (bundle " + std::to_string(i) + ")";
    if (f.prefix_len && !prefix) return arg_error(err, "null prefix blob" + at);
    if (f.body_len && !body) return arg_error(err, "null body buffer" + at);
    if (f.file_off % 16) return arg_error(err, "a file offset that is not 16-byte aligned" + at);
    if (f.prefix_len > (1ull << 40) || f.body_len > (1ull << 40)) return arg_error(err, "a length over 2^40" + at);
    file_size[i] = zcaes::bundle_file_size(f.prefix_len, f.body_len, keyed);
    const uint64_t a = (uint64_t)(uintptr_t)files_out + f.file_off;
    if (a + file_size[i] < a) return arg_error(err, "a file wraps the address space" + at);
    exts[i] = Ext{a, a + file_size[i], i};
    stage_bytes += f.prefix_len + 4 + 4 + 16;
    f_lo = std::min(f_lo, f.file_off);
    f_hi = std::max(f_hi, f.file_off + file_size[i]);
    if (f.body_len) {
      b_lo = std::min(b_lo, f.body_off);
      b_hi = std::max(b_hi, f.body_off + f.body_len);
    }
  }
  size_t bad = 0;
  if (sort_and_find_overlap(exts, &bad)) return arg_error(err, "files overlap (bundle " + std::to_string(bad) + ")");
  if (b_lo > b_hi) b_lo = b_hi = 0;  // no body bytes at all
  const uint8_t* d_body = (const uint8_t*)body;
  uint8_t* d_files = (uint8_t*)files_out;
  if (host) {
    ACK(s->h_in.ensure(b_hi - b_lo));
    ACK(s->h_out.ensure(f_hi - f_lo));
    if (b_hi > b_lo)
      ACK(hipMemcpyAsync(s->h_in.p, (const uint8_t*)body + b_lo, b_hi - b_lo, hipMemcpyHostToDevice, st));
    d_body = s->h_in.p;
    d_files = s->h_out.p;
  } else {
    b_lo = f_lo = 0;
    const int rc = order_after_default(ev_in, st, err);
    if (rc) return rc;
  }
  // the bodies' Adler-32 shares on the device
  std::vector<uint64_t> boff(n), blen(n), fdst(n);
  std::vector<uint32_t> bad32(n);
  for (size_t i = 0; i < n; i++) {
    boff[i] = files[i].body_len ? files[i].body_off - b_lo : 0;
    blen[i] = files[i].body_len;
    fdst[i] = files[i].file_off - f_lo + files[i].prefix_len + 4;
  }
  ACK(lzo_adler32(lz, d_body ? d_body : d_files, boff.data(), blen.data(), n, bad32.data(), st));
  // everything but the bodies, built on the host and uploaded in one copy:
  // per bundle the head (prefix, A1) and the tail (A2, padding)
  std::vector<uint8_t> blob(stage_bytes);
  std::vector<uint64_t> soff(2 * n), ssize(2 * n), sdst(2 * n);
  uint64_t pos = 0;
  for (size_t i = 0; i < n; i++) {
    const zc_bundle_file& f = files[i];
    const uint64_t P = f.prefix_len, B = f.body_len;
    uint8_t* h = blob.data() + pos;
    if (P) memcpy(h, (const uint8_t*)prefix + f.prefix_off, P);
    const uint32_t a1 = zcaes::adler32_host(h, P);
    for (int k = 0; k < 4; k++) h[P + k] = (uint8_t)(a1 >> (8 * k));
    const uint32_t a2 = zcaes::adler32_join(zcaes::adler32_host(h + P, 4, a1), bad32[i], B);
    uint8_t* t = h + P + 4;
    for (int k = 0; k < 4; k++) t[k] = (uint8_t)(a2 >> (8 * k));
    const uint64_t npad = file_size[i] - (P + B + 8);  // 0 without a key, else 1..16
    memset(t + 4, (int)npad, npad);
    soff[2 * i] = pos;
    ssize[2 * i] = P + 4;
    sdst[2 * i] = f.file_off - f_lo;
    soff[2 * i + 1] = pos + P + 4;
    ssize[2 * i + 1] = 4 + npad;
    sdst[2 * i + 1] = f.file_off - f_lo + P + 4 + B;
    pos += P + 4 + 4 + 16;
  }
  ACK(s->stage.ensure(stage_bytes));
  ACK(hipMemcpyAsync(s->stage.p, blob.data(), stage_bytes, hipMemcpyHostToDevice, st));
  ACK(lzo_scatter(lz, s->stage.p, soff.data(), ssize.data(), 2 * n, d_files, sdst.data(), st));
  ACK(lzo_scatter(lz, d_body, boff.data(), blen.data(), n, d_files, fdst.data(), st));
  if (keyed) {
    std::vector<AesChain> list(n);
    for (size_t i = 0; i < n; i++) {
      list[i] = AesChain{};
      list[i].in = list[i].out = (uint64_t)(uintptr_t)d_files + files[i].file_off - f_lo;
      list[i].nblk = file_size[i] / 16;
    }
    const int rc = run_cbc(s, false, key, list, st, err);
    if (rc) return rc;
  }
  if (host) {
    for (size_t i = 0; i < n; i++)
      ACK(hipMemcpyAsync((uint8_t*)files_out + files[i].file_off, d_files + (files[i].file_off - f_lo), file_size[i],
                         hipMemcpyDeviceToHost, st));
    ACK(hipStreamSynchronize(st));
  }
  return ZC_OK;
}

int bundle_unseal(AesScratch* s, LzoScratch* lz, bool host, const uint8_t* key, const void* files,
                  const uint64_t* file_off, const uint64_t* file_size, size_t n, void* plain,
                  const uint64_t* plain_off, zc_bundle_layout* layout, hipEvent_t ev_in, hipStream_t st,
                  std::string& err) {
  if (n && (!files || !file_off || !file_size || !plain || !plain_off || !layout)) return arg_error(err, "null pointer");
  if (!n) return ZC_OK;
  if (n > 0x7fffffffull) return arg_error(err, "more than 2^31 files");
  const bool keyed = key != nullptr;
  if (keyed && !host && (((uintptr_t)files | (uintptr_t)plain) & 15))
    return arg_error(err, "a base pointer is not 16-byte aligned");
  std::vector<Ext> ins, outs;
  uint64_t f_lo = ~0ull, f_hi = 0, p_lo = ~0ull, p_hi = 0;
  for (size_t i = 0; i < n; i++) {
    const std::string at = " (file " + std::to_string(i) + ")";
    if (keyed && (file_off[i] | plain_off[i]) % 16) return arg_error(err, "an offset that is not 16-byte aligned" + at);
    const uint64_t a = (uint64_t)(uintptr_t)files + file_off[i], o = (uint64_t)(uintptr_t)plain + plain_off[i];
    if (a + file_size[i] < a || o + file_size[i] < o) return arg_error(err, "an extent wraps the address space" + at);
    if (!file_size[i]) continue;
    ins.push_back(Ext{a, a + file_size[i], i});
    outs.push_back(Ext{o, o + file_size[i], i});
    f_lo = std::min(f_lo, file_off[i]);
    f_hi = std::max(f_hi, file_off[i] + file_size[i]);
    p_lo = std::min(p_lo, plain_off[i]);
    p_hi = std::max(p_hi, plain_off[i] + file_size[i]);
  }
  size_t bad = 0;
  if (sort_and_find_overlap(outs, &bad))
    return arg_error(err, "plaintext extents overlap (file " + std::to_string(bad) + ")");
  if (inputs_touch_outputs(ins, outs, false, &bad))
    return arg_error(err, "a file overlaps a plaintext extent (file " + std::to_string(bad) + ")");
  if (f_lo > f_hi) f_lo = f_hi = p_lo = p_hi = 0;  // only empty files
  const uint8_t* d_files = (const uint8_t*)files;
  uint8_t* d_plain = (uint8_t*)plain;
  if (host) {
    ACK(s->h_in.ensure(f_hi - f_lo));
    ACK(s->h_out.ensure(p_hi - p_lo));
    if (f_hi > f_lo)
      ACK(hipMemcpyAsync(s->h_in.p, (const uint8_t*)files + f_lo, f_hi - f_lo, hipMemcpyHostToDevice, st));
    d_files = s->h_in.p;
    d_plain = s->h_out.p;
  } else {
    f_lo = p_lo = 0;
    const int rc = order_after_default(ev_in, st, err);
    if (rc) return rc;
  }
  // files of a size the reader refuses are left alone (exIncorrectFileSize)
  std::vector<size_t> good;
  for (size_t i = 0; i < n; i++)
    if (file_size[i] && !(keyed && file_size[i] % 16)) good.push_back(i);
  if (keyed) {
    std::vector<AesChain> list(good.size());
    for (size_t k = 0; k < good.size(); k++) {
      const size_t i = good[k];
      list[k] = AesChain{};
      list[k].in = (uint64_t)(uintptr_t)d_files + file_off[i] - f_lo;
      list[k].out = (uint64_t)(uintptr_t)d_plain + plain_off[i] - p_lo;
      list[k].nblk = file_size[i] / 16;
    }
    const int rc = run_cbc(s, true, key, list, st, err);
    if (rc) return rc;
  } else {
    std::vector<uint64_t> so, sz, dst;
    for (size_t i : good) {
      so.push_back(file_off[i] - f_lo);
      sz.push_back(file_size[i]);
      dst.push_back(plain_off[i] - p_lo);
    }
    ACK(lzo_scatter(lz, d_files, so.data(), sz.data(), so.size(), d_plain, dst.data(), st));
  }
  // the lengths, stored Adler-32s and padding of every file, a lane each
  std::vector<FileDesc> fd(n);
  for (size_t i = 0; i < n; i++) fd[i] = FileDesc{(uint64_t)(uintptr_t)d_plain + plain_off[i] - p_lo, file_size[i]};
  std::vector<zcaes::Parsed> parsed(n);
  ACK(s->fdesc.ensure(n));
  ACK(s->parsed.ensure(n));
  ACK(hipMemcpyAsync(s->fdesc.p, fd.data(), n * sizeof(FileDesc), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(zc_bundle_parse_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, st, s->fdesc.p, (uint32_t)n,
                     keyed ? 1 : 0, s->parsed.p);
  ACK(hipGetLastError());
  ACK(hipMemcpyAsync(parsed.data(), s->parsed.p, n * sizeof(zcaes::Parsed), hipMemcpyDeviceToHost, st));
  ACK(hipStreamSynchronize(st));
  // both Adler-32s: the share before A1, and the share from A1 to A2
  std::vector<uint64_t> aoff, alen;
  std::vector<size_t> who;
  for (size_t i = 0; i < n; i++) {
    const zcaes::Parsed& p = parsed[i];
    if (p.status != zcaes::kBundleOk) continue;
    who.push_back(i);
    aoff.push_back(plain_off[i] - p_lo);
    alen.push_back(p.a1_off);
    aoff.push_back(plain_off[i] - p_lo + p.a1_off);
    alen.push_back(4 + p.body_len);
  }
  std::vector<uint32_t> ad(aoff.size());
  ACK(lzo_adler32(lz, d_plain, aoff.data(), alen.data(), aoff.size(), ad.data(), st));
  for (size_t k = 0; k < who.size(); k++) {
    zcaes::Parsed& p = parsed[who[k]];
    if (ad[2 * k] != p.a1)
      p.status = zcaes::kBundleAdler1;
    else if (zcaes::adler32_join(ad[2 * k], ad[2 * k + 1], alen[2 * k + 1]) != p.a2)
      p.status = zcaes::kBundleAdler2;
  }
  for (size_t i = 0; i < n; i++) {
    const zcaes::Parsed& p = parsed[i];
    layout[i] = zc_bundle_layout{p.status,   0,          p.header_off, p.header_len,
                                 p.info_off, p.info_len, p.body_off,   p.body_len};
  }
  if (host) {
    for (size_t i : good)
      ACK(hipMemcpyAsync((uint8_t*)plain + plain_off[i], d_plain + (plain_off[i] - p_lo), file_size[i],
                         hipMemcpyDeviceToHost, st));
    ACK(hipStreamSynchronize(st));
  }
  return ZC_OK;
}

static_assert(ZC_BUNDLE_OK == zcaes::kBundleOk && ZC_BUNDLE_BAD_SIZE == zcaes::kBundleBadSize &&
                  ZC_BUNDLE_TRUNCATED == zcaes::kBundleTruncated && ZC_BUNDLE_BAD_ADLER1 == zcaes::kBundleAdler1 &&
                  ZC_BUNDLE_BAD_ADLER2 == zcaes::kBundleAdler2 && ZC_BUNDLE_BAD_PADDING == zcaes::kBundleBadPadding,
              "bundle status codes");

}  // namespace zc
