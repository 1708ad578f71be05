// zc_ser.hip -- a backup's records serialized in HBM: the BackupInstruction
// stream of zc_serialize_records, written where the stream's bytes already lie
// (zc_ser_core.h has the definitions; the host function is the reference):
//
//   zc_ser_sizes   a lane per record: its message's length and the copies of
//                  its payload (pieces of 64 KiB, a big record's only)
//   the three scan kernels (zc_scan_body.h) over the lengths -- the position of
//                  every message -- and, when a record is big, over the pieces
//   zc_ser_write   a wave per group of 64 consecutive records: every lane builds
//                  its header, a chunk's id comes from the record, a payload of
//                  at most kStage bytes from the stream, all into LDS at the
//                  output's 16-byte phase; the run is flushed with 16-byte
//                  stores, its first and last partial slot with byte stores
//   zc_ser_copy    a wave per piece of a big payload: the record by binary
//                  search over the scan, then zccopy::wave_copy
//
// A group's output range is contiguous, and so is a run's (zc_ser_core.h); the
// 16-byte slots at a run's two ends are shared with the neighbouring group or
// with a big payload, so only the run's own bytes are stored there.  Every
// loop bound is a count the host fixed before the launch or a constant of
// zc_ser_core.h; every kernel is grid-stride; no kernel waits on another wave
// or workgroup or spins.  The host has checked every range against the stream
// and the sum of the lengths against the room before the first launch, with
// the functions the kernels use.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/zchunk.h"
#define ZC_HD __host__ __device__
#include "zc_copy_body.h"
#include "zc_device.h"
#include "zc_scan_body.h"
#include "zc_ser_core.h"

static_assert(sizeof(zc_record) == 40, "zc_record is read as ten 32-bit words");
static_assert(ZC_BYTES == zcser::kKindBytes, "record kinds");

namespace zc {

namespace {

constexpr int kBlock = zcscan::kBlock;
constexpr uint64_t kCountLimit = 0xffffffffull;  // counts stay below 2^32 - 1
// a run in LDS: its bytes behind the output's phase (at most 15), in whole slots
constexpr uint32_t kLdsBytes = (15 + zcser::kRunMax + 15) / 16 * 16;

typedef zccopy::u32x4 u32x4;

__device__ __forceinline__ zcser::Rec load_rec(const uint2* __restrict__ recs, uint64_t i) {
  const uint2* p = recs + 5 * i;
  const uint2 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
  zcser::Rec r;
  r.offset = (uint64_t)a.x | (uint64_t)a.y << 32;
  r.size = b.x;
  r.kind = b.y;
  r.rolling = (uint64_t)c.x | (uint64_t)c.y << 32;
  r.sha[0] = d.x;
  r.sha[1] = d.y;
  r.sha[2] = e.x;
  r.sha[3] = e.y;
  return r;
}

__global__ __launch_bounds__(kBlock) void zc_ser_sizes(const uint2* __restrict__ recs, uint64_t n,
                                                       uint64_t* __restrict__ len, uint32_t* __restrict__ pc) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {  // bound: n
    const uint2 sk = recs[5 * i + 1];
    len[i] = zcser::message_len(sk.y, sk.x);
    pc[i] = zcser::pieces(sk.y, sk.x);
  }
}

// pos: the exclusive scan of the lengths, pos[n] their sum; groups = ceil(n / 64); one wave a workgroup
__global__ __launch_bounds__(64) void zc_ser_write(const uint2* __restrict__ recs, uint64_t n, uint64_t groups,
                                                   const uint64_t* __restrict__ pos,
                                                   const uint8_t* __restrict__ stream, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  const uint32_t lane = threadIdx.x;
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {  // bound: groups
    const uint64_t first = g * zcser::kGroup;
    const uint32_t cnt = (uint32_t)min((uint64_t)zcser::kGroup, n - first);  // first < n
    const bool have = lane < cnt;
    zcser::Rec r{};
    uint64_t p = 0;
    if (have) {
      r = load_rec(recs, first + lane);
      p = pos[first + lane];
    }
    const bool big = have && zcser::is_big(r.kind, r.size);
    const bool raw = have && r.kind == zcser::kKindBytes;
    const uint32_t staged = have ? zcser::staged_len(r.kind, r.size) : 0;
    const uint64_t bigmask = __ballot(big);
    uint32_t lo = 0;
    for (uint32_t run = 0; run < zcser::kGroup && lo < cnt; run++) {  // bound: a group has at most 64 runs
      const uint32_t hi = zcser::run_last(bigmask, lo, cnt);
      // the run: the staged bytes of lanes [lo, hi], [a, a + len) of the output
      const uint64_t a = __shfl((unsigned long long)p, (int)lo, 64);
      const uint32_t len = (uint32_t)(__shfl((unsigned long long)(p + staged), (int)hi, 64) - a);  // <= kRunMax
      const uint32_t phase = (uint32_t)((uintptr_t)(out + a) & 15);  // of the address: any d_out gets aligned stores
      const bool mine = lane >= lo && lane <= hi;
      const uint32_t at = mine ? phase + (uint32_t)(p - a) : 0;  // this lane's place in LDS
      if (mine) {
        const uint32_t h = zcser::put_header(lds + at, r.kind, r.size);
        if (!raw) zcser::put_chunk_id(lds + at + h, r);
      }
      // the staged payloads, one after the other, the wave copying each: bound 64, then ceil(kStage / 64)
      const uint32_t pay_at = at + staged - r.size;  // of a staged BYTES record: its payload ends its message
      for (uint64_t m = __ballot(mine && raw && !big && r.size); m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        const uint64_t src = __shfl((unsigned long long)r.offset, j, 64);
        const uint32_t sz = __shfl(r.size, j, 64), dst = __shfl(pay_at, j, 64);
        for (uint32_t t = lane; t < sz; t += 64) lds[dst + t] = stream[src + t];
      }
      __syncthreads();
      // the flush: bytes up to the output's next slot, whole slots, the bytes that are left
      uint8_t* o = out + a;
      const uint32_t head = min(len, (16 - phase) & 15);
      if (lane < head) o[lane] = lds[phase + lane];
      const uint32_t nv = (len - head) >> 4, base = phase + head;  // base is 0 or 16 when nv > 0
      for (uint32_t v = lane; v < nv; v += 64)                     // bound: kLdsBytes / 16 / 64 rounds
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(lds + base + 16 * v),
                                    reinterpret_cast<u32x4*>(o + head + 16 * v));
      const uint32_t tail = (len - head) & 15;
      if (lane < tail) o[head + 16 * nv + lane] = lds[base + 16 * nv + lane];
      __syncthreads();  // lds is the next run's
      lo = hi + 1;
    }
  }
}

// pstart: the exclusive scan of the piece counts, pstart[n] = pieces
__global__ __launch_bounds__(kBlock) void zc_ser_copy(const uint2* __restrict__ recs, uint64_t n, uint64_t pieces,
                                                      const uint64_t* __restrict__ pos,
                                                      const uint64_t* __restrict__ pstart,
                                                      const uint8_t* __restrict__ stream, uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t q = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); q < pieces; q += waves) {
    // the record of piece q: pstart[lo] <= q < pstart[lo + 1]; bound: 32 halvings, n < 2^32
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (pstart[mid] <= q)
        lo = mid;
      else
        hi = mid;
    }
    const uint2 ofs = recs[5 * lo], sk = recs[5 * lo + 1];
    const uint64_t at = (q - pstart[lo]) * zcser::kPiece;
    if (!zcser::is_big(sk.y, sk.x) || at >= sk.x) continue;  // neither happens: the scan is of these records
    const uint64_t src = ((uint64_t)ofs.x | (uint64_t)ofs.y << 32) + at;
    zccopy::wave_copy(out + pos[lo] + zcser::header_len(sk.y, sk.x) + at, stream + src,
                      min(zcser::kPiece, (uint64_t)sk.x - at), lane);
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

int hip_error(std::string& err, hipError_t e, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  err = hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZC_ERR_NOMEM : ZC_ERR_HIP;
}
#define SCK(x)                                           \
  do {                                                   \
    hipError_t e_ = (x);                                 \
    if (e_ != hipSuccess) return hip_error(err, e_, st); \
  } while (0)

}  // namespace

struct SerScratch {
  Buf<uint2> recs;  // five a record
  Buf<uint64_t> len, pos, pstart, tsum;
  Buf<uint32_t> pc;
  Buf<unsigned long long> total;
  hipEvent_t ev[4] = {};
  int cus = 0;
  SerTimes times{};
  ~SerScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

SerScratch* ser_scratch_new() { return new SerScratch(); }
void ser_scratch_free(SerScratch* s) { delete s; }
const SerTimes* ser_times(const SerScratch* s) { return &s->times; }

int ser_measure(const zc_record* recs, size_t n, const uint64_t* stream_len, SerPlan* plan, std::string& err) {
  char msg[200];
  *plan = SerPlan{};
  if (n && !recs) {
    err = "null record array";
    return ZC_ERR_ARG;
  }
  for (size_t i = 0; i < n; i++) {
    const zc_record& r = recs[i];
    if (stream_len && r.kind == ZC_BYTES && (r.offset > *stream_len || r.size > *stream_len - r.offset)) {
      snprintf(msg, sizeof msg, "record %zu: bytes [%llu, +%u) past the end of a stream of %llu bytes", i,
               (unsigned long long)r.offset, r.size, (unsigned long long)*stream_len);
      err = msg;
      return ZC_ERR_ARG;
    }
    if (__builtin_add_overflow(plan->bytes, zcser::message_len(r.kind, r.size), &plan->bytes)) {
      snprintf(msg, sizeof msg, "record %zu: the stream's length passes 2^64", i);
      err = msg;
      return ZC_ERR_ARG;
    }
    const uint32_t pc = zcser::pieces(r.kind, r.size);
    plan->pieces += pc;  // below 2^16 a record
    plan->staged += pc ? 0 : 1;
  }
  return ZC_OK;
}

int ser_validate(const zc_record* recs, size_t n, const void* d_stream, uint64_t stream_len, const void* d_out,
                 uint64_t out_cap, uint64_t* n_out, SerPlan* plan, std::string& err) {
  char msg[200];
  *plan = SerPlan{};
  if (!n_out) {
    err = "null n_out";
    return ZC_ERR_ARG;
  }
  if (stream_len && !d_stream) {
    err = "null stream pointer";
    return ZC_ERR_ARG;
  }
  if (out_cap && !d_out) {
    err = "null output pointer";
    return ZC_ERR_ARG;
  }
  if (n >= kCountLimit) {
    snprintf(msg, sizeof msg, "%zu records: the count must stay below 2^32 - 1", n);
    err = msg;
    return ZC_ERR_ARG;
  }
  const int rc = ser_measure(recs, n, &stream_len, plan, err);
  if (rc != ZC_OK) return rc;
  *n_out = plan->bytes;  // written, or needed
  if (plan->bytes > out_cap) {
    snprintf(msg, sizeof msg, "the stream takes %llu bytes, the output has room for %llu",
             (unsigned long long)plan->bytes, (unsigned long long)out_cap);
    err = msg;
    return ZC_ERR_ARG;
  }
  return ZC_OK;
}

namespace {

// out[i] = the sum of src[0 .. i) for i < n, out[n] the sum
template <class T>
int scan(SerScratch* s, const T* src, uint64_t n, uint64_t* out, hipStream_t st, std::string& err) {
  const uint32_t ntiles = (uint32_t)((n + zcscan::kTile - 1) / zcscan::kTile);  // n < 2^32
  const int gt = (int)std::min<uint64_t>(ntiles, (uint64_t)s->cus * 16);
  zcscan::zc_scan_tile_sums<T><<<gt, kBlock, 0, st>>>(src, n, ntiles, s->tsum.p);
  zcscan::zc_scan_tile_scan<<<1, kBlock, 0, st>>>(s->tsum.p, ntiles, s->total.p);
  zcscan::zc_scan_write<T><<<gt, kBlock, 0, st>>>(src, n, ntiles, s->tsum.p, out, 1);
  SCK(hipGetLastError());
  return ZC_OK;
}

}  // namespace

int ser_write(SerScratch* s, int device, const zc_record* recs, size_t n, const void* d_stream, void* d_out,
              const SerPlan& plan, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  s->times = SerTimes{};
  s->times.staged_msgs = plan.staged;
  s->times.copy_pieces = plan.pieces;
  if (!n) return ZC_OK;  // nothing to write, no device work
  if (!s->cus) {
    int cus = 0;
    SCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    for (hipEvent_t& e : s->ev) SCK(hipEventCreate(&e));
    SCK(s->total.ensure(1));
    s->cus = std::max(cus, 1);
  }
  SCK(s->recs.ensure(5 * n));
  SCK(s->len.ensure(n));
  SCK(s->pc.ensure(n));
  SCK(s->pos.ensure(n + 1));
  if (plan.pieces) SCK(s->pstart.ensure(n + 1));
  SCK(s->tsum.ensure((n + zcscan::kTile - 1) / zcscan::kTile));
  // after the work queued on the legacy default stream so far
  SCK(hipEventRecord(ev_in, nullptr));
  SCK(hipStreamWaitEvent(st, ev_in, 0));
  SCK(hipEventRecord(s->ev[0], st));
  SCK(hipMemcpyAsync(s->recs.p, recs, sizeof(zc_record) * n, hipMemcpyHostToDevice, st));
  SCK(hipEventRecord(s->ev[1], st));
  const uint64_t groups = (n + zcser::kGroup - 1) / zcser::kGroup;
  const int lane_grid = (int)std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)s->cus * 16);
  zc_ser_sizes<<<lane_grid, kBlock, 0, st>>>(s->recs.p, n, s->len.p, s->pc.p);
  int rc = scan<uint64_t>(s, s->len.p, n, s->pos.p, st, err);
  if (rc == ZC_OK && plan.pieces) rc = scan<uint32_t>(s, s->pc.p, n, s->pstart.p, st, err);
  if (rc != ZC_OK) return rc;
  SCK(hipEventRecord(s->ev[2], st));
  // a wave a workgroup, 8.6 KiB of LDS each: up to 16 on a CU
  zc_ser_write<<<(int)std::min<uint64_t>(groups, (uint64_t)s->cus * 16), 64, 0, st>>>(
      s->recs.p, n, groups, s->pos.p, (const uint8_t*)d_stream, (uint8_t*)d_out);
  if (plan.pieces)
    zc_ser_copy<<<(int)std::min<uint64_t>((plan.pieces + kBlock / 64 - 1) / (kBlock / 64), (uint64_t)s->cus * 16),
                  kBlock, 0, st>>>(s->recs.p, n, plan.pieces, s->pos.p, s->pstart.p, (const uint8_t*)d_stream,
                                   (uint8_t*)d_out);
  SCK(hipGetLastError());
  SCK(hipEventRecord(s->ev[3], st));
  SCK(hipStreamSynchronize(st));
  float ms[3] = {};
  for (int k = 0; k < 3; k++) SCK(hipEventElapsedTime(&ms[k], s->ev[k], s->ev[k + 1]));
  s->times.upload_ms = ms[0];
  s->times.size_ms = ms[1];
  s->times.write_ms = ms[2];
  return ZC_OK;
}

}  // namespace zc
