// zc_range.hip -- random-access restore: any byte range of a backup, served on
// the GPU from resident decoded bundle payloads.
//
// What zbackup runs: BackupRestorer::IndexedRestorer (backup_restorer.cc:182-316),
// which `zbackup nbd` serves a backup through (zutils.cc:262-297): the
// constructor's running sum over the instructions, then per saveData an
// upper_bound, one step back, and a walk that copies each instruction's overlap
// with the range.
//
// Work split (zc_range_core.h holds the search and the clip, for host and
// device):
//   host    the running sum and the bounds of every entry, once, at creation;
//           per call the range check and, while any slot is absent, the
//           residency check (the same walk over the touched entries, nothing
//           copied); then each read cut into pieces of at most 64 KiB
//           (zclzo::kPiece, the scatter's piece): O(bytes / 64 KiB), whatever
//           the entry count;
//   zc_range_read_kernel  one wave per piece: the search, the walk, and per
//           overlapping entry the copy body of zc_lzo_copy_kernel
//           (zc_copy_body.h) from base[slot] + off + start.
// A slot is one decoded bundle payload (or the instruction stream, whose
// bytes_to_emit runs are read in place); its device pointer may change between
// calls, so only the payloads a batch touches need to be in HBM.
//
// The kernel waits on nothing: no barrier, no spin, no cross-lane operation.
// Its loops are the 64-step search and a walk whose trip count is fixed before
// it starts; every source range is checked against its slot's size again
// before it is copied.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#define ZC_HD __host__ __device__
#include "zc_copy_body.h"
#include "zc_device.h"
#include "zc_lzo_core.h"
#include "zc_range_core.h"

namespace zc {
namespace {

struct Piece {
  uint64_t start;  // stream position of the piece's first byte
  uint8_t* dst;    // where that byte goes
  uint32_t size;   // 1 .. kPiece
  uint32_t read;   // the read it belongs to
};

// hands each overlap to the wave's copy body
struct WaveSink {
  const uint8_t* const* base;
  uint8_t* dst;
  uint32_t lane;
  __device__ bool operator()(uint32_t slot, uint64_t src_off, uint64_t at, uint64_t len) const {
    const uint8_t* b = base[slot];
    if (!b) return false;
    zccopy::wave_copy(dst + at, b + src_off, len, lane);
    return true;
  }
};

// one wave per piece; status[0]: the zcrange status bits any piece raised,
// status[1]: the smallest read index with one
__global__ __launch_bounds__(256) void zc_range_read_kernel(zcrange::Index ix, const uint8_t* const* __restrict__ base,
                                                            const Piece* __restrict__ pieces, uint32_t n,
                                                            uint32_t* __restrict__ status) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (w >= n) return;
  const Piece p = pieces[w];
  WaveSink sink{base, p.dst, lane};
  const uint32_t bits = zcrange::serve_piece(ix, p.start, p.size, sink);
  if (bits && lane == 0) {
    atomicOr(&status[0], bits);
    atomicMin(&status[1], p.read);
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
    cap = n;
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
  if (st) (void)hipStreamSynchronize(st);
  err = hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZC_ERR_NOMEM : ZC_ERR_HIP;
}
#define RCK(x)                                            \
  do {                                                    \
    hipError_t e_ = (x);                                  \
    if (e_ != hipSuccess) return hip_error(err, e_, st);  \
  } while (0)

struct SetDevice {
  int prev = -1;
  explicit SetDevice(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~SetDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// pieces per launch: the list's host memory is reused from one to the next
constexpr size_t kMaxPieces = 1u << 20;

}  // namespace
}  // namespace zc

// The index: host copies of everything (the checks read them), device copies
// of the arrays made once, and per slot the payload's device pointer.
struct zc_range_index {
  std::mutex mu;
  std::vector<uint64_t> pos, off, slot_size;
  std::vector<uint32_t> slot;
  std::vector<const uint8_t*> base;  // per slot: the resident payload, or null
  std::vector<uint8_t*> owned;       // per slot: the index's own copy (zc_range_slot_upload), or null
  int device = -1;                   // -1: made without a context, host only so far
  bool base_dirty = true;
  uint64_t *d_pos = nullptr, *d_off = nullptr, *d_slot_size = nullptr;
  uint32_t* d_slot = nullptr;
  const uint8_t** d_base = nullptr;

  uint64_t n() const { return off.size(); }
  uint64_t total() const { return pos.back(); }
  zcrange::Index host_view() const {
    return zcrange::Index{pos.data(), slot.data(), off.data(), n(), slot_size.data(), (uint32_t)slot_size.size()};
  }
  zcrange::Index device_view() const {
    return zcrange::Index{d_pos, d_slot, d_off, n(), d_slot_size, (uint32_t)slot_size.size()};
  }
};

namespace zc {

struct RangeScratch {
  Buf<Piece> pieces;
  Buf<uint32_t> status;
  Buf<uint8_t> stage;  // zc_range_read_host: the reads back to back
  uint8_t* pinned = nullptr;
  size_t pinned_cap = 0;
  hipEvent_t ev[3] = {};
  RangeTimes times{};
  ~RangeScratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (pinned) (void)hipHostFree(pinned);
  }
};

RangeScratch* range_scratch_new() { return new RangeScratch(); }
void range_scratch_free(RangeScratch* s) { delete s; }
const RangeTimes* range_times(const RangeScratch* s) { return &s->times; }

int range_index_create(const uint64_t* slot_sizes, size_t n_slots, const uint32_t* slot, const uint64_t* off,
                       const uint64_t* sizes, size_t n, zc_range_index** out, std::string& err) {
  if (!out) return arg_error(err, "null index pointer");
  *out = nullptr;
  if ((n_slots && !slot_sizes) || (n && (!slot || !off || !sizes)))
    return arg_error(err, "null slot_sizes, slot, off or sizes with a count > 0");
  if (n_slots >= 0xFFFFFFFFull) return arg_error(err, "the slot count must stay below 2^32 - 1");
  std::unique_ptr<zc_range_index> ix(new zc_range_index());  // no device memory yet: plain delete
  ix->slot_size.assign(slot_sizes, slot_sizes + n_slots);
  ix->base.assign(n_slots, nullptr);
  ix->owned.assign(n_slots, nullptr);
  ix->pos.resize(n + 1);
  ix->slot.assign(slot, slot + n);
  ix->off.assign(off, off + n);
  // the exclusive running sum, with every entry's bounds checked on the way
  uint64_t sum = 0;
  for (size_t e = 0; e < n; ++e) {
    ix->pos[e] = sum;
    std::string bad;
    if (slot[e] >= n_slots)
      bad = "names slot " + std::to_string(slot[e]) + " of " + std::to_string(n_slots);
    else if (off[e] > slot_sizes[slot[e]] || sizes[e] > slot_sizes[slot[e]] - off[e])
      bad = "[" + std::to_string(off[e]) + ", +" + std::to_string(sizes[e]) + ") ends past slot " +
            std::to_string(slot[e]) + "'s " + std::to_string(slot_sizes[slot[e]]) + " bytes";
    else if (sum + sizes[e] < sum)
      bad = "takes the stream's length past 2^64";
    if (!bad.empty()) return arg_error(err, "entry " + std::to_string(e) + " " + bad);
    sum += sizes[e];
  }
  ix->pos[n] = sum;
  *out = ix.release();
  return ZC_OK;
}

std::mutex& range_mutex(zc_range_index* ix) { return ix->mu; }

// the device copies of the arrays, made once, on the first call that brings a
// context (range_mutex held).  All or nothing: a failure frees what it made and
// leaves the index host only, so the next call tries again.
static void free_device_arrays(zc_range_index* ix) {
  for (void* p : {(void*)ix->d_pos, (void*)ix->d_off, (void*)ix->d_slot, (void*)ix->d_slot_size, (void*)ix->d_base})
    if (p) (void)hipFree(p);
  ix->d_pos = ix->d_off = ix->d_slot_size = nullptr;
  ix->d_slot = nullptr;
  ix->d_base = nullptr;
}

int range_index_attach(zc_range_index* ix, int device, hipStream_t st, std::string& err) {
  if (ix->device >= 0) {
    if (ix->device == device) return ZC_OK;
    return arg_error(err, "the index lives on device " + std::to_string(ix->device) + ", the context on device " +
                              std::to_string(device));
  }
  const size_t n = ix->n(), ns = ix->slot_size.size();
  auto upload = [&]() -> hipError_t {
#define ACK(x)                        \
  do {                                \
    hipError_t e_ = (x);              \
    if (e_ != hipSuccess) return e_;  \
  } while (0)
    ACK(hipMalloc(&ix->d_pos, (n + 1) * sizeof(uint64_t)));
    ACK(hipMalloc(&ix->d_off, std::max<size_t>(n, 1) * sizeof(uint64_t)));
    ACK(hipMalloc(&ix->d_slot, std::max<size_t>(n, 1) * sizeof(uint32_t)));
    ACK(hipMalloc(&ix->d_slot_size, std::max<size_t>(ns, 1) * sizeof(uint64_t)));
    ACK(hipMalloc(&ix->d_base, std::max<size_t>(ns, 1) * sizeof(uint8_t*)));
    ACK(hipMemcpyAsync(ix->d_pos, ix->pos.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (n) {
      ACK(hipMemcpyAsync(ix->d_off, ix->off.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      ACK(hipMemcpyAsync(ix->d_slot, ix->slot.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (ns)
      ACK(hipMemcpyAsync(ix->d_slot_size, ix->slot_size.data(), ns * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    return hipStreamSynchronize(st);
#undef ACK
  };
  const hipError_t e = upload();
  if (e != hipSuccess) {
    const int rc = hip_error(err, e, st);  // waits for the stream first
    free_device_arrays(ix);
    return rc;
  }
  ix->device = device;
  ix->base_dirty = true;
  return ZC_OK;
}

void range_index_destroy(zc_range_index* ix) {
  if (!ix) return;
  if (ix->device >= 0) {
    SetDevice g(ix->device);
    for (uint8_t* p : ix->owned)
      if (p) (void)hipFree(p);
    free_device_arrays(ix);
  }
  delete ix;
}

uint64_t range_index_total(const zc_range_index* ix) { return ix->total(); }

static int slot_check(const zc_range_index* ix, uint32_t slot, std::string& err) {
  if (slot >= ix->slot_size.size())
    return arg_error(err, "slot " + std::to_string(slot) + " of " + std::to_string(ix->slot_size.size()));
  return ZC_OK;
}

// drops the index's own copy of a slot, if it has one (ix->mu held)
static void release_owned(zc_range_index* ix, uint32_t slot) {
  if (!ix->owned[slot]) return;
  SetDevice g(ix->device);
  (void)hipFree(ix->owned[slot]);
  ix->owned[slot] = nullptr;
}

int range_set_slot(zc_range_index* ix, uint32_t slot, const void* d_ptr, std::string& err) {
  std::lock_guard<std::mutex> lk(ix->mu);
  if (int rc = slot_check(ix, slot, err)) return rc;
  release_owned(ix, slot);
  ix->base[slot] = (const uint8_t*)d_ptr;
  ix->base_dirty = true;
  return ZC_OK;
}

int range_slot_upload(zc_range_index* ix, uint32_t slot, const void* host, uint64_t size, std::string& err) {
  std::lock_guard<std::mutex> lk(ix->mu);
  if (int rc = slot_check(ix, slot, err)) return rc;
  if (size != ix->slot_size[slot])
    return arg_error(err, "slot " + std::to_string(slot) + " holds " + std::to_string(ix->slot_size[slot]) +
                              " bytes, " + std::to_string(size) + " given");
  if (size && !host) return arg_error(err, "null payload");
  if (ix->device < 0) return arg_error(err, "the index was made without a context: it has no device to upload to");
  SetDevice g(ix->device);
  hipStream_t st = nullptr;
  uint8_t* p = nullptr;
  RCK(hipMalloc(&p, std::max<uint64_t>(size, 1)));
  hipError_t e = size ? hipMemcpy(p, host, size, hipMemcpyHostToDevice) : hipSuccess;
  if (e != hipSuccess) {
    (void)hipFree(p);
    return hip_error(err, e, st);
  }
  release_owned(ix, slot);
  ix->owned[slot] = p;
  ix->base[slot] = p;
  ix->base_dirty = true;
  return ZC_OK;
}

int range_slot_drop(zc_range_index* ix, uint32_t slot, std::string& err) {
  return range_set_slot(ix, slot, nullptr, err);
}

// offset[i] + size[i] <= total for every read (the reference's exOutOfRange;
// 0 bytes at offset == total is a read like any other)
static int reads_in_range(const zc_range_index* ix, const uint64_t* offset, const uint64_t* size, size_t n_reads,
                          std::string& err) {
  const uint64_t total = ix->total();
  for (size_t i = 0; i < n_reads; ++i)
    if (offset[i] > total || size[i] > total - offset[i])
      return arg_error(err, "read " + std::to_string(i) + " [" + std::to_string(offset[i]) + ", +" +
                                std::to_string(size[i]) + ") is out of range: the stream has " +
                                std::to_string(total) + " bytes");
  return ZC_OK;
}

int range_needs(const zc_range_index* ix, const uint64_t* offset, const uint64_t* size, size_t n_reads,
                uint32_t* slots_out, size_t cap, size_t* n_out, std::string& err) {
  if (!n_out || (n_reads && (!offset || !size)) || (cap && !slots_out))
    return arg_error(err, "null offset, size, slots_out or n_out");
  if (int rc = reads_in_range(ix, offset, size, n_reads, err)) return rc;
  std::vector<uint8_t> seen(ix->slot_size.size(), 0);
  const zcrange::Index v = ix->host_view();
  for (size_t i = 0; i < n_reads; ++i) zcrange::mark_slots(v, offset[i], size[i], seen.data());
  size_t k = 0;
  for (size_t s = 0; s < seen.size(); ++s)
    if (seen[s]) {
      if (k < cap) slots_out[k] = (uint32_t)s;
      ++k;
    }
  *n_out = k;
  if (k > cap)
    return arg_error(err, "the batch touches " + std::to_string(k) + " slots, room for " + std::to_string(cap));
  return ZC_OK;
}

int range_validate_read(zc_range_index* ix, const uint64_t* offset, const uint64_t* size, size_t n_reads,
                        const void* dst, const uint64_t* dst_off, std::string& err) {
  if (!n_reads) return ZC_OK;
  if (!offset || !size || !dst_off) return arg_error(err, "null offset, size or dst_off with reads > 0");
  if (int rc = reads_in_range(ix, offset, size, n_reads, err)) return rc;
  bool any = false;
  for (size_t i = 0; i < n_reads; ++i) any = any || size[i];
  if (any && !dst) return arg_error(err, "null destination");
  // with every slot resident there is nothing to find: the walk over the
  // touched entries is only made when a slot is absent
  if (std::find(ix->base.begin(), ix->base.end(), nullptr) == ix->base.end()) return ZC_OK;
  std::vector<uint8_t> seen(ix->slot_size.size(), 0);
  const zcrange::Index v = ix->host_view();
  for (size_t i = 0; i < n_reads; ++i) zcrange::mark_slots(v, offset[i], size[i], seen.data());
  for (size_t s = 0; s < seen.size(); ++s)
    if (seen[s] && !ix->base[s])
      return arg_error(err, "slot " + std::to_string(s) + " is not resident (zc_range_set_slot or "
                                "zc_range_slot_upload it; zc_range_needs lists the slots a batch touches)");
  return ZC_OK;
}

static std::string status_text(const uint32_t st[2]) {
  std::string s = "the device walk of read " + std::to_string(st[1]) + " found";
  if (st[0] & zcrange::kBadSlot) s += " an entry naming no slot";
  if (st[0] & zcrange::kNoPayload) s += " a slot without a payload";
  if (st[0] & zcrange::kBadRange) s += " an entry ending past its slot";
  return s + " (internal error: the host checks passed under the same lock)";
}

int range_read(RangeScratch* s, zc_range_index* ix, const uint64_t* offset, const uint64_t* size, size_t n_reads,
               void* dst, const uint64_t* dst_off, bool host, hipEvent_t ev_in, hipStream_t st, std::string& err) {
  s->times = RangeTimes{};
  if (!s->ev[0])
    for (hipEvent_t& e : s->ev) RCK(hipEventCreate(&e));
  constexpr uint64_t kPiece = zclzo::kPiece;
  uint8_t* d_dst = (uint8_t*)dst;
  const uint64_t* const user_off = dst_off;
  std::vector<uint64_t> packed;  // host: where each read lies in the staging buffer
  uint64_t bytes = 0;
  if (host) {
    packed.resize(n_reads);
    for (size_t i = 0; i < n_reads; ++i) {
      packed[i] = bytes;
      if (bytes + size[i] < bytes) return arg_error(err, "the reads' sizes sum past 2^64");
      bytes += size[i];
    }
    if (!bytes) return ZC_OK;
    RCK(s->stage.ensure(bytes));
    if (s->pinned_cap < bytes) {
      if (s->pinned) (void)hipHostFree(s->pinned);
      s->pinned = nullptr;
      s->pinned_cap = 0;
      RCK(hipHostMalloc(&s->pinned, bytes, hipHostMallocDefault));
      s->pinned_cap = bytes;
    }
    d_dst = s->stage.p;
    dst_off = packed.data();
  }
  if (ev_in) {
    // after the caller's default-stream work: the slots are device memory in
    // both forms, and the caller may have just filled them there
    RCK(hipEventRecord(ev_in, nullptr));
    RCK(hipStreamWaitEvent(st, ev_in, 0));
  }
  RCK(s->status.ensure(2));
  static const uint32_t clean[2] = {0u, 0xFFFFFFFFu};  // outlives the asynchronous copy
  RCK(hipMemcpyAsync(s->status.p, clean, sizeof clean, hipMemcpyHostToDevice, st));
  if (ix->base_dirty) {
    if (!ix->base.empty())
      RCK(hipMemcpyAsync(ix->d_base, ix->base.data(), ix->base.size() * sizeof(uint8_t*), hipMemcpyHostToDevice, st));
    RCK(hipStreamSynchronize(st));  // ix->base may change once the caller lets go of the lock
    ix->base_dirty = false;
  }
  std::vector<Piece> list;
  size_t i = 0;
  uint64_t k = 0;  // the next piece of read i starts k bytes into it
  while (i < n_reads) {
    list.clear();
    while (i < n_reads && list.size() < kMaxPieces) {
      if (k >= size[i]) {
        ++i;
        k = 0;
        continue;
      }
      const uint32_t len = (uint32_t)std::min<uint64_t>(kPiece, size[i] - k);
      list.push_back(Piece{offset[i] + k, d_dst + dst_off[i] + k, len, (uint32_t)std::min<size_t>(i, 0xFFFFFFFEu)});
      k += len;
    }
    if (list.empty()) break;
    const uint32_t np = (uint32_t)list.size();
    RCK(s->pieces.ensure(np));
    RCK(hipEventRecord(s->ev[0], st));
    RCK(hipMemcpyAsync(s->pieces.p, list.data(), np * sizeof(Piece), hipMemcpyHostToDevice, st));
    RCK(hipEventRecord(s->ev[1], st));
    hipLaunchKernelGGL(zc_range_read_kernel, dim3((np + 3) / 4), dim3(256), 0, st, ix->device_view(),
                       (const uint8_t* const*)ix->d_base, s->pieces.p, np, s->status.p);
    RCK(hipGetLastError());
    RCK(hipEventRecord(s->ev[2], st));
    uint32_t status[2] = {0, 0};
    RCK(hipMemcpyAsync(status, s->status.p, sizeof status, hipMemcpyDeviceToHost, st));
    RCK(hipStreamSynchronize(st));  // the list's host memory is reused
    float ms = 0;
    RCK(hipEventElapsedTime(&ms, s->ev[1], s->ev[2]));
    s->times.kernel_ms += ms;
    RCK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->times.upload_ms += ms;
    s->times.pieces += np;
    if (status[0]) {
      err = status_text(status);
      return ZC_ERR_STATE;
    }
  }
  if (host) {
    RCK(hipMemcpyAsync(s->pinned, s->stage.p, bytes, hipMemcpyDeviceToHost, st));
    RCK(hipStreamSynchronize(st));
    for (size_t r = 0; r < n_reads; ++r)
      if (size[r]) memcpy((uint8_t*)dst + user_off[r], s->pinned + packed[r], size[r]);
  }
  return ZC_OK;
}

}  // namespace zc
