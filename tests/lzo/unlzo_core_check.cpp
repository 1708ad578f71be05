// Test infrastructure: checks zc_lzo_dec.h (the LZO1X token walker and the
// framing rules the GPU bundle decompressor runs) against liblzo2's own
// lzo1x_decompress_safe, compiled for the host (with ASan + UBSan when
// tests/test_unlzo.py can link them).  The cases come from a file the test
// writes (tests/unlzo_inputs.py makes them): per case
//   int32 expect (kAny: whatever the library says), uint64 out_cap,
//   uint32 frame bytes, the framed bundle.
// The walker runs with a sink that ABORTS on any op outside the validity rule
// (src_off + len <= csize, dst_off + len <= cap, 1 <= dist <= dst_off) and a
// reader that aborts on a control-byte read at or past csize; the copies go
// to a buffer of exactly cap bytes, so the sanitizer sees any other overrun.
// Status, length and bytes must equal the library's under the reference's
// framing (compression.cc:369-402,472-490).  Prints "codes" (how many walks
// ended with each library code), "frame" (how many bundles ended with each
// frame code) and "ok N", or the first mismatch.
#include <lzo/lzo1x.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "zc_lzo_dec.h"

using namespace zclzo;

static const int32_t kAny = 1000;

struct HostIn {
  const uint8_t* p;
  uint32_t csize;
  uint64_t reads = 0;
  uint32_t byte(uint32_t i) {
    if (i >= csize) {
      fprintf(stderr, "control byte %u read past csize %u\n", i, csize);
      abort();
    }
    reads++;
    return p[i];
  }
};

struct HostSink {
  const uint8_t* in;
  uint32_t csize;
  uint8_t* out;
  uint32_t cap;
  uint32_t end = 0;  // ops must tile the output in order
  void literal(uint32_t src, uint32_t dst, uint32_t len) {
    if (!len || (uint64_t)src + len > csize || (uint64_t)dst + len > cap || dst != end) {
      fprintf(stderr, "literal(%u, %u, %u) outside csize %u / cap %u / end %u\n", src, dst, len, csize, cap, end);
      abort();
    }
    memcpy(out + dst, in + src, len);
    end = dst + len;
  }
  void match(uint32_t dst, uint32_t dist, uint32_t len) {
    if (!len || !dist || dist > dst || (uint64_t)dst + len > cap || dst != end || dist > kMaxDistance) {
      fprintf(stderr, "match(%u, %u, %u) outside cap %u / end %u\n", dst, dist, len, cap, end);
      abort();
    }
    // the form the device sink uses: every source below dst
    for (uint32_t k = 0; k < len; k++) out[dst + k] = out[dst - dist + (k % dist)];
    end = dst + len;
  }
};

struct Result {
  int status;
  int walk_rc;  // the decoder's own code (kAny: the frame was refused before it)
  std::vector<uint8_t> bytes;
};

static Result core_decode(const uint8_t* f, uint64_t avail, uint64_t out_cap) {
  Result r{0, kAny, {}};
  uint32_t n, csize;
  r.status = frame_read(f, avail, &n, &csize);
  if (r.status) return r;
  const uint32_t cap = frame_cap(n, out_cap);
  // exactly csize and cap bytes, so the sanitizer bounds both
  std::vector<uint8_t> in(f + kDecFrame, f + kDecFrame + csize), out(cap);
  HostIn hin{in.data(), csize};
  HostSink sink{in.data(), csize, out.data(), cap};
  uint32_t produced = 0;
  r.walk_rc = walk(hin, csize, cap, sink, &produced);
  if (produced != sink.end || hin.reads > 4ull * csize + 4) {
    fprintf(stderr, "produced %u, ops end at %u; %llu reads of %u bytes\n", produced, sink.end,
            (unsigned long long)hin.reads, csize);
    abort();
  }
  r.status = frame_status(r.walk_rc, produced, n);
  out.resize(produced);
  r.bytes.swap(out);
  return r;
}

static Result lib_decode(const uint8_t* f, uint64_t avail, uint64_t out_cap) {
  Result r{0, kAny, {}};
  if (avail < 16) return Result{kFrameBad, kAny, {}};
  uint32_t n, csize;
  memcpy(&n, f, 4);
  memcpy(&csize, f + 8, 4);
  if (16ull + csize > avail) return Result{kFrameBad, kAny, {}};
  const uint32_t cap = out_cap < n ? (uint32_t)out_cap : n;
  std::vector<uint8_t> in(f + 16, f + 16 + csize), out(cap);
  lzo_uint olen = cap;
  r.walk_rc = lzo1x_decompress_safe(in.data(), csize, out.data(), &olen, nullptr);
  r.status = r.walk_rc != LZO_E_OK ? r.walk_rc : olen == n ? 0 : kFrameSize;
  out.resize(olen);
  r.bytes.swap(out);
  return r;
}

int main(int argc, char** argv) {
  if (argc < 2 || lzo_init() != LZO_E_OK) return 3;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) return 3;
  std::map<int, int> codes, frames;
  int n_ok = 0;
  for (int c = 0;; c++) {
    int32_t expect;
    uint64_t out_cap;
    uint32_t flen;
    if (fread(&expect, 4, 1, fp) != 1) break;
    if (fread(&out_cap, 8, 1, fp) != 1 || fread(&flen, 4, 1, fp) != 1) return 3;
    std::vector<uint8_t> f(flen);
    if (flen && fread(f.data(), 1, flen, fp) != flen) return 3;
    const Result a = lib_decode(f.data(), flen, out_cap), b = core_decode(f.data(), flen, out_cap);
    if (a.walk_rc != kAny) codes[a.walk_rc]++;
    frames[a.status]++;
    if (a.status != b.status || a.walk_rc != b.walk_rc || (expect != kAny && a.status != expect)) {
      printf("MISMATCH case %d: library status %d (rc %d), core %d (rc %d), expected %d\n", c, a.status, a.walk_rc,
             b.status, b.walk_rc, expect);
      return 1;
    }
    // the bytes produced before an error are the library's too (both stop at the failing token)
    if (a.walk_rc == LZO_E_OK && a.bytes != b.bytes) {
      printf("MISMATCH case %d: %zu bytes from the library, %zu from the core, or other bytes\n", c, a.bytes.size(),
             b.bytes.size());
      return 1;
    }
    n_ok++;
  }
  fclose(fp);
  printf("codes");
  for (auto& kv : codes) printf(" %d:%d", kv.first, kv.second);
  printf("\nframe");
  for (auto& kv : frames) printf(" %d:%d", kv.first, kv.second);
  printf("\nok %d\n", n_ok);
  return 0;
}
