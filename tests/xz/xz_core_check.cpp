// Host check of zc_xz_core.h (test infrastructure only; built by
// tests/test_xz.py under ASan + UBSan).  Without arguments: the CRC constants
// and the combine rule.  With a case file the Python test wrote from liblzma's
// answers: every stream through the core, with a sink that aborts on any write
// outside [0, cap), any write that is not at the write position and any read
// at or past it -- the rule the device sink relies on.
//
// case file: u32 count, then per case
//   i32 lzma_ret (-1: not compared)   i32 want_status (-1: any)
//   u64 cap   u64 in_pos   u32 stream bytes, the stream   u32 expected bytes, the bytes
// output: one line per case "<status> <decoded> <consumed> <wide>", then "ok <count>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zc_xz_core.h"

namespace {

[[noreturn]] void die(const char* what, size_t i) {
  fprintf(stderr, "case %zu: %s\n", i, what);
  abort();
}

struct In {
  const uint8_t* p;
  uint64_t n;
  uint32_t byte(uint64_t i) const {
    if (i >= n) {
      fprintf(stderr, "read of input byte %llu of %llu\n", (unsigned long long)i, (unsigned long long)n);
      abort();
    }
    return p[i];
  }
};

struct Probs {
  std::vector<uint16_t> v;
  uint32_t filled = 0;
  uint32_t cap() const { return (uint32_t)v.size(); }
  uint32_t ld(uint32_t i) const {
    if (i >= filled) abort();  // a probability never set
    return v[i];
  }
  void st(uint32_t i, uint32_t x) {
    if (i >= filled || x == 0 || x >= 2048) abort();
    v[i] = (uint16_t)x;
  }
  void fill(uint32_t n) {
    if (n > v.size()) abort();
    for (uint32_t i = 0; i < n; ++i) v[i] = 1024;
    filled = n;
  }
};

struct Out {
  uint8_t* buf;  // exactly cap bytes: the sanitizer sees what the checks below miss
  uint64_t cap, wp;
  const In* in;
  void lit(uint64_t pos, uint32_t b) {
    if (pos != wp || pos >= cap || b > 255) abort();
    buf[pos] = (uint8_t)b;
    wp = pos + 1;
  }
  uint32_t get(uint64_t pos) const {
    if (pos >= wp) abort();
    return buf[pos];
  }
  void copy(uint64_t pos, uint32_t dist, uint32_t len) {
    if (pos != wp || dist < 1 || dist > pos || len < 1 || len > zcxz::kMatchLenMax || len > cap - pos) abort();
    // as the device copies: 64 lanes a step, lane k from the period
    for (uint32_t k0 = 0; k0 < len; k0 += 64) {
      uint8_t lane[64];
      const uint32_t m = len - k0 < 64 ? len - k0 : 64;
      for (uint32_t l = 0; l < m; ++l) lane[l] = buf[pos - dist + (k0 + l) % dist];
      for (uint32_t l = 0; l < m; ++l) buf[pos + k0 + l] = lane[l];
    }
    wp = pos + len;
  }
  void stored(uint64_t src, uint64_t pos, uint32_t len) {
    if (pos != wp || len < 1 || len > cap - pos || src > in->n || len > in->n - src) abort();
    memcpy(buf + pos, in->p + src, len);
    wp = pos + len;
  }
};

struct Payload {
  const uint8_t* p;
  uint32_t byte(uint64_t i) const { return p[i]; }
};

void self_checks() {
  const char* d = "123456789";
  In in{(const uint8_t*)d, 9};
  if (zcxz::crc32_of(in, 0, 9) != 0xCBF43926u) die("crc32 of 123456789", 0);
  if (zcxz::crc64_of(in, 0, 9) != 0x995DC9BBDF1939FAull) die("crc64 of 123456789", 0);
  std::vector<uint8_t> v(5000);
  uint32_t s = 12345;
  for (auto& b : v) {
    s = s * 1664525u + 1013904223u;
    b = (uint8_t)(s >> 24);
  }
  In all{v.data(), v.size()};
  const uint64_t cuts[] = {0, 1, 63, 64, 1000, 4999, 5000};
  for (uint64_t c : cuts) {
    const uint64_t nb = v.size() - c;
    if (zcxz::crc32_combine(zcxz::crc32_of(all, 0, c), zcxz::crc32_of(all, c, nb), nb) !=
        zcxz::crc32_of(all, 0, v.size()))
      die("crc32 combine", (size_t)c);
    if (zcxz::crc64_combine(zcxz::crc64_of(all, 0, c), zcxz::crc64_of(all, c, nb), nb) !=
        zcxz::crc64_of(all, 0, v.size()))
      die("crc64 combine", (size_t)c);
  }
  // the device's form: 64 raw slices, front-padded with zeros, one operator
  for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 4999ull}) {
    const uint64_t slice = ((n + 63) / 64 + 15) & ~15ull, pad = slice * 64 - n;  // as zc_xz_check_kernel cuts
    const uint64_t X = zcxz::gf_x8n<uint64_t>(slice, zcxz::kPoly64);
    const uint32_t X32 = zcxz::gf_x8n<uint32_t>(slice, zcxz::kPoly32);
    uint64_t acc = 0;
    uint32_t acc32 = 0;
    for (uint64_t k = 0; k < 64; ++k) {
      uint64_t raw = 0;
      uint32_t raw32 = 0;
      for (uint64_t j = k * slice; j < (k + 1) * slice; ++j)
        if (j >= pad) {
          raw = zcxz::crc64_byte(raw, v[j - pad]);
          raw32 = zcxz::crc32_byte(raw32, v[j - pad]);
        }
      acc = zcxz::gf_mul(acc, X, zcxz::kPoly64) ^ raw;
      acc32 = zcxz::gf_mul(acc32, X32, zcxz::kPoly32) ^ raw32;
    }
    if (zcxz::crc64_finish_raw(acc, n) != zcxz::crc64_of(all, 0, n)) die("crc64 from 64 slices", (size_t)n);
    if (zcxz::crc32_finish_raw(acc32, n) != zcxz::crc32_of(all, 0, n)) die("crc32 from 64 slices", (size_t)n);
  }
}

template <class T>
T rd(FILE* f) {
  T v;
  if (fread(&v, sizeof v, 1, f) != 1) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  self_checks();
  if (argc < 2) {
    printf("ok 0\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t count = rd<uint32_t>(f);
  for (uint32_t i = 0; i < count; ++i) {
    const int32_t lzma_ret = rd<int32_t>(f), want = rd<int32_t>(f);
    const uint64_t cap = rd<uint64_t>(f), in_pos = rd<uint64_t>(f);
    const uint32_t sn = rd<uint32_t>(f);
    // exactly sn bytes on the heap: a read past the stream is the sanitizer's
    uint8_t* stream = (uint8_t*)malloc(sn ? sn : 1);
    if (sn && fread(stream, 1, sn, f) != sn) return 2;
    const uint32_t en = rd<uint32_t>(f);
    std::vector<uint8_t> expect(en);
    if (en && fread(expect.data(), 1, en, f) != en) return 2;

    In in{stream, sn};
    uint8_t* buf = (uint8_t*)malloc(cap ? cap : 1);
    zcxz::Result r{};
    int wide = 0;
    for (int form = 0; form < 2; ++form) {  // the common form, then the wide one if asked for
      Probs probs;
      probs.v.assign(form ? zcxz::kProbsWide : zcxz::kProbsCommon, 0);
      Out out{buf, cap, 0, &in};
      r = zcxz::decode(in, (uint64_t)sn, cap, probs, out);
      if (r.decoded != out.wp) die("decoded differs from the sink's write position", i);
      if (r.status != zcxz::kNeedWide) break;
      if (form) die("the wide form asks for more", i);
      wide = 1;
    }
    if (r.status == zcxz::kOk && r.check_id != zcxz::kCheckNone && r.decoded > 0) {
      Payload p{buf};
      if (zcxz::check_of(p, r.decoded, r.check_id) != r.stored) r.status = zcxz::kCheck;
    }
    if (r.status == zcxz::kBudget) die("the trip count ran out", i);
    if (r.decoded > cap) die("decoded more than cap", i);
    if (lzma_ret == 0) {
      if (r.status != zcxz::kOk && want < 0) die("liblzma accepts, the core does not", i);
      if (r.status == zcxz::kOk) {
        if (r.decoded != en || (en && memcmp(buf, expect.data(), en) != 0)) die("bytes differ from liblzma's", i);
        if (r.consumed != in_pos) die("consumed differs from liblzma's in_pos", i);
      }
    } else if (lzma_ret > 0) {
      if (r.status == zcxz::kOk) die("liblzma refuses, the core accepts", i);
    }
    if (want >= 0 && r.status != want) {
      fprintf(stderr, "case %u: status %d, want %d\n", i, r.status, want);
      abort();
    }
    printf("%d %llu %llu %d\n", r.status, (unsigned long long)r.decoded, (unsigned long long)r.consumed, wide);
    free(buf);
    free(stream);
  }
  fclose(f);
  printf("ok %u\n", count);
  return 0;
}
