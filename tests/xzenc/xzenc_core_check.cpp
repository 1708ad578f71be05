// Host check of zc_xzenc_core.h (test infrastructure only; built by
// tests/test_xzenc.py under ASan + UBSan).  Every case of the file the Python
// test wrote goes through the encoder into a buffer of exactly the capacity
// asked for, the stream through zc_xz_core.h's decoder in the same program, and
// any difference from the payload aborts.  Then the same payload again into a
// buffer of exactly the stream's length (the same bytes: the outcome does not
// depend on the room, and two runs agree) and into one a byte shorter
// (ZC_XZ_E_OUTPUT, and the sanitizer sees any store past the room).
//
// case file: u32 count, then per case   u32 check id   u32 payload bytes, the payload
// stream file: per case   i32 status   u32 stored chunks   u64 size, the stream
// stdout: one line per case "<status> <stored> <size> <capacity>", a line
// "kinds <count per zcxzenc::Kind>", then "ok <count>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "zc_xzenc_core.h"

namespace {

[[noreturn]] void die(const char* what, size_t i) {
  fprintf(stderr, "case %zu: %s\n", i, what);
  abort();
}

// the payload, exactly n bytes on the heap, with the candidate array
struct Src {
  const uint8_t* p;
  uint64_t n;
  const uint32_t* c;
  uint32_t byte(uint64_t i) const {
    if (i >= n) abort();
    return p[i];
  }
  uint32_t back_byte(uint64_t i) const { return byte(i); }
  uint32_t word(uint64_t i) const {
    if (i + 4 > n) abort();
    return p[i] | p[i + 1] << 8 | p[i + 2] << 16 | (uint32_t)p[i + 3] << 24;
  }
  uint32_t match_len(uint64_t at, uint32_t d, uint32_t limit) const {
    if (d < 1 || d > at || at + limit > n) abort();
    uint32_t k = 0;
    while (k < limit && p[at + k] == p[at + k - d]) ++k;
    return k;
  }
  void rep_lens(uint64_t at, const uint32_t* d, uint32_t limit, uint32_t* l) const {
    for (int r = 0; r < 4; ++r) l[r] = d[r] <= at ? match_len(at, d[r], limit) : 0;
  }
  uint32_t cand(uint64_t i) const {
    if (i >= n) abort();
    return c[i];
  }
};

// XZENC_PLAIN_BITS: the plain form of the bit coder (a probability read and written per
// bit); the default is the batched form the device runs.  Both give the same bytes.
struct Probs {
#ifdef XZENC_PLAIN_BITS
  static constexpr bool kBatched = false;
#else
  static constexpr bool kBatched = true;
#endif
  struct Vec {
    uint32_t p[16];
  };
  // as the device does it: every probability of the batch read, then every one written,
  // which equals bit-by-bit coding only if they are distinct
  template <class F>
  Vec gather_update(uint32_t n, uint32_t bits, F idx_of) {
    if (n > 16) abort();
    Vec out;
    uint32_t idx[16];
    for (uint32_t k = 0; k < n; ++k) {
      idx[k] = idx_of(k);
      for (uint32_t j = 0; j < k; ++j)
        if (idx[j] == idx[k]) abort();
      out.p[k] = ld(idx[k]);
    }
    for (uint32_t k = 0; k < n; ++k)
      st(idx[k], (bits >> k) & 1 ? out.p[k] - (out.p[k] >> 5) : out.p[k] + ((2048 - out.p[k]) >> 5));
    return out;
  }
  uint32_t vec_get(const Vec& v, uint32_t k) const { return v.p[k]; }
  std::vector<uint16_t> v;
  uint32_t filled = 0;
  uint32_t cap() const { return (uint32_t)v.size(); }
  uint32_t ld(uint32_t i) const {
    if (i >= filled) abort();
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

struct Sink {
  uint8_t* buf;  // exactly cap bytes
  uint64_t cap;
  const Src* in;
  void put(uint64_t pos, uint32_t b) {
    if (pos >= cap || b > 255) abort();
    buf[pos] = (uint8_t)b;
  }
  void finish() {}
  void stored(uint64_t pos, uint64_t src, uint32_t len) {
    if (len < 1 || len > 65536 || pos > cap || len > cap - pos || src > in->n || len > in->n - src) abort();
    memcpy(buf + pos, in->p + src, len);
  }
};

struct Counts {
  uint64_t k[zcxzenc::kKinds] = {};
  void hit(int kind) { k[kind]++; }
};

// the decoder's side, as tests/xz/xz_core_check.cpp has it
struct DecIn {
  const uint8_t* p;
  uint64_t n;
  uint32_t byte(uint64_t i) const {
    if (i >= n) abort();
    return p[i];
  }
};
struct DecOut {
  uint8_t* buf;
  uint64_t cap, wp;
  const DecIn* in;
  void lit(uint64_t pos, uint32_t b) {
    if (pos != wp || pos >= cap) abort();
    buf[pos] = (uint8_t)b;
    wp = pos + 1;
  }
  uint32_t get(uint64_t pos) const {
    if (pos >= wp) abort();
    return buf[pos];
  }
  void copy(uint64_t pos, uint32_t dist, uint32_t len) {
    if (pos != wp || dist < 1 || dist > pos || len > cap - pos) abort();
    for (uint32_t k = 0; k < len; ++k) buf[pos + k] = buf[pos + k - dist];
    wp = pos + len;
  }
  void stored(uint64_t src, uint64_t pos, uint32_t len) {
    if (pos != wp || len > cap - pos || len > in->n - src) abort();
    memcpy(buf + pos, in->p + src, len);
    wp = pos + len;
  }
};

zcxzenc::EncResult run(const Src& src, uint32_t check, uint64_t cap, uint8_t* buf, Counts& cnt) {
  Probs probs;
  probs.v.assign(zcxz::kProbsCommon, 0);
  Sink sink{buf, cap, &src};
  return zcxzenc::encode(src, src.n, cap, check, zcxz::check_of(src, src.n, check), probs, sink, cnt);
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
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  const uint32_t count = rd<uint32_t>(f);
  Counts cnt;
  std::vector<uint64_t> table((size_t)1 << zcxzenc::kHashBits);
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t check = rd<uint32_t>(f), n = rd<uint32_t>(f);
    uint8_t* pay = (uint8_t*)malloc(n ? n : 1);
    if (n && fread(pay, 1, n, f) != n) return 2;
    uint32_t* cand = (uint32_t*)malloc(n ? (size_t)n * 4 : 4);
    Src src{pay, n, cand};
    std::fill(table.begin(), table.end(), 0);
    zcxzenc::find_all(src, n, table.data(), cand);

    const uint64_t cap = zcxzenc::capacity(n);
    uint8_t* buf = (uint8_t*)malloc(cap);
    const zcxzenc::EncResult r = run(src, check, cap, buf, cnt);
    if (r.status != zcxz::kOk) die("the capacity did not suffice", i);
    if (r.size > cap) die("a stream longer than the capacity", i);
    // back through the decoder
    {
      DecIn din{buf, r.size};
      uint8_t* back = (uint8_t*)malloc(n ? n : 1);
      Probs probs;
      probs.v.assign(zcxz::kProbsCommon, 0);
      DecOut dout{back, n, 0, &din};
      const zcxz::Result d = zcxz::decode(din, r.size, (uint64_t)n, probs, dout);
      if (d.status != zcxz::kOk) die("the decoder refuses the stream", i);
      if (d.decoded != n || d.consumed != r.size || (n && memcmp(back, pay, n) != 0)) die("the round trip differs", i);
      if (d.check_id != check) die("check id", i);
      if (n && d.stored != zcxz::check_of(src, n, check)) die("the stored check", i);
      free(back);
    }
    // exactly the stream's room: the same bytes; a byte less: E_OUTPUT
    {
      Counts scrap;
      uint8_t* exact = (uint8_t*)malloc(r.size);
      const zcxzenc::EncResult e = run(src, check, r.size, exact, scrap);
      if (e.status != zcxz::kOk || e.size != r.size || e.stored != r.stored || memcmp(exact, buf, r.size) != 0)
        die("the stream depends on the room", i);
      free(exact);
      uint8_t* tight = (uint8_t*)malloc(r.size - 1);
      const zcxzenc::EncResult t = run(src, check, r.size - 1, tight, scrap);
      if (t.status != zcxz::kOutput) die("a byte short is not E_OUTPUT", i);
      free(tight);
    }
    const int32_t status = r.status;
    fwrite(&status, 4, 1, o);
    fwrite(&r.stored, 4, 1, o);
    fwrite(&r.size, 8, 1, o);
    fwrite(buf, 1, r.size, o);
    printf("%d %u %llu %llu\n", r.status, r.stored, (unsigned long long)r.size, (unsigned long long)cap);
    free(buf);
    free(cand);
    free(pay);
  }
  printf("kinds");
  for (int k = 0; k < zcxzenc::kKinds; ++k) printf(" %llu", (unsigned long long)cnt.k[k]);
  printf("\nok %u\n", count);
  fclose(o);
  fclose(f);
  return 0;
}
