// CPU check of zc_index_core.h: the varint reader, the frame walker and the
// record walker the kernels of zc_index.hip run, compiled for the host with a
// main of its own (under ASan + UBSan where that links).
//
//   index_core_check            valid files from a writer of its own, every
//                               truncation of a small one, thousands of mutated
//                               ones; prints "ok <files read>"
//   index_core_check <cases>    reads plaintexts from a file (u32 count, then per
//                               case u8 keyed, u32 length, the bytes) and prints
//                               per case: status bundles records digest
//
// The byte source aborts on any byte(i) with i >= n; the sink aborts on any
// bundle or record beyond the capacity the host computes for the kernels
// (max_bundles / max_records of the byte count).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "zc_index_core.h"

namespace {

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "index_core_check: %s\n", what);
  abort();
}

struct Checked {
  const uint8_t* p;
  uint64_t n;
  uint32_t byte(uint64_t i) const {
    if (i >= n) die("byte() past the end");
    return p[i];
  }
};

struct Rec {
  uint8_t id[24];
  uint32_t size;
};
struct Bundle {
  uint8_t id[24];
  std::vector<Rec> recs;
};

struct Sink {
  const Checked& in;
  uint64_t bundle_cap, record_cap, n_records = 0;
  std::vector<Bundle> bundles;
  explicit Sink(const Checked& s) : in(s), bundle_cap(zcidx::max_bundles(s.n)), record_cap(zcidx::max_records(s.n)) {}
  void bundle(uint64_t b, uint64_t id_off, uint64_t info_off, uint32_t info_len) {
    if (b != bundles.size()) die("bundles out of order");
    if (b >= bundle_cap) die("a bundle beyond the capacity");
    if (info_off + info_len > in.n) die("a BundleInfo past the end");
    Bundle x;
    for (int k = 0; k < 24; k++) x.id[k] = (uint8_t)in.byte(id_off + k);
    bundles.push_back(x);
  }
  void record(uint64_t b, uint32_t k, uint64_t id_off, uint32_t size) {
    if (b + 1 != bundles.size() || k != bundles[b].recs.size()) die("records out of order");
    if (n_records >= record_cap) die("a record beyond the capacity");
    Rec r;
    for (int j = 0; j < 24; j++) r.id[j] = (uint8_t)in.byte(id_off + j);
    r.size = size;
    bundles[b].recs.push_back(r);
    n_records++;
  }
};

uint64_t g_seed = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_seed += 0x9e3779b97f4a7c15ull;
  uint64_t z = g_seed;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// a writer of its own (IndexFile::Writer's bytes)
void put_varint(std::string& s, uint32_t v) {
  while (v >= 0x80) {
    s.push_back((char)(v | 0x80));
    v >>= 7;
  }
  s.push_back((char)v);
}
std::string record_bytes(const Rec& r, bool size_first) {
  std::string a = "\x0a\x18", b = "\x10";
  a.append((const char*)r.id, 24);
  put_varint(b, r.size);
  return size_first ? b + a : a + b;
}
uint32_t adler(const std::string& s) {
  uint64_t a = 1, b = 0;
  for (unsigned char c : s) {
    a = (a + c) % 65521;
    b = (b + a) % 65521;
  }
  return (uint32_t)(b << 16 | a);
}
std::string finish(std::string p, bool keyed) {
  const uint32_t ad = adler(p);
  for (int k = 0; k < 4; k++) p.push_back((char)(ad >> (8 * k)));
  if (keyed) {
    const size_t n = 16 - p.size() % 16;
    p.append(n, (char)n);
  }
  return p;
}
std::string plaintext(const std::vector<Bundle>& bundles, bool keyed, int order) {
  std::string p;
  if (keyed)
    for (int k = 0; k < 16; k++) p.push_back((char)rnd());
  p += std::string("\x02\x08\x01", 3);
  for (const Bundle& b : bundles) {
    p += std::string("\x1a\x0a\x18", 3);
    p.append((const char*)b.id, 24);
    std::string info;
    for (size_t k = 0; k < b.recs.size(); k++) {
      const std::string r = record_bytes(b.recs[k], order == 2 ? (k & 1) : order);
      info.push_back('\x0a');
      put_varint(info, (uint32_t)r.size());
      info += r;
    }
    put_varint(p, (uint32_t)info.size());
    p += info;
  }
  p.push_back('\0');
  return finish(p, keyed);
}
std::vector<Bundle> random_bundles(size_t nb, size_t max_recs) {
  static const uint32_t edge[] = {0, 1, 127, 128, 16383, 16384, (1u << 21) - 1, 1u << 21, 1u << 28, 0xffffffffu};
  std::vector<Bundle> out(nb);
  for (Bundle& b : out) {
    for (int k = 0; k < 24; k++) b.id[k] = (uint8_t)rnd();
    b.recs.resize(rnd() % (max_recs + 1));
    for (Rec& r : b.recs) {
      for (int k = 0; k < 24; k++) r.id[k] = (uint8_t)rnd();
      r.size = rnd() % 3 ? (uint32_t)(rnd() % 70000) : edge[rnd() % 10];
    }
  }
  return out;
}

int read_checked(const std::string& p, bool keyed, Sink** out) {
  // an exact-size copy, so that the sanitizer sees any read past the end too
  uint8_t* copy = (uint8_t*)malloc(p.size() ? p.size() : 1);
  memcpy(copy, p.data(), p.size());
  const Checked in{copy, p.size()};
  Sink* sink = new Sink(in);
  const int rc = zcidx::read_file(in, p.size(), keyed, *sink);
  if (rc < 0 || rc > zcidx::kBadAdler) die("a status out of range");
  if (out)
    *out = sink;
  else
    delete sink;
  free(copy);
  return rc;
}

bool same(const std::vector<Bundle>& a, const std::vector<Bundle>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    if (memcmp(a[i].id, b[i].id, 24) || a[i].recs.size() != b[i].recs.size()) return false;
    for (size_t k = 0; k < a[i].recs.size(); k++)
      if (memcmp(a[i].recs[k].id, b[i].recs[k].id, 24) || a[i].recs[k].size != b[i].recs[k].size) return false;
  }
  return true;
}

uint64_t self_test() {
  uint64_t files = 0;
  // varint edges
  {
    const uint8_t five[] = {0xff, 0xff, 0xff, 0xff, 0x0f}, big[] = {0xff, 0xff, 0xff, 0xff, 0x1f},
                  six[] = {0x80, 0x80, 0x80, 0x80, 0x80, 0x00}, padded[] = {0x98, 0x80, 0x00};
    uint32_t v = 0;
    uint64_t pos = 0;
    if (zcidx::read_varint32(Checked{five, 5}, pos, 5, &v) != zcidx::kVarOk || v != 0xffffffffu || pos != 5)
      die("varint 2^32 - 1");
    pos = 0;
    if (zcidx::read_varint32(Checked{big, 5}, pos, 5, &v) != zcidx::kVarBad) die("varint of 33 bits");
    pos = 0;
    if (zcidx::read_varint32(Checked{six, 6}, pos, 6, &v) != zcidx::kVarBad) die("varint of 6 bytes");
    pos = 0;
    if (zcidx::read_varint32(Checked{five, 5}, pos, 3, &v) != zcidx::kVarEnd) die("varint cut");
    pos = 0;
    if (zcidx::read_varint32(Checked{padded, 3}, pos, 3, &v) != zcidx::kVarOk || v != 24 || pos != 3)
      die("padded varint");
    for (uint32_t s : {0u, 127u, 128u, 16383u, 16384u, 0xffffffffu}) {
      std::string e;
      put_varint(e, s);
      if (zcidx::varint_len(s) != e.size()) die("varint_len");
    }
  }
  // valid files: round trips, both field orders and a mix, keyed and not
  for (int round = 0; round < 60; round++) {
    const bool keyed = round & 1;
    const std::vector<Bundle> want = random_bundles(rnd() % 6, round % 7 == 0 ? 700 : 9);
    const std::string p = plaintext(want, keyed, round % 3);
    if (p.size() != zcidx::file_size(p.size() - (keyed ? 16 : 0) - 4 - (keyed ? (unsigned char)p.back() : 0), keyed))
      die("file_size");
    Sink* got = nullptr;
    if (read_checked(p, keyed, &got) != zcidx::kOk) die("a valid file did not read");
    if (!same(want, got->bundles)) die("a valid file read differently");
    delete got;
    files++;
  }
  // every truncation of a small file; a cut file is never OK (unkeyed: its
  // Adler-32 is gone or the walk ends early; keyed: the padding goes first)
  for (int keyed = 0; keyed < 2; keyed++) {
    const std::string p = plaintext(random_bundles(3, 4), keyed != 0, 2);
    for (size_t cut = 0; cut < p.size(); cut++) {
      const int rc = read_checked(p.substr(0, cut), keyed != 0, nullptr);
      if (rc == zcidx::kOk) die("a truncated file read as whole");
      files++;
    }
  }
  // mutated files: whatever the bytes, the walk stays inside them and ends;
  // with the Adler-32 (and padding) made right again after the change the
  // walkers' own statuses are reached
  uint64_t seen[zcidx::kBadAdler + 1] = {};
  for (int m = 0; m < 6000; m++) {
    const bool keyed = m & 1;
    std::string p = plaintext(random_bundles(1 + rnd() % 3, 5), keyed, 2);
    if (m & 2) {
      p[rnd() % p.size()] ^= (char)(1u << (rnd() % 8));
    } else {
      const size_t tail = 4 + (keyed ? (unsigned char)p.back() : 0);
      std::string b = p.substr(0, p.size() - tail);
      const size_t lo = keyed ? 16 : 0, i = lo + rnd() % (b.size() - lo);
      switch (rnd() % 4) {
        case 0: b[i] ^= (char)(1u << (rnd() % 8)); break;
        case 1: b[i] = (char)rnd(); break;
        case 2: b.erase(i, 1 + rnd() % 3); break;
        default: b.insert(i, 1, (char)rnd()); break;
      }
      p = finish(b, keyed);
    }
    seen[read_checked(p, keyed, nullptr)]++;
    files++;
  }
  for (int s : {zcidx::kOk, zcidx::kBadPadding, zcidx::kTruncated, zcidx::kBadMessage, zcidx::kBadBundleId,
                zcidx::kBadChunkId, zcidx::kBadAdler})
    if (!seen[s]) {
      fprintf(stderr, "status %d\n", s);
      die("the mutations never reached a status");
    }
  return files;
}

int run_cases(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the cases");
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) die("short read");
  for (uint32_t c = 0; c < n; c++) {
    uint8_t keyed = 0;
    uint32_t len = 0;
    if (fread(&keyed, 1, 1, f) != 1 || fread(&len, 4, 1, f) != 1) die("short read");
    std::string p(len, '\0');
    if (len && fread(&p[0], 1, len, f) != len) die("short read");
    Sink* got = nullptr;
    const int rc = read_checked(p, keyed != 0, &got);
    // FNV-1a over what a good file contributes: bundle ids, record ids, sizes, counts
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](const uint8_t* q, size_t k) {
      for (size_t i = 0; i < k; i++) h = (h ^ q[i]) * 0x100000001b3ull;
    };
    uint64_t nb = 0, nr = 0;
    if (rc == zcidx::kOk) {
      for (const Bundle& b : got->bundles) {
        mix(b.id, 24);
        const uint32_t cnt = (uint32_t)b.recs.size();
        mix((const uint8_t*)&cnt, 4);
        for (const Rec& r : b.recs) {
          mix(r.id, 24);
          mix((const uint8_t*)&r.size, 4);
        }
        nr += cnt;
      }
      nb = got->bundles.size();
    }
    delete got;
    printf("%d %llu %llu %016llx\n", rc, (unsigned long long)nb, (unsigned long long)nr, (unsigned long long)h);
  }
  fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) return run_cases(argv[1]);
  printf("ok %llu\n", (unsigned long long)self_test());
  return 0;
}
