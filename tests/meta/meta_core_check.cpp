// TEST INFRASTRUCTURE: zbackup_amd/csrc/zc_meta_core.h -- the scalar definition
// of a chunk's metadata record the kernels of zc_meta.hip are checked against --
// compiled for the host with a main of its own (under ASan + UBSan where that
// links) and run over chunk files the test writes.
//
//   meta_core_check W file...        one line per file, the record of the file's bytes
//                                    as one chunk under chunk.max_size W:
//                                    sha1(32 hex) rolling size anchor_def anchor gear fingerprint
//   meta_core_check --time W S file  the file cut into chunks of S bytes (the last may be
//                                    shorter), every record computed once on this core:
//                                    "chunks bytes seconds xor-of-rolling"
//   meta_core_check --compare        compare()'s status bits on hand-made pairs: "ok"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "zc_meta_core.h"

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t rd;
  out.clear();
  while ((rd = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + rd);
  fclose(f);
  return true;
}

static int check_compare() {
  zcmeta::Record r{};
  for (int k = 0; k < 16; ++k) r.sha1[k] = (uint8_t)(k * 7 + 1);
  r.rolling = 0x0123456789abcdefull;
  r.size = 4096;
  zcmeta::Expect e{};
  memcpy(e.sha1, r.sha1, 16);
  e.rolling = r.rolling;
  e.size = r.size;
  if (zcmeta::compare(r, e) != 0) return 1;
  e.sha1[15] ^= 1;
  if (zcmeta::compare(r, e) != zcmeta::kBadSha1) return 2;
  e.rolling ^= 1ull << 63;
  if (zcmeta::compare(r, e) != (zcmeta::kBadSha1 | zcmeta::kBadRolling)) return 3;
  e.sha1[15] ^= 1;
  e.size = 4095;
  if (zcmeta::compare(r, e) != (zcmeta::kBadRolling | zcmeta::kBadSize)) return 4;
  // a record without an anchor carries no gear and no fingerprint, whatever it is handed
  const zcmeta::Record n = zcmeta::make_record(r.sha1, 5, 7, 9, zcmeta::kNoAnchor, 0x1234, 0x5678);
  if (n.gear != 0 || n.fingerprint != 0 || n.anchor != zcmeta::kNoAnchor || n.rolling != 5 || n.size != 7) return 5;
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "--compare") == 0) return check_compare();
  if (argc == 5 && strcmp(argv[1], "--time") == 0) {
    const uint32_t W = (uint32_t)strtoul(argv[2], 0, 10), S = (uint32_t)strtoul(argv[3], 0, 10);
    std::vector<uint8_t> data;
    if (!W || !S || !read_file(argv[4], data)) return 2;
    uint64_t x = 0, chunks = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t at = 0; at < data.size(); at += S, ++chunks) {
      const uint32_t n = (uint32_t)(data.size() - at < S ? data.size() - at : S);
      const zcmeta::Record r = zcmeta::chunk_record(data.data() + at, n, W);
      x ^= r.rolling ^ r.fingerprint ^ r.sha1[0];
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%llu %zu %.6f %016llx\n", (unsigned long long)chunks, data.size(), sec, (unsigned long long)x);
    return 0;
  }
  if (argc < 3) {
    fprintf(stderr, "usage: %s W file... | --time W S file | --compare\n", argv[0]);
    return 2;
  }
  const uint32_t W = (uint32_t)strtoul(argv[1], 0, 10);
  for (int i = 2; i < argc; ++i) {
    std::vector<uint8_t> data;
    if (!W || !read_file(argv[i], data) || data.empty() || data.size() > 0xFFFFFFFFull) {
      fprintf(stderr, "%s: cannot read a chunk of 1 .. 2^32 - 1 bytes\n", argv[i]);
      return 2;
    }
    // an exact-size copy: a read past the chunk's end is a sanitizer report
    std::vector<uint8_t> exact(data.begin(), data.end());
    exact.shrink_to_fit();
    const zcmeta::Record r = zcmeta::chunk_record(exact.data(), (uint32_t)exact.size(), W);
    for (int k = 0; k < 16; ++k) printf("%02x", r.sha1[k]);
    printf(" %llu %u %u %u %u %llu\n", (unsigned long long)r.rolling, r.size, r.anchor_def, r.anchor, r.gear,
           (unsigned long long)r.fingerprint);
  }
  return 0;
}
