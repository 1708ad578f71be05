// zbc_ref_cli.cpp -- TEST INFRASTRUCTURE ONLY.  The reference's own
// BackupCreator and ChunkIndex (compiled by oracle/Makefile from where they
// lie, over the stand-ins of standins.hh), driven over a stream from stdin as
// zutils.cc drives them, with the record list printed in the golden format.
//
// Usage: zbc_ref_cli <W> [seed_file|-] [feed_max]  < stream
//   seed_file  entries of 28 bytes: the 24-byte chunk id blob (SHA-1[0:16],
//              rolling hash little-endian) and the chunk size as uint32
//              little-endian; each goes through ChunkIndex::addChunk in order
//   feed_max   cap on the bytes handed over per handleMoreData (0: none)
//
// Output: N|D|B <offset> <size> <rolling> <sha1_16> per instruction, then one
// line `X <record index>` for each NEW record whose Writer::add returned
// false (the id was in the index already).
//
// The records are read off two hooks, in call order: Writer::add(id, size) ->
// result, and Message::serialize(instruction).  saveChunkToSave calls add
// immediately before it serializes its chunk instruction, so a chunk
// instruction that directly follows an add is NEW with the add's size; any
// other chunk instruction is a match of the W-byte window (DUP); a bytes
// instruction is BYTES.  Offsets are the running sum of the sizes.  Only the
// sequence of instructions and adds is the reference's: the wire encoding of
// the instruction stream is not produced here at all.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "backup_creator.hh"  // the reference's, via -I
#include "debug.hh"

namespace {
struct Event {
  bool isAdd;
  bool result;       // add: what addChunk answered
  bool isChunk;      // instruction: chunk_to_emit (else bytes_to_emit)
  std::string blob;  // add / chunk instruction: the 24-byte id
  uint64_t size;     // add: chunk size; bytes instruction: byte count
};
std::vector<Event> events;
Bundle::Id bundleId;  // all zero: one bundle holds everything
}  // namespace

bool ChunkStorage::Writer::add(const ChunkId& id, const void*, size_t size) {
  Event e;
  e.isAdd = true;
  e.isChunk = false;
  e.blob = id.toBlob();
  e.size = size;
  e.result = index_.addChunk(id, size, bundleId);
  events.push_back(e);
  return e.result;
}

void Message::serialize(const BackupInstruction& instr, google::protobuf::io::StringOutputStream&) {
  Event e;
  e.isAdd = false;
  e.result = false;
  e.isChunk = instr.has_chunk_to_emit();
  if (e.isChunk == instr.has_bytes_to_emit()) {
    fprintf(stderr, "instruction with both or neither field\n");
    exit(3);
  }
  e.blob = instr.chunk_to_emit();
  e.size = instr.bytes_to_emit().size();
  events.push_back(e);
}

static void printRecord(char kind, uint64_t off, uint64_t size, const std::string& blob) {
  uint64_t rolling = 0;
  unsigned char sha[16] = {0};
  if (kind != 'B') {
    memcpy(sha, blob.data(), 16);
    for (int i = 7; i >= 0; --i) rolling = (rolling << 8) | (unsigned char)blob[16 + i];
  }
  printf("%c %" PRIu64 " %" PRIu64 " %016" PRIx64 " ", kind, off, size, rolling);
  for (int k = 0; k < 16; ++k) printf("%02x", sha[k]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <W> [seed_file|-] [feed_max] < stream\n", argv[0]);
    return 2;
  }
  const uint32_t W = (uint32_t)strtoul(argv[1], 0, 0);
  const char* seedFile = argc > 2 && strcmp(argv[2], "-") ? argv[2] : 0;
  const size_t feedMax = argc > 3 ? (size_t)strtoull(argv[3], 0, 0) : 0;
  if (!W) return 2;

  verboseMode = false;  // debug.cc: no progress lines on stderr
  Config config(W);
  EncryptionKey key;
  TmpMgr tmpMgr;
  ChunkIndex index(key, tmpMgr, "index", false);  // loadIndex runs over the empty listing
  if (seedFile) {
    FILE* f = fopen(seedFile, "rb");
    if (!f) {
      perror(seedFile);
      return 2;
    }
    unsigned char ent[ChunkId::BlobSize + 4];
    size_t got;
    while ((got = fread(ent, 1, sizeof ent, f)) == sizeof ent) {
      ChunkId id;
      id.setFromBlob(ent);
      const unsigned char* s = ent + ChunkId::BlobSize;
      index.addChunk(id, s[0] | s[1] << 8 | s[2] << 16 | (uint32_t)s[3] << 24, bundleId);
    }
    fclose(f);
    if (got) {
      fprintf(stderr, "%s: truncated seed entry\n", seedFile);
      return 2;
    }
  }
  ChunkStorage::Writer writer(index);
  BackupCreator creator(config, index, writer);

  // zutils.cc: fill getInputBuffer() with up to getInputBufferSize() bytes,
  // handleMoreData(what was read), until nothing is read; then finish()
  uint64_t total = 0;
  for (;;) {
    size_t toRead = creator.getInputBufferSize();
    if (feedMax && toRead > feedMax) toRead = feedMax;
    size_t rd = fread(creator.getInputBuffer(), 1, toRead, stdin);
    if (!rd) break;
    creator.handleMoreData((unsigned)rd);
    total += rd;
  }
  if (ferror(stdin)) {
    perror("stdin");
    return 2;
  }
  creator.finish();

  std::vector<size_t> refused;
  uint64_t off = 0;
  size_t nrec = 0;
  for (size_t i = 0; i < events.size(); ++i) {
    const Event& e = events[i];
    if (e.isAdd) {
      // an add is always followed at once by the chunk instruction of the same id
      if (i + 1 == events.size() || events[i + 1].isAdd || !events[i + 1].isChunk ||
          events[i + 1].blob != e.blob) {
        fprintf(stderr, "add without its chunk instruction at event %zu\n", i);
        return 3;
      }
      continue;
    }
    if (!e.isChunk) {
      printRecord('B', off, e.size, e.blob);
      off += e.size;
    } else if (i && events[i - 1].isAdd) {
      printRecord('N', off, events[i - 1].size, e.blob);
      off += events[i - 1].size;
      if (!events[i - 1].result) refused.push_back(nrec);
    } else {
      printRecord('D', off, W, e.blob);
      off += W;
    }
    ++nrec;
  }
  if (off != total) {
    fprintf(stderr, "records cover %" PRIu64 " of %" PRIu64 " bytes\n", off, total);
    return 3;
  }
  for (size_t i = 0; i < refused.size(); ++i) printf("X %zu\n", refused[i]);
  return 0;
}
