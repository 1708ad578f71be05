// standins.hh -- TEST INFRASTRUCTURE ONLY.
//
// Stand-ins for the headers of the reference that its backup_creator.cc and
// chunk_index.cc include but that cannot be compiled without protobuf, file
// I/O and threads.  oracle/Makefile force-includes this file in front of every
// reference source of _ref/zbc_ref_cli; each block below defines the include
// guard of the header it replaces, so the reference's own #include of that
// header expands to nothing and the names come from here.  Only what the seven
// compiled reference sources name is declared.  All of it is this project's
// text; the state machine (BackupCreator) and the index (ChunkIndex) are the
// reference's own and are NOT replaced.
//
// The two hooks the driver (zbc_ref_cli.cpp) listens on are declared here and
// defined there: ChunkStorage::Writer::add and Message::serialize.
#ifndef ZBC_REFPIN_STANDINS_HH
#define ZBC_REFPIN_STANDINS_HH

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

struct ChunkId;
class ChunkIndex;

// --- zbackup.pb.h (generated from zbackup.proto; no guard to define: the
// file of that name next to this one is found through -I) ------------------
class BackupInstruction {
  std::string chunk_, bytes_;
  bool has_chunk_, has_bytes_;

 public:
  BackupInstruction() : has_chunk_(false), has_bytes_(false) {}
  void set_chunk_to_emit(const std::string& v) { chunk_ = v; has_chunk_ = true; }
  void set_bytes_to_emit(const void* p, size_t n) { bytes_.assign((const char*)p, n); has_bytes_ = true; }
  bool has_chunk_to_emit() const { return has_chunk_; }
  bool has_bytes_to_emit() const { return has_bytes_; }
  const std::string& chunk_to_emit() const { return chunk_; }
  const std::string& bytes_to_emit() const { return bytes_; }
};
class BundleInfo_ChunkRecord {
  std::string id_;

 public:
  const std::string& id() const { return id_; }
  uint32_t size() const { return 0; }
};
class BundleInfo {
  BundleInfo_ChunkRecord none_;

 public:
  int chunk_record_size() const { return 0; }
  const BundleInfo_ChunkRecord& chunk_record(int) const { return none_; }
};

// --- <google/protobuf/io/zero_copy_stream_impl_lite.h> ---------------------
namespace google {
namespace protobuf {
namespace io {
class StringOutputStream {
 public:
  explicit StringOutputStream(std::string*) {}
};
}  // namespace io
}  // namespace protobuf
}  // namespace google

// --- config.hh --------------------------------------------------------------
#define CONFIG_HH_INCLUDED
#define GET_STORABLE(storage, property) storage##_##property
class Config {
 public:
  uint32_t chunk_max_size;
  explicit Config(uint32_t w) : chunk_max_size(w) {}
};

// --- bundle.hh --------------------------------------------------------------
#define BUNDLE_HH_INCLUDED
namespace Bundle {
enum { IdSize = 24 };
struct Id {
  char blob[IdSize];
  bool operator!=(const Id& o) const { return memcmp(blob, o.blob, sizeof blob) != 0; }
};
}  // namespace Bundle

// --- dir.hh: a listing with no entries (loadIndex is never asked to load) ----
#define DIR_HH_INCLUDED
namespace Dir {
class Entry {
 public:
  std::string getFileName() const { return std::string(); }
};
class Listing {
 public:
  explicit Listing(const std::string&) {}
  bool getNext(Entry&) { return false; }
};
inline std::string addPath(const std::string& a, const std::string& b) { return a + "/" + b; }
}  // namespace Dir

// --- encryption_key.hh --------------------------------------------------------
#define ENCRYPTION_KEY_HH_INCLUDED
class EncryptionKey {
 public:
  bool hasKey() const { return false; }
};

// --- tmp_mgr.hh, file.hh ------------------------------------------------------
#define TMP_MGR_HH_INCLUDED
#define FILE_HH_INCLUDED
class TmpMgr {};

// --- index_file.hh: a reader that reads nothing ------------------------------
#define INDEX_FILE_HH_INCLUDED
namespace IndexFile {
class Reader {
 public:
  Reader(const EncryptionKey&, const std::string&) {}
  bool readNextRecord(BundleInfo&, Bundle::Id&) { return false; }
};
}  // namespace IndexFile

// --- message.hh: hook 1, defined by the driver --------------------------------
#define MESSAGE_HH_INCLUDED
namespace Message {
void serialize(const BackupInstruction&, google::protobuf::io::StringOutputStream&);
}

// --- chunk_storage.hh: hook 2, defined by the driver.  add() hands the id to
// the real ChunkIndex::addChunk and returns its answer, as the reference's
// Writer::add does before it touches any bundle ------------------------------
#define CHUNK_STORAGE_HH_INCLUDED
namespace ChunkStorage {
class Writer {
  ChunkIndex& index_;

 public:
  explicit Writer(ChunkIndex& index) : index_(index) {}
  bool add(const ChunkId&, const void* data, size_t size);
};
}  // namespace ChunkStorage

#endif
