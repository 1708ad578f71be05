// TEST INFRASTRUCTURE (see nocopy.hh): a Writer that records what it is given
// (Writer::add, chunk_storage.hh:50)
#pragma once
#include <set>
#include <string>
#include <vector>
#include "chunk_id.hh"
#include "nocopy.hh"
namespace ChunkStorage {
class Writer : NoCopy {
 public:
  std::vector<std::string> ids;     // blobs, in call order
  std::vector<std::string> chunks;  // the bytes
  std::vector<char> answers;        // what add returned, in call order
  // answerAsReference: add returns false for an id it has been given before
  // or that is in `known` (the index the backup started with), as the real
  // Writer::add does through ChunkIndex::addChunk (chunk_storage.cc:31-46);
  // otherwise it returns true always
  bool answerAsReference;
  std::set<std::string> known;
  Writer() : answerAsReference(false) {}
  bool add(ChunkId const& id, void const* data, size_t size) {
    ids.push_back(id.toBlob());
    chunks.push_back(std::string((const char*)data, size));
    bool added = !answerAsReference || known.insert(ids.back()).second;
    answers.push_back(added);
    return added;
  }
};
}  // namespace ChunkStorage
