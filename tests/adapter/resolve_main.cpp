// TEST INFRASTRUCTURE: drives GpuResidentChunkIndex (integration/
// gpu_backup_creator.hh) the way a restore would: the index files' bytes and
// the key in, a batch findChunk and the plan of one backup out.
//
//   resolve_main <key hex | none> <backup data file> <ids file> <index file>...
//
// The ids file holds 24-byte ChunkId blobs back to back.  Prints
//   "index bundles <B> records <N> ids <I> flagged <F>", "status <s> ..." (one per index file),
//   "find <id hex> <bundle id hex | none> <offset> <size>" per id,
//   "plan length <L> used <U> entries <E>", "used <bundle id hex> <payload size>" per used bundle,
//   "entry <slot> <off> <size> <dst>" per entry,
// or, where the plan throws, "plan exNoSuchChunk <what>" / "plan exDuplicateChunks <what>".
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>

#include "gpu_backup_creator.hh"

namespace {

string slurp( char const * path )
{
  std::ifstream f( path, std::ios::binary );
  if ( !f )
    throw std::runtime_error( string( "cannot open " ) + path );
  return string( std::istreambuf_iterator< char >( f ), std::istreambuf_iterator< char >() );
}

string hex( string const & bytes )
{
  string out;
  for ( size_t i = 0; i < bytes.size(); ++i )
  {
    char b[ 3 ];
    snprintf( b, sizeof b, "%02x", (unsigned char)bytes[ i ] );
    out += b;
  }
  return out;
}

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc < 4 )
    return 2;
  try
  {
    EncryptionKey noKey;
    unsigned char keyBytes[ 16 ];
    bool keyed = string( argv[ 1 ] ) != "none";
    for ( int i = 0; keyed && i < 16; ++i )
    {
      unsigned v = 0;
      sscanf( argv[ 1 ] + 2 * i, "%2x", &v );
      keyBytes[ i ] = (unsigned char)v;
    }
    EncryptionKey withKey( keyBytes );
    EncryptionKey const & key = keyed ? withKey : noKey;
    string backupData = slurp( argv[ 2 ] ), idBlobs = slurp( argv[ 3 ] );
    std::vector< string > indexFiles;
    for ( int i = 4; i < argc; ++i )
      indexFiles.push_back( slurp( argv[ i ] ) );

    GpuResidentChunkIndex index( indexFiles, key );
    uint64_t records = 0, ids = 0, flagged = 0;
    index.counts( records, ids, flagged );
    std::cout << "index bundles " << index.bundles() << " records " << records << " ids " << ids << " flagged "
              << flagged << "\n";
    std::cout << "status";
    for ( size_t i = 0; i < index.fileStatus().size(); ++i )
      std::cout << " " << index.fileStatus()[ i ];
    std::cout << "\n";

    std::vector< string > wanted;
    for ( size_t at = 0; at + 24 <= idBlobs.size(); at += 24 )
      wanted.push_back( idBlobs.substr( at, 24 ) );
    std::vector< GpuResidentChunkIndex::Found > found;
    index.findChunks( wanted, found );
    for ( size_t i = 0; i < found.size(); ++i )
      std::cout << "find " << hex( wanted[ i ] ) << " "
                << ( found[ i ].bundle == GpuResidentChunkIndex::NoBundle ? string( "none" )
                                                                          : hex( index.bundleId( found[ i ].bundle ) ) )
                << " " << found[ i ].offset << " " << found[ i ].size << "\n";

    GpuResidentChunkIndex::Plan plan;
    try
    {
      index.plan( backupData, plan );
    }
    catch ( GpuResidentChunkIndex::exNoSuchChunk & e )
    {
      std::cout << "plan exNoSuchChunk " << e.what() << "\n";
      return 0;
    }
    catch ( GpuResidentChunkIndex::exDuplicateChunks & e )
    {
      std::cout << "plan exDuplicateChunks " << e.what() << "\n";
      return 0;
    }
    std::cout << "plan length " << plan.length << " used " << plan.used.size() << " entries " << plan.slot.size()
              << "\n";
    for ( size_t k = 0; k < plan.used.size(); ++k )
      std::cout << "used " << hex( index.bundleId( plan.used[ k ] ) ) << " " << plan.usedSize[ k ] << "\n";
    for ( size_t e = 0; e < plan.slot.size(); ++e )
      std::cout << "entry " << plan.slot[ e ] << " " << plan.off[ e ] << " " << plan.size[ e ] << " " << plan.dst[ e ]
                << "\n";
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "resolve_main: " << e.what() << "\n";
    return 1;
  }
}
