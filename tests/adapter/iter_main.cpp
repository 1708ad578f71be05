// TEST INFRASTRUCTURE: drives GpuBackupRestorer::restoreIterations (integration/
// gpu_backup_creator.hh) the way zbackup's restore would: the index files'
// bytes and the key in, BackupInfo's backup_data and iterations, the decoded
// payloads from files named by their bundle ids, the user data out.
//
//   iter_main <key hex | none> <backup data file> <iterations> <payload dir> <out file> <index file>...
//
// <payload dir>/<bundle id hex> holds a bundle's decoded payload.  Prints
//   "round <k> <bytes>" per round, "fetched <bundle id hex>" per payload asked
//   for, in order, and "restored <bytes>",
// or "exNoSuchChunk <what>" / "exDuplicateChunks <what>".
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <iterator>

#include "gpu_backup_creator.hh"

namespace {

string slurp( string const & path )
{
  std::ifstream f( path.c_str(), std::ios::binary );
  if ( !f )
    throw std::runtime_error( "cannot open " + path );
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

// what restoreIterations reads of zbackup's BackupInfo (zbackup.proto)
struct Info
{
  string data;
  uint32_t iters;
  string const & backup_data() const { return data; }
  uint32_t iterations() const { return iters; }
};

struct FilePayloads: GpuBackupRestorer::PayloadSource
{
  GpuResidentChunkIndex & index;
  string dir;
  std::vector< string > asked;
  FilePayloads( GpuResidentChunkIndex & i, string const & d ): index( i ), dir( d ) {}
  virtual void getPayload( size_t bundle, std::string & payload )
  {
    string name = hex( index.bundleId( bundle ) );
    asked.push_back( name );
    payload = slurp( dir + "/" + name );
  }
};

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc < 7 )
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
    Info info;
    info.data = slurp( argv[ 2 ] );
    info.iters = (uint32_t)atoi( argv[ 3 ] );
    std::vector< string > indexFiles;
    for ( int i = 6; i < argc; ++i )
      indexFiles.push_back( slurp( argv[ i ] ) );

    GpuResidentChunkIndex index( indexFiles, key );
    FilePayloads source( index, argv[ 4 ] );
    string out;
    std::vector< uint64_t > rounds;
    try
    {
      GpuBackupRestorer::restoreIterations( info, index, source, out, &rounds );
    }
    catch ( GpuResidentChunkIndex::exNoSuchChunk & e )
    {
      std::cout << "exNoSuchChunk " << e.what() << "\n";
      return 0;
    }
    catch ( GpuResidentChunkIndex::exDuplicateChunks & e )
    {
      std::cout << "exDuplicateChunks " << e.what() << "\n";
      return 0;
    }
    for ( size_t k = 0; k < rounds.size(); ++k )
      std::cout << "round " << k << " " << rounds[ k ] << "\n";
    for ( size_t k = 0; k < source.asked.size(); ++k )
      std::cout << "fetched " << source.asked[ k ] << "\n";
    std::ofstream f( argv[ 5 ], std::ios::binary );
    f.write( out.data(), out.size() );
    std::cout << "restored " << out.size() << "\n";
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "iter_main: " << e.what() << "\n";
    return 1;
  }
}
