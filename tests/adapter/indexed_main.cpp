// TEST INFRASTRUCTURE: drives GpuIndexedRestorer (integration/
// gpu_backup_creator.hh) the way `zbackup nbd` drives IndexedRestorer:
//
//   indexed_main <bundles file> <backup data file> <reads file> <budget bytes>
//
// The bundles file is adopt_main's: LE32 bundle count, then per bundle its
// 24-byte id, LE32 chunk count, per chunk the 24-byte ChunkId blob and LE32
// size, then LE64 payload length and the decoded payload.  The reads file holds
// one "offset size" pair per line.  Prints "size <n>", one line
// "read <offset> <size> <sha256 hex>" per read, "out of range: threw" for a
// saveData past the end, and "fetched <f> evicted <e> resident <bytes>".
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "gpu_backup_creator.hh"

namespace {

struct Input
{
  string data;
  size_t at;
  explicit Input( string const & d ): data( d ), at( 0 ) {}
  string take( size_t n )
  {
    if ( n > data.size() - at )
      throw std::runtime_error( "the bundles file is truncated" );
    string out = data.substr( at, n );
    at += n;
    return out;
  }
  uint64_t le( int bytes )
  {
    string b = take( bytes );
    uint64_t v = 0;
    for ( int i = 0; i < bytes; ++i )
      v |= (uint64_t)(unsigned char)b[ i ] << ( 8 * i );
    return v;
  }
};

string slurp( char const * path )
{
  std::ifstream f( path, std::ios::binary );
  if ( !f )
    throw std::runtime_error( string( "cannot open " ) + path );
  return string( std::istreambuf_iterator< char >( f ), std::istreambuf_iterator< char >() );
}

// what a bundle cache over Bundle::Reader would be: the decoded payloads by bundle number
struct Payloads: GpuIndexedRestorer::PayloadSource
{
  std::vector< string > payloads;
  virtual void getPayload( size_t bundle, string & payload ) { payload = payloads.at( bundle ); }
};

string sha256Hex( string const & bytes )
{
  zc_sha256 * h = 0;
  unsigned char digest[ 32 ];
  if ( zc_sha256_create( &h ) != ZC_OK || zc_sha256_add( h, bytes.data(), bytes.size() ) != ZC_OK ||
       zc_sha256_finish( h, digest ) != ZC_OK )
    throw std::runtime_error( "zc_sha256 failed" );
  zc_sha256_destroy( h );
  string hex;
  for ( int i = 0; i < 32; ++i )
  {
    char b[ 3 ];
    snprintf( b, sizeof b, "%02x", digest[ i ] );
    hex += b;
  }
  return hex;
}

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc != 5 )
    return 2;
  try
  {
    Input in( slurp( argv[ 1 ] ) );
    string backupData = slurp( argv[ 2 ] );
    std::istringstream reads( slurp( argv[ 3 ] ) );
    uint64_t budget = strtoull( argv[ 4 ], 0, 10 );

    Payloads source;
    std::vector< GpuIndexedRestorer::ChunkList > bundles;
    uint32_t count = (uint32_t)in.le( 4 );
    for ( uint32_t b = 0; b < count; ++b )
    {
      in.take( 24 );  // the bundle's id: a restore finds bundles through the chunk index, not by id
      GpuIndexedRestorer::ChunkList chunks;
      uint32_t n = (uint32_t)in.le( 4 );
      for ( uint32_t i = 0; i < n; ++i )
      {
        string id = in.take( 24 );
        chunks.push_back( std::make_pair( id, (uint32_t)in.le( 4 ) ) );
      }
      bundles.push_back( chunks );
      source.payloads.push_back( in.take( (size_t)in.le( 8 ) ) );
    }

    GpuIndexedRestorer const restorer( backupData, bundles, source, budget );
    std::cout << "size " << restorer.size() << "\n";
    int64_t offset;
    uint64_t size;
    while ( reads >> offset >> size )
    {
      string out( size + 2, '\xEE' );
      restorer.saveData( offset, &out[ 1 ], size );
      if ( out[ 0 ] != '\xEE' || out[ size + 1 ] != '\xEE' )
        throw std::runtime_error( "saveData wrote outside its buffer" );
      std::cout << "read " << offset << " " << size << " " << sha256Hex( out.substr( 1, size ) ) << "\n";
    }
    char one;
    int threw = 0;
    try { restorer.saveData( restorer.size(), &one, 1 ); } catch ( GpuIndexedRestorer::exOutOfRange & ) { ++threw; }
    try { restorer.saveData( -1, &one, 1 ); } catch ( GpuIndexedRestorer::exOutOfRange & ) { ++threw; }
    try { restorer.saveData( 5, &one, (size_t)-3 ); } catch ( GpuIndexedRestorer::exOutOfRange & ) { ++threw; }
    restorer.saveData( restorer.size(), &one, 0 );  // 0 bytes at the very end: allowed, as in the reference
    std::cout << "out of range: " << ( threw == 3 ? "threw" : "accepted" ) << "\n";
    std::cout << "fetched " << restorer.payloadsFetched() << " evicted " << restorer.payloadsEvicted()
              << " resident " << restorer.residentPayloadBytes() << "\n";
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "indexed_main: " << e.what() << "\n";
    return 1;
  }
}
