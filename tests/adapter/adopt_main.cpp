// TEST INFRASTRUCTURE: drives GpuRepositoryAdopter (integration/
// gpu_backup_creator.hh) the way a maintainer's loop over bundles/ would:
//
//   adopt_main <chunk.max_size> <bundles file> <meta dir>
//
// The bundles file holds what Bundle::Reader would hand over, already decoded:
// LE32 bundle count, then per bundle its 24-byte id, LE32 chunk count, per chunk
// the 24-byte ChunkId blob and LE32 size, then LE64 payload length and the
// payload.  Prints "path <sidecar file>", "chunks <n> bytes <m>" and one line
// "bad <bundle id hex> <chunk index> <status>" per mismatch.
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>

#include "gpu_backup_creator.hh"

namespace {

// BundleInfo as zbackup.pb.h declares it (zbackup.proto:107-120), as far as
// the adopter reads it; the stand-in zbackup.pb.h of tests/adapter/mock keeps
// BundleInfo empty
struct ChunkRecord
{
  string id_;
  uint32_t size_;
  string const & id() const { return id_; }
  uint32_t size() const { return size_; }
};
struct Info
{
  std::vector< ChunkRecord > records;
  int chunk_record_size() const { return (int)records.size(); }
  ChunkRecord const & chunk_record( int i ) const { return records[ i ]; }
};

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

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc != 4 )
    return 2;
  try
  {
    StorableConfig storable = { { (uint32_t)strtoul( argv[ 1 ], 0, 10 ) } };
    Config config;
    config.storable = &storable;
    std::ifstream f( argv[ 2 ], std::ios::binary );
    string all = string( std::istreambuf_iterator< char >( f ), std::istreambuf_iterator< char >() );
    Input in( all );

    GpuRepositoryAdopter adopter( config, 0 );
    uint32_t bundles = (uint32_t)in.le( 4 );
    for ( uint32_t b = 0; b < bundles; ++b )
    {
      Bundle::Id id;
      memcpy( id.blob, in.take( 24 ).data(), 24 );
      Info info;
      uint32_t count = (uint32_t)in.le( 4 );
      for ( uint32_t i = 0; i < count; ++i )
      {
        ChunkRecord r;
        r.id_ = in.take( 24 );
        r.size_ = (uint32_t)in.le( 4 );
        info.records.push_back( r );
      }
      size_t payloadSize = (size_t)in.le( 8 );
      string payload = in.take( payloadSize );
      adopter.addBundle( id, info, payload );
    }
    // a bundle whose payload is short is refused and leaves nothing behind
    {
      Bundle::Id id;
      memset( id.blob, 0xEE, 24 );
      Info info;
      ChunkRecord r = { string( 24, 'x' ), 10 };
      info.records.push_back( r );
      bool threw = false;
      try
      {
        adopter.addBundle( id, info, string( 9, 'y' ) );
      }
      catch ( std::exception & e )
      {
        threw = true;
        std::cout << "refused: " << e.what() << "\n";
      }
      if ( !threw )
        throw std::runtime_error( "a short payload was accepted" );
    }
    string path;
    std::vector< GpuRepositoryAdopter::Mismatch > bad = adopter.finish( argv[ 3 ], &path );
    std::cout << "path " << path << "\n";
    std::cout << "chunks " << adopter.chunksSeen() << " bytes " << adopter.bytesSeen() << "\n";
    for ( size_t i = 0; i < bad.size(); ++i )
    {
      std::cout << "bad ";
      for ( int k = 0; k < 24; ++k )
      {
        char hex[ 3 ];
        snprintf( hex, sizeof hex, "%02x", (unsigned char)bad[ i ].bundle.blob[ k ] );
        std::cout << hex;
      }
      std::cout << " " << bad[ i ].chunk << " " << (unsigned)bad[ i ].status << "\n";
    }
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "adopt_main: " << e.what() << "\n";
    return 1;
  }
}
