// TEST INFRASTRUCTURE: drives GpuXzBundleDecoder (integration/
// gpu_backup_creator.hh) and the two paths that keep its payloads in HBM:
//
//   xz_main <chunk.max_size> <bundles file> <backup data file> <reads file> <meta dir host> <meta dir device>
//
// The bundles file is adopt_main's with the bundle's LZMA body behind each
// payload: LE32 bundle count, then per bundle its 24-byte id, LE32 chunk
// count, per chunk the 24-byte ChunkId blob and LE32 size, LE64 payload length
// and the payload liblzma decoded, LE64 body length and the xz stream.
// Prints "decodeAll ok <n>", "decode ok", one "threw: <message>" per refused
// body, "in use: threw"; then per adopter ("host": addBundle over decodeAll's
// payloads, "device": addBundlesDevice over decodeToDevice's) "<which> path
// <sidecar>", "<which> chunks <n> bytes <m>" and "<which> bad <bundle id hex>
// <chunk> <status>" lines; then "size <n>", "read <offset> <size> <sha256>"
// per read served from the device payloads and "fetched <f>".
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "gpu_backup_creator.hh"

namespace {

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

string slurp( char const * path )
{
  std::ifstream f( path, std::ios::binary );
  if ( !f )
    throw std::runtime_error( string( "cannot open " ) + path );
  return string( std::istreambuf_iterator< char >( f ), std::istreambuf_iterator< char >() );
}

string hexOf( unsigned char const * p, int n )
{
  string hex;
  for ( int i = 0; i < n; ++i )
  {
    char b[ 3 ];
    snprintf( b, sizeof b, "%02x", p[ i ] );
    hex += b;
  }
  return hex;
}

string sha256Hex( string const & bytes )
{
  zc_sha256 * h = 0;
  unsigned char digest[ 32 ];
  if ( zc_sha256_create( &h ) != ZC_OK || zc_sha256_add( h, bytes.data(), bytes.size() ) != ZC_OK ||
       zc_sha256_finish( h, digest ) != ZC_OK )
    throw std::runtime_error( "zc_sha256 failed" );
  zc_sha256_destroy( h );
  return hexOf( digest, 32 );
}

// the restorer must not come here: every payload it needs is in HBM already
struct NoHostPayloads: GpuIndexedRestorer::PayloadSource
{
  virtual void getPayload( size_t, string & ) { throw std::runtime_error( "a host payload was asked for" ); }
};

void report( char const * which, GpuRepositoryAdopter & adopter, char const * dir )
{
  string path;
  std::vector< GpuRepositoryAdopter::Mismatch > bad = adopter.finish( dir, &path );
  std::cout << which << " path " << path << "\n";
  std::cout << which << " chunks " << adopter.chunksSeen() << " bytes " << adopter.bytesSeen() << "\n";
  for ( size_t i = 0; i < bad.size(); ++i )
    std::cout << which << " bad " << hexOf( (unsigned char const *)bad[ i ].bundle.blob, 24 ) << " " << bad[ i ].chunk
              << " " << (unsigned)bad[ i ].status << "\n";
}

template< class F >
void mustThrow( char const * what, F f )
{
  try
  {
    f();
  }
  catch ( std::runtime_error & e )
  {
    std::cout << "threw: " << e.what() << "\n";
    return;
  }
  throw std::runtime_error( string( what ) + " was accepted" );
}

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc != 7 )
    return 2;
  try
  {
    StorableConfig storable = { { (uint32_t)strtoul( argv[ 1 ], 0, 10 ) } };
    Config config;
    config.storable = &storable;
    Input in( slurp( argv[ 2 ] ) );
    string backupData = slurp( argv[ 3 ] );
    std::istringstream reads( slurp( argv[ 4 ] ) );

    std::vector< Bundle::Id > ids;
    std::vector< Info > infos;
    std::vector< string > payloads, bodies;
    std::vector< GpuIndexedRestorer::ChunkList > lists;
    uint32_t count = (uint32_t)in.le( 4 );
    for ( uint32_t b = 0; b < count; ++b )
    {
      Bundle::Id id;
      memcpy( id.blob, in.take( 24 ).data(), 24 );
      ids.push_back( id );
      Info info;
      GpuIndexedRestorer::ChunkList list;
      uint32_t n = (uint32_t)in.le( 4 );
      for ( uint32_t i = 0; i < n; ++i )
      {
        ChunkRecord r;
        r.id_ = in.take( 24 );
        r.size_ = (uint32_t)in.le( 4 );
        info.records.push_back( r );
        list.push_back( std::make_pair( r.id_, r.size_ ) );
      }
      infos.push_back( info );
      lists.push_back( list );
      payloads.push_back( in.take( (size_t)in.le( 8 ) ) );
      bodies.push_back( in.take( (size_t)in.le( 8 ) ) );
    }
    std::vector< string const * > bodyPtrs;
    std::vector< Info const * > infoPtrs;
    std::vector< uint64_t > sizes;
    std::vector< size_t > numbers;
    for ( size_t b = 0; b < bodies.size(); ++b )
    {
      bodyPtrs.push_back( &bodies[ b ] );
      infoPtrs.push_back( &infos[ b ] );
      sizes.push_back( payloads[ b ].size() );
      numbers.push_back( b );
    }

    GpuXzBundleDecoder decoder;
    // ---- to the host: Bundle::Reader's payload strings ----
    std::vector< string > decoded;
    decoder.decodeAll( bodyPtrs, sizes, decoded );
    if ( decoded != payloads )
      throw std::runtime_error( "decodeAll's payloads differ from liblzma's" );
    std::cout << "decodeAll ok " << decoded.size() << "\n";
    string one;
    decoder.decode( bodies[ 0 ], sizes[ 0 ], one );
    if ( one != payloads[ 0 ] )
      throw std::runtime_error( "decode's payload differs from liblzma's" );
    std::cout << "decode ok\n";
    std::vector< string > none;
    decoder.decodeAll( std::vector< string const * >(), std::vector< uint64_t >(), none );
    // ---- what Bundle::Reader refuses: a bad stream, bytes behind it, another size ----
    string cut = bodies[ 1 ].substr( 0, bodies[ 1 ].size() - 7 ), longer = bodies[ 1 ] + string( 4, '\0' );
    mustThrow( "a truncated body", [ & ] { decoder.decode( cut, sizes[ 1 ], one ); } );
    mustThrow( "a body with bytes behind its stream", [ & ] { decoder.decode( longer, sizes[ 1 ], one ); } );
    mustThrow( "a payload one byte short of its size", [ & ] { decoder.decode( bodies[ 1 ], sizes[ 1 ] + 1, one ); } );
    mustThrow( "a payload one byte over its room", [ & ] { decoder.decode( bodies[ 1 ], sizes[ 1 ] - 1, one ); } );
    {
      std::vector< string const * > mixed( bodyPtrs );
      mixed[ 1 ] = &cut;
      GpuXzBundleDecoder::DevicePayloads refused;
      mustThrow( "a truncated body among good ones", [ & ] { decoder.decodeToDevice( mixed, sizes, refused ); } );
    }  // refused frees what the call had made
    // ---- to the device ----
    GpuXzBundleDecoder::DevicePayloads dev;
    decoder.decodeToDevice( bodyPtrs, sizes, dev );
    try
    {
      decoder.decodeToDevice( bodyPtrs, sizes, dev );
      throw std::runtime_error( "a DevicePayloads in use was taken again" );
    }
    catch ( std::logic_error & )
    {
      std::cout << "in use: threw\n";
    }
    {
      GpuRepositoryAdopter host( config, 0 ), device( config, 0 );
      for ( size_t b = 0; b < ids.size(); ++b )
        host.addBundle( ids[ b ], infos[ b ], decoded[ b ] );
      report( "host", host, argv[ 5 ] );
      // a size that is not the bundle's is refused and leaves nothing behind
      std::vector< Info const * > wrong( infoPtrs );
      wrong[ 0 ] = &infos[ 1 ];
      mustThrow( "another bundle's BundleInfo", [ & ] { device.addBundlesDevice( ids, wrong, dev ); } );
      device.addBundlesDevice( ids, infoPtrs, dev );
      report( "device", device, argv[ 6 ] );
    }
    {
      NoHostPayloads source;
      GpuIndexedRestorer restorer( backupData, lists, source, 0 );
      restorer.setPayloads( numbers, dev );
      std::cout << "size " << restorer.size() << "\n";
      int64_t offset;
      uint64_t size;
      while ( reads >> offset >> size )
      {
        string out( size, '\xEE' );
        restorer.saveData( offset, &out[ 0 ], size );
        std::cout << "read " << offset << " " << size << " " << sha256Hex( out ) << "\n";
      }
      std::cout << "fetched " << restorer.payloadsFetched() << "\n";
      restorer.clearPayloads();
      char c;
      mustThrow( "a read after clearPayloads", [ & ] { restorer.saveData( 0, &c, 1 ); } );
    }
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "xz_main: " << e.what() << "\n";
    return 1;
  }
}
