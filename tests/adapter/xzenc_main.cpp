// TEST INFRASTRUCTURE: drives GpuXzBundleCompressor and GpuXzBundleDecoder
// (integration/gpu_backup_creator.hh) against each other:
//
//   xzenc_main <payloads file> <bodies file>
//
// The payloads file: LE32 count, then per payload LE64 length and the bytes.
// Every payload goes through compressAll in one call and the first also
// through compress; the bodies go through decodeAll, and the program fails
// unless every payload comes back.  The bodies file gets LE32 count, then per
// body LE64 length and the xz stream, for the test to hold to another decoder.
// Prints "compressAll ok <n>", "compress ok", "decodeAll ok <n>".
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>

#include "gpu_backup_creator.hh"

namespace {

uint64_t le( string const & d, size_t & at, int bytes )
{
  if ( (size_t) bytes > d.size() - at )
    throw std::runtime_error( "the payloads file is truncated" );
  uint64_t v = 0;
  for ( int i = 0; i < bytes; ++i )
    v |= (uint64_t)(unsigned char) d[ at + i ] << ( 8 * i );
  at += bytes;
  return v;
}

void putLe( std::ofstream & o, uint64_t v, int bytes )
{
  for ( int i = 0; i < bytes; ++i )
    o.put( (char)( v >> ( 8 * i ) ) );
}

}

int main( int argc, char ** argv )
{
  if ( argc < 3 )
    return 2;
  try
  {
    std::ifstream f( argv[ 1 ], std::ios::binary );
    string d( ( std::istreambuf_iterator< char >( f ) ), std::istreambuf_iterator< char >() );
    size_t at = 0;
    size_t n = le( d, at, 4 );
    std::vector< string > payloads( n );
    for ( size_t i = 0; i < n; ++i )
    {
      uint64_t len = le( d, at, 8 );
      if ( len > d.size() - at )
        throw std::runtime_error( "the payloads file is truncated" );
      payloads[ i ] = d.substr( at, len );
      at += len;
    }
    std::vector< string const * > in( n );
    std::vector< uint64_t > sizes( n );
    for ( size_t i = 0; i < n; ++i )
    {
      in[ i ] = &payloads[ i ];
      sizes[ i ] = payloads[ i ].size();
    }
    GpuXzBundleCompressor enc;
    std::vector< string > bodies;
    enc.compressAll( in, bodies );
    if ( bodies.size() != n )
      throw std::runtime_error( "compressAll: another number of bodies" );
    printf( "compressAll ok %zu\n", n );
    if ( n )
    {
      string one;
      enc.compress( payloads[ 0 ], one );
      if ( one != bodies[ 0 ] )
        throw std::runtime_error( "compress and compressAll differ" );
      printf( "compress ok\n" );
    }
    GpuXzBundleDecoder dec;
    std::vector< string const * > b( n );
    for ( size_t i = 0; i < n; ++i )
      b[ i ] = &bodies[ i ];
    std::vector< string > back;
    dec.decodeAll( b, sizes, back );
    for ( size_t i = 0; i < n; ++i )
      if ( back[ i ] != payloads[ i ] )
        throw std::runtime_error( "a payload did not come back" );
    printf( "decodeAll ok %zu\n", n );
    std::ofstream o( argv[ 2 ], std::ios::binary );
    putLe( o, n, 4 );
    for ( size_t i = 0; i < n; ++i )
    {
      putLe( o, bodies[ i ].size(), 8 );
      o.write( bodies[ i ].data(), bodies[ i ].size() );
    }
  }
  catch ( std::exception & e )
  {
    printf( "threw: %s\n", e.what() );
    return 1;
  }
  return 0;
}
