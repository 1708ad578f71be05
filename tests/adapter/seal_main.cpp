// TEST INFRASTRUCTURE: drives GpuBundleSealer / GpuBundleUnsealer
// (integration/gpu_backup_creator.hh) the way Bundle::Creator::write and
// Bundle::Reader would: seal_main <32 hex digits | none> <prefix file> <body file> <out file>
// seals one bundle alone and a batch of three, writes the single file to <out
// file>, unseals it again and checks the pieces; then flips one byte and
// expects the unsealer to throw.  Prints "ok <file size>".
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <iterator>

#include "gpu_backup_creator.hh"

static string slurp( char const * path )
{
  std::ifstream f( path, std::ios::binary );
  return string( std::istreambuf_iterator< char >( f ), std::istreambuf_iterator< char >() );
}

int main( int argc, char ** argv )
{
  if ( argc != 5 )
    return 2;
  try
  {
    EncryptionKey noKey;
    unsigned char keyBytes[ 16 ];
    bool keyed = string( argv[ 1 ] ) != "none";
    for ( int i = 0; keyed && i < 16; ++i )
    {
      unsigned v;
      sscanf( argv[ 1 ] + 2 * i, "%2x", &v );
      keyBytes[ i ] = (unsigned char) v;
    }
    EncryptionKey withKey( keyBytes );
    EncryptionKey const & key = keyed ? withKey : noKey;
    string prefix = slurp( argv[ 2 ] ), body = slurp( argv[ 3 ] ), file;

    GpuBundleSealer sealer( key );
    sealer.seal( prefix, body, file );
    string half = body.substr( 0, body.size() / 2 ), none;
    std::vector< string const * > prefixes( 3, &prefix ), bodies;
    bodies.push_back( &half );
    bodies.push_back( &body );
    bodies.push_back( &none );
    std::vector< string > files;
    sealer.sealAll( prefixes, bodies, files );
    if ( files.size() != 3 || files[ 1 ] != file )
      throw std::runtime_error( "a batch seals a bundle differently" );
    std::ofstream( argv[ 4 ], std::ios::binary ).write( file.data(), file.size() );

    GpuBundleUnsealer unsealer( key );
    GpuBundleUnsealer::Opened o;
    unsealer.unseal( file, o );
    if ( o.body != body )
      throw std::runtime_error( "the body does not come back" );
    if ( o.info.empty() || prefix.size() < o.info.size() ||
         prefix.compare( prefix.size() - o.info.size(), o.info.size(), o.info ) != 0 ||
         prefix.find( o.header ) == string::npos )
      throw std::runtime_error( "the messages do not come back" );
    unsealer.unseal( files[ 2 ], o );
    if ( !o.body.empty() )
      throw std::runtime_error( "an empty body does not come back empty" );

    string bad = file;
    bad[ bad.size() / 2 ] ^= 0x20;
    bool threw = false;
    try
    {
      unsealer.unseal( bad, o );
    }
    catch ( std::exception & e )
    {
      threw = true;
      std::cout << "refused: " << e.what() << "\n";
    }
    if ( !threw )
      throw std::runtime_error( "a damaged file was accepted" );
    std::cout << "ok " << file.size() << "\n";
    return 0;
  }
  catch ( std::exception & e )
  {
    std::cerr << "seal_main: " << e.what() << "\n";
    return 1;
  }
}
