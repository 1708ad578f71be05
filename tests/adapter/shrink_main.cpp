// TEST INFRASTRUCTURE: drives GpuDeviceBackup::backup (integration/
// gpu_backup_creator.hh) the way zbackup would for data that lies in HBM: the
// input file is uploaded once, the backup and its shrink passes run on the
// device, BackupInfo's backup_data, iterations and size come back.
//
//   shrink_main W input out_prefix
//     writes out_prefix.data (the final backup data), out_prefix.meta
//     ("iterations adds size"), out_prefix.adds (24-byte ids of Writer::add
//     calls) and out_prefix.chunks (the bytes given to them, back to back)
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <string>

#include "gpu_backup_creator.hh"

namespace {

// what GpuDeviceBackup::backup writes of zbackup's BackupInfo (zbackup.proto:161-176)
struct Info
{
  string data;
  uint32_t iters;
  uint64_t bytes;
  Info(): iters( 0 ), bytes( 0 ) {}
  string * mutable_backup_data() { return &data; }
  uint32_t iterations() const { return iters; }
  void set_iterations( uint32_t v ) { iters = v; }
  void set_size( uint64_t v ) { bytes = v; }
};

}  // namespace

int main( int argc, char ** argv )
{
  if ( argc != 4 )
  {
    fprintf( stderr, "usage: %s W input out_prefix\n", argv[ 0 ] );
    return 2;
  }
  StorableConfig st;
  st.chunk_.max_size_ = (uint32_t) strtoul( argv[ 1 ], 0, 10 );
  Config config;
  config.storable = &st;
  ChunkIndex chunkIndex;
  ChunkStorage::Writer chunkStorageWriter;
  try
  {
    std::ifstream f( argv[ 2 ], std::ios::binary );
    if ( !f )
      throw std::runtime_error( string( "cannot open " ) + argv[ 2 ] );
    string input( ( std::istreambuf_iterator< char >( f ) ), std::istreambuf_iterator< char >() );
    GpuChunkIndex gpuIndex( config, chunkIndex, 0 );
    zc_ctx * ctx = gpuIndex.context();
    void * d_data = 0;
    zcCheck( zc_device_alloc( ctx, input.size(), &d_data ), ctx, "zc_device_alloc" );
    zcCheck( zc_upload( ctx, d_data, input.data(), input.size() ), ctx, "zc_upload" );
    Info info;
    {
      GpuDeviceBackup deviceBackup( gpuIndex, chunkStorageWriter );
      deviceBackup.backup( d_data, input.size(), info );
    }
    zcCheck( zc_device_free( ctx, d_data ), ctx, "zc_device_free" );
    const string p( argv[ 3 ] );
    std::ofstream( ( p + ".data" ).c_str(), std::ios::binary ).write( info.data.data(), info.data.size() );
    std::ofstream adds( ( p + ".adds" ).c_str(), std::ios::binary ), chunks( ( p + ".chunks" ).c_str(), std::ios::binary );
    for ( size_t i = 0; i < chunkStorageWriter.ids.size(); ++i )
    {
      adds.write( chunkStorageWriter.ids[ i ].data(), 24 );
      chunks.write( chunkStorageWriter.chunks[ i ].data(), chunkStorageWriter.chunks[ i ].size() );
    }
    std::ofstream meta( ( p + ".meta" ).c_str() );
    meta << info.iters << " " << chunkStorageWriter.ids.size() << " " << info.bytes << "\n";
  }
  catch ( std::exception const & e )
  {
    fprintf( stderr, "shrink_main: %s\n", e.what() );
    return 1;
  }
  return 0;
}
