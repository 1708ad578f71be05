// gpu_backup_creator.hh -- the zbackup-side binding of libzchunk (include/zchunk.h).
//
// Header-only C++ adapter with BackupCreator's public interface
// (/root/reference/backup_creator.hh:73-89), compiled into zbackup next to
// backup_creator.cc.  ZBackup::backupFromFileHandle (zutils.cc:89-182) keeps its
// read loop and its iterative shrink loop; it only constructs these classes:
//
//   GpuChunkIndex gpuIndex( config, chunkIndex, 0, ZC_FLAG_SHA1, metaDir );  // once per backup
//   GpuBackupCreator backupCreator( gpuIndex, chunkStorageWriter );  // zutils.cc:96
//   ...
//   GpuBackupCreator backupCreator( gpuIndex, chunkStorageWriter );  // zutils.cc:140
//   ...
//   chunkStorageWriter.commit();                                     // zutils.cc:175
//   gpuIndex.saveChunkMeta( metaDir );   // metaDir = Dir::addPath( dir, "zchunk" )
//
// GpuChunkIndex is the device-side probe set: one libzchunk context, seeded
// with every chunk id of the repository's index files (ChunkIndex::loadIndex
// driving this class as its IndexProcessor, chunk_index.cc:26-79).  Every
// GpuBackupCreator on it is one stream on that context (zc_reset), so a shrink
// pass matches the chunks the passes before it wrote, as the reference's
// passes share one ChunkIndex that Writer::add grows (chunk_storage.cc:31-46).
//
// Records are taken as they are cut (zc_take_records, during handleMoreData):
// a NEW chunk goes to Writer::add with its bytes, every record to the
// instruction stream (Message::serialize, message.cc:16-23), exactly as
// saveChunkToSave / addChunkIfMatched / outputInstruction do
// (backup_creator.cc:110-145,242-273).  Errors become exceptions, as the
// reference's DEF_EX / CHECK paths are.
#ifndef GPU_BACKUP_CREATOR_HH_INCLUDED
#define GPU_BACKUP_CREATOR_HH_INCLUDED

#include <dirent.h>
#include <google/protobuf/io/zero_copy_stream_impl_lite.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "chunk_id.hh"
#include "chunk_index.hh"
#include "chunk_storage.hh"
#include "config.hh"
#include "encryption_key.hh"
#include "message.hh"
#include "nocopy.hh"
#include "sptr.hh"
#include "zbackup.pb.h"
#include "zchunk.h"

inline void zcCheck( int rc, zc_ctx * ctx, char const * what )
{
  if ( rc != ZC_OK )
    throw std::runtime_error( std::string( what ) + ": " + ( ctx ? zc_last_error( ctx ) : "libzchunk" ) );
}

/// The content-anchor metadata of a repository's chunks (zc_chunk_meta, ABI 5),
/// kept in files of its own beside the index -- "<repo>/zchunk/<sha256 hex>" --
/// and never inside index/ or bundles/, whose formats stay zbackup's.  One
/// file per backup, written at the end of the backup next to the index file
/// Writer::commit moves into place (chunk_storage.cc:61-90); a new process
/// reads every file and seeds the ids ChunkIndex::loadIndex reports together
/// with the entries that match them by full ChunkId.  The metadata is a pure
/// function of a chunk's bytes, so it never goes stale: entries of chunks a gc
/// removed are simply never joined to an id, and a file that is damaged or of
/// another anchor definition only costs speed (those ids are screened by key),
/// never a different backup.
///
/// File: "ZCMETA01", LE32 record size (48), LE32 0, LE64 count, count records,
/// then the SHA-256 of everything before it (zc_sha256_*); written to a
/// temporary name and renamed, as tmp_mgr.cc:16-24 does for zbackup's files.
class GpuChunkMetaSidecar
{
  static void sha256( std::string const & data, unsigned char out[ 32 ] )
  {
    zc_sha256 * h = 0;
    if ( zc_sha256_create( &h ) != ZC_OK )
      throw std::runtime_error( "zc_sha256_create" );
    zc_sha256_add( h, data.data(), data.size() );
    zc_sha256_finish( h, out );
    zc_sha256_destroy( h );
  }

public:
  /// the entries of one file; false (and nothing added) if it is not a valid one
  static bool read( std::string const & path, std::vector< zc_chunk_meta > & out )
  {
    FILE * f = fopen( path.c_str(), "rb" );
    if ( !f )
      return false;
    std::string data;
    char buf[ 65536 ];
    size_t rd;
    while ( ( rd = fread( buf, 1, sizeof( buf ), f ) ) > 0 )
      data.append( buf, rd );
    fclose( f );
    if ( data.size() < 24 + 32 || data.compare( 0, 8, "ZCMETA01" ) != 0 )
      return false;
    uint32_t recSize;
    uint64_t count;
    memcpy( &recSize, data.data() + 8, 4 );
    memcpy( &count, data.data() + 16, 8 );
    if ( recSize != sizeof( zc_chunk_meta ) || count > ( data.size() - 56 ) / recSize ||
         data.size() != 24 + count * recSize + 32 )
      return false;
    unsigned char want[ 32 ];
    sha256( data.substr( 0, data.size() - 32 ), want );
    if ( memcmp( want, data.data() + data.size() - 32, 32 ) != 0 )
      return false;
    size_t at = out.size();
    out.resize( at + count );
    memcpy( &out[ at ], data.data() + 24, count * recSize );
    return true;
  }

  /// every valid file of dir (a missing dir: none)
  static void readDir( std::string const & dir, std::vector< zc_chunk_meta > & out )
  {
    DIR * d = opendir( dir.c_str() );
    if ( !d )
      return;
    while ( struct dirent * e = readdir( d ) )
    {
      std::string name( e->d_name );
      if ( name.size() == 64 && name.find_first_not_of( "0123456789abcdef" ) == std::string::npos )
        read( dir + "/" + name, out );
    }
    closedir( d );
  }

  /// the metadata of the chunks ctx's streams added, as one new file of dir
  /// (made if missing); returns its path, or "" when there is nothing to write
  static std::string write( std::string const & dir, zc_ctx * ctx )
  {
    size_t n = 0;
    zc_export_chunk_meta( ctx, 0, 0, &n );
    if ( !n )
      return std::string();
    std::vector< zc_chunk_meta > meta( n );
    zcCheck( zc_export_chunk_meta( ctx, meta.data(), meta.size(), &n ), ctx, "zc_export_chunk_meta" );
    return write( dir, meta );
  }

  /// the same for records from anywhere (GpuRepositoryAdopter's, say)
  static std::string write( std::string const & dir, std::vector< zc_chunk_meta > const & meta )
  {
    size_t n = meta.size();
    if ( !n )
      return std::string();
    std::string data( "ZCMETA01", 8 );
    uint32_t words[ 2 ] = { (uint32_t)sizeof( zc_chunk_meta ), 0 };
    uint64_t count = n;
    data.append( (char const *)words, 8 );
    data.append( (char const *)&count, 8 );
    data.append( (char const *)meta.data(), n * sizeof( zc_chunk_meta ) );
    unsigned char sum[ 32 ];
    sha256( data, sum );
    data.append( (char const *)sum, 32 );
    char hex[ 65 ];
    for ( int i = 0; i < 32; ++i )
      snprintf( hex + 2 * i, 3, "%02x", sum[ i ] );
    mkdir( dir.c_str(), 0755 );
    std::string path = dir + "/" + hex, tmp = path + ".tmp";
    FILE * f = fopen( tmp.c_str(), "wb" );
    if ( !f || fwrite( data.data(), 1, data.size(), f ) != data.size() || fflush( f ) != 0 ||
         fsync( fileno( f ) ) != 0 )
    {
      if ( f )
        fclose( f );
      unlink( tmp.c_str() );
      throw std::runtime_error( "chunk metadata: cannot write " + tmp );
    }
    fclose( f );
    if ( rename( tmp.c_str(), path.c_str() ) != 0 )
    {
      unlink( tmp.c_str() );
      throw std::runtime_error( "chunk metadata: cannot rename " + tmp );
    }
    return path;
  }
};

/// The repository's chunk index on the GPU (one libzchunk context)
class GpuChunkIndex: NoCopy, public IndexProcessor
{
  zc_ctx * ctx;
  std::vector< zc_seed > seeds;

public:
  /// flags: ZC_FLAG_SHA1 (the default) is what zbackup needs -- the instruction
  /// stream carries whole ChunkIds (backup_creator.cc:127-141,231-234).
  /// metaDir: the repository's chunk-metadata directory (GpuChunkMetaSidecar),
  /// or "" to seed the ids alone
  GpuChunkIndex( Config const & config, ChunkIndex & chunkIndex, int device, uint32_t flags = ZC_FLAG_SHA1,
                 std::string const & metaDir = std::string() ):
    ctx( 0 )
  {
    zcCheck( zc_create( &ctx, config.GET_STORABLE( chunk, max_size ), device, flags ), 0, "zc_create" );
    // the feed window's buffers (pinned host mirror + HBM, ~0.3 s to pin 1 GiB)
    // are made on a helper thread while the index loads
    zcCheck( zc_set_window( ctx, zc_get_window( ctx ) ), ctx, "zc_set_window" );
    chunkIndex.loadIndex( *this );  // every chunk id of every index file -> processChunk
    std::vector< zc_chunk_meta > meta;
    if ( !metaDir.empty() )
      GpuChunkMetaSidecar::readDir( metaDir, meta );
    if ( meta.empty() )
      zcCheck( zc_seed_index( ctx, seeds.data(), seeds.size() ), ctx, "zc_seed_index" );
    else
      zcCheck( zc_seed_index_meta( ctx, seeds.data(), seeds.size(), meta.data(), meta.size() ), ctx,
               "zc_seed_index_meta" );
    std::vector< zc_seed >().swap( seeds );
  }
  ~GpuChunkIndex() { zc_destroy( ctx ); }
  zc_ctx * context() { return ctx; }

  /// after chunkStorageWriter.commit() (zutils.cc:175): the metadata of the
  /// chunks this backup wrote, as a new file of metaDir
  std::string saveChunkMeta( std::string const & metaDir ) { return GpuChunkMetaSidecar::write( metaDir, ctx ); }

  // IndexProcessor (chunk_index.hh:47-55)
  void startIndex( string const & ) {}
  void startBundle( Bundle::Id const & ) {}
  void processChunk( ChunkId const & id, uint32_t size )
  {
    zc_seed s;
    memcpy( s.sha1, id.cryptoHash, sizeof( s.sha1 ) );
    s.rolling = id.rollingHash;
    s.size = size;
    s.reserved = 0;
    seeds.push_back( s );
  }
  void finishBundle( Bundle::Id const &, BundleInfo const & ) {}
  void finishIndex( string const & ) {}
};

/// BackupCreator's interface (backup_creator.hh:73-89) over libzchunk
class GpuBackupCreator: NoCopy
{
  zc_ctx * ctx;
  ChunkStorage::Writer & chunkStorageWriter;
  string backupData;
  sptr< google::protobuf::io::StringOutputStream > backupDataStream;
  std::vector< zc_record > records;
  string bytes;

  void take( zc_record const & r )
  {
    BackupInstruction instr;
    if ( r.kind == ZC_BYTES )  // backup_creator.cc:114-121
    {
      bytes.resize( r.size );
      zcCheck( zc_read_stream( ctx, r.offset, r.size, &bytes[ 0 ] ), ctx, "zc_read_stream" );
      instr.set_bytes_to_emit( bytes );
    }
    else
    {
      ChunkId id;
      memcpy( id.cryptoHash, r.sha1, sizeof( id.cryptoHash ) );
      id.rollingHash = r.rolling;
      if ( r.kind == ZC_CHUNK_NEW )  // saveChunkToSave: backup_creator.cc:124-139
      {
        // the chunk's bytes straight from the feed window's host mirror (no
        // copy); a device-resident stream's are copied out
        void const * data = zc_stream_data( ctx, r.offset, r.size );
        if ( !data )
        {
          bytes.resize( r.size );
          zcCheck( zc_read_stream( ctx, r.offset, r.size, &bytes[ 0 ] ), ctx, "zc_read_stream" );
          data = bytes.data();
        }
        chunkStorageWriter.add( id, data, r.size );
      }
      instr.set_chunk_to_emit( id.toBlob() );
    }
    Message::serialize( instr, *backupDataStream );  // outputInstruction: backup_creator.cc:267-273
  }

  // the records cut so far, in stream order; their bytes are readable until
  // the next feed call
  void drain()
  {
    for ( ; ; )
    {
      records.resize( 4096 );
      size_t got = 0;
      zcCheck( zc_take_records( ctx, records.data(), records.size(), &got ), ctx, "zc_take_records" );
      for ( size_t i = 0; i < got; ++i )
        take( records[ i ] );
      if ( got < records.size() )
        break;
    }
  }

public:
  GpuBackupCreator( GpuChunkIndex & index, ChunkStorage::Writer & writer ):
    ctx( index.context() ), chunkStorageWriter( writer ),
    backupDataStream( new google::protobuf::io::StringOutputStream( &backupData ) )
  {
    zcCheck( zc_reset( ctx ), ctx, "zc_reset" );  // a new stream on the shared index
  }

  void * getInputBuffer()  // backup_creator.cc:40-43
  {
    void * p = zc_get_input_buffer( ctx );
    if ( !p )
      zcCheck( ZC_ERR_STATE, ctx, "getInputBuffer" );
    return p;
  }

  size_t getInputBufferSize()  // backup_creator.cc:45-54
  {
    size_t n = zc_get_input_buffer_size( ctx );
    if ( !n )
      zcCheck( ZC_ERR_STATE, ctx, "getInputBufferSize" );
    return n;
  }

  void handleMoreData( unsigned added )  // backup_creator.cc:56-108
  {
    zcCheck( zc_handle_more_data( ctx, added ), ctx, "handleMoreData" );
    drain();
  }

  void finish()  // backup_creator.cc:147-172
  {
    zcCheck( zc_finish( ctx ), ctx, "finish" );
    drain();
  }

  void getBackupData( string & str )  // backup_creator.cc:275-280
  {
    if ( !backupDataStream.get() )
      throw std::logic_error( "getBackupData() called twice" );
    backupDataStream.reset();
    str.swap( backupData );
  }
};

/// backupFromFileHandle (zutils.cc:89-182) for data that already lies in HBM,
/// with the backup data kept there through the shrink loop (zutils.cc:137-166):
/// every pass is zc_chunk_device on the buffer the pass before wrote with
/// zc_serialize_records_device, on GpuChunkIndex's context, so a pass matches
/// the chunks the passes before it added.  Per pass the host sees the records;
/// the NEW chunks' bytes are gathered on the device (zc_bundle_gather) and read
/// once, for Writer::add; no bytes_to_emit payload and no intermediate stream
/// comes to the host, and only the final stream is read back.  The whole-stream
/// SHA-256 stays with the caller, who has the data (zc_sha256_*).
///
///   GpuDeviceBackup deviceBackup( gpuIndex, chunkStorageWriter );
///   deviceBackup.backup( d_data, n, info );   // backup_data, iterations, size
///   info.set_sha256( ... ); chunkStorageWriter.commit(); ...
class GpuDeviceBackup: NoCopy
{
  zc_ctx * ctx;
  ChunkStorage::Writer & chunkStorageWriter;

  // a device buffer of this call
  struct Buffer: NoCopy
  {
    zc_ctx * ctx;
    void * p;
    uint64_t size;
    explicit Buffer( zc_ctx * c ): ctx( c ), p( 0 ), size( 0 ) {}
    void make( uint64_t bytes )
    {
      drop();
      zcCheck( zc_device_alloc( ctx, bytes, &p ), ctx, "zc_device_alloc" );
      size = bytes;
    }
    void drop()
    {
      if ( p )
        zc_device_free( ctx, p );
      p = 0;
      size = 0;
    }
    void swap( Buffer & other )
    {
      std::swap( p, other.p );
      std::swap( size, other.size );
    }
    ~Buffer() { drop(); }
  };

  // n device bytes to the host, one read through the range reader's staging buffer
  void download( void const * d, uint64_t n, string & out )
  {
    out.resize( n );
    if ( !n )
      return;
    zc_range_index * one = 0;
    uint32_t slot = 0;
    uint64_t zero = 0;
    zcCheck( zc_range_index_create( ctx, &n, 1, &slot, &zero, &n, 1, &one ), ctx, "zc_range_index_create" );
    int rc = zc_range_set_slot( one, 0, d );
    if ( rc == ZC_OK )
      rc = zc_range_read_host( ctx, one, &zero, &n, 1, &out[ 0 ], &zero );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    zc_range_index_destroy( one );
    if ( rc != ZC_OK )
      throw std::runtime_error( "GpuDeviceBackup: reading from the device: " + err );
  }

  // One BackupCreator's life on the stream [d, d + n): the records, Writer::add
  // for every NEW chunk (saveChunkToSave, backup_creator.cc:124-139), the
  // instruction stream into `out`
  void pass( void const * d, uint64_t n, Buffer & out )
  {
    zcCheck( zc_reset( ctx ), ctx, "zc_reset" );  // a new stream on the shared index
    zcCheck( zc_chunk_device( ctx, d, n ), ctx, "zc_chunk_device" );
    std::vector< zc_record > records( zc_record_count( ctx ) + 1 );
    size_t count = 0;
    zcCheck( zc_get_records( ctx, records.data(), records.size(), &count ), ctx, "zc_get_records" );
    std::vector< uint64_t > off, size;
    uint64_t total = 0;
    for ( size_t i = 0; i < count; ++i )
      if ( records[ i ].kind == ZC_CHUNK_NEW )
      {
        off.push_back( records[ i ].offset );
        size.push_back( records[ i ].size );
        total += records[ i ].size;
      }
    if ( !off.empty() )
    {
      Buffer payload( ctx );
      payload.make( total );
      zcCheck( zc_bundle_gather( ctx, d, off.data(), size.data(), off.size(), payload.p ), ctx, "zc_bundle_gather" );
      string bytes;
      download( payload.p, total, bytes );
      uint64_t at = 0;
      for ( size_t i = 0; i < count; ++i )
        if ( records[ i ].kind == ZC_CHUNK_NEW )
        {
          ChunkId id;
          memcpy( id.cryptoHash, records[ i ].sha1, sizeof( id.cryptoHash ) );
          id.rollingHash = records[ i ].rolling;
          chunkStorageWriter.add( id, bytes.data() + at, records[ i ].size );
          at += records[ i ].size;
        }
    }
    uint64_t need = 0, wrote = 0;
    if ( zc_serialized_size( records.data(), count, &need ) != ZC_OK )
      throw std::runtime_error( string( "zc_serialized_size: " ) + zc_last_error( 0 ) );
    out.make( need );
    zcCheck( zc_serialize_records_device( ctx, records.data(), count, n ? d : 0, n, out.p, need, &wrote ), ctx,
             "zc_serialize_records_device" );
  }

public:
  GpuDeviceBackup( GpuChunkIndex & index, ChunkStorage::Writer & writer ):
    ctx( index.context() ), chunkStorageWriter( writer ) {}

  /// d_data: n bytes in device memory, 16-byte aligned (zc_chunk_device).
  /// BackupInfoT: zbackup's BackupInfo, or anything with set_size,
  /// iterations / set_iterations and mutable_backup_data.
  template< class BackupInfoT >
  void backup( void const * d_data, uint64_t n, BackupInfoT & info )
  {
    Buffer serialized( ctx ), newGen( ctx );
    pass( d_data, n, serialized );
    info.set_size( n );
    // Shrink the serialized data iteratively until it wouldn't shrink anymore
    for ( ; ; )
    {
      pass( serialized.p, serialized.size, newGen );
      if ( newGen.size < serialized.size )
      {
        serialized.swap( newGen );  // the pass is complete: nothing reads the older generation again
        newGen.drop();
        info.set_iterations( info.iterations() + 1 );
      }
      else
        break;
    }
    download( serialized.p, serialized.size, *info.mutable_backup_data() );
    zcCheck( zc_reset( ctx ), ctx, "zc_reset" );  // the context refers to no buffer of this call
  }
};

/// lzo1x_1 of finished bundles on the GPU, for Bundle::Creator::write
/// (bundle.cc:96-155) when the selected compression is "lzo1x_1": the framed
/// bytes equal what LZO1X_1_Encoder writes (compression.cc:435-466, 586-606),
/// so the encoder loop there becomes
///
///   string framed;
///   gpuLzo.compress( payload, framed );    // one payload, or compressAll for a batch
///   os.write( framed.data(), framed.size() );
///
/// (EncryptedFile::OutputStream::write, as bundle.cc:84 uses it), followed by the
/// os.writeAdler32() the reference already does.
///
/// Bundle::Creator::write runs on detached compressor threads, several at a time
/// (chunk_storage.cc:133-141,175), while the main thread feeds the backup stream
/// through GpuChunkIndex's context.  So this class never touches that context:
/// it keeps a pool of contexts of its own, one per compressor thread that is
/// inside compress() at the moment (made on first need, reused after), and each
/// call runs on a context no other thread is using.  (libzchunk also serializes
/// the calls on one context with a per-context lock, so sharing one would be
/// safe, only not concurrent.)
class GpuLzoBundleCompressor: NoCopy
{
  int device;
  std::mutex poolMutex;
  std::vector< zc_ctx * > idle, all;

  zc_ctx * acquire()
  {
    std::lock_guard< std::mutex > lock( poolMutex );
    if ( !idle.empty() )
    {
      zc_ctx * c = idle.back();
      idle.pop_back();
      return c;
    }
    zc_ctx * c = 0;
    zcCheck( zc_create( &c, 65536, device, 0 ), 0, "zc_create" );
    all.push_back( c );
    return c;
  }

  void release( zc_ctx * c )
  {
    std::lock_guard< std::mutex > lock( poolMutex );
    idle.push_back( c );
  }

public:
  explicit GpuLzoBundleCompressor( int device_ = 0 ): device( device_ ) {}
  ~GpuLzoBundleCompressor()
  {
    for ( size_t i = 0; i < all.size(); ++i )
      zc_destroy( all[ i ] );
  }

  void compress( string const & payload, string & framed )
  {
    std::vector< string const * > one( 1, &payload );
    std::vector< string > out;
    compressAll( one, out );
    framed.swap( out[ 0 ] );
  }

  /// several finished bundles in one device call (Writer::finishCurrentBundle
  /// can queue them instead of starting a compressor thread per bundle)
  void compressAll( std::vector< string const * > const & payloads, std::vector< string > & framed )
  {
    size_t n = payloads.size();
    std::vector< uint64_t > payOff( n ), paySize( n ), outOff( n ), outSize( n );
    string in, out;
    uint64_t inPos = 0, outPos = 0;
    for ( size_t i = 0; i < n; ++i )
    {
      payOff[ i ] = inPos;
      paySize[ i ] = payloads[ i ]->size();
      inPos += paySize[ i ];
      outOff[ i ] = outPos;
      outPos += zc_lzo_capacity( paySize[ i ] );
    }
    in.reserve( inPos );
    for ( size_t i = 0; i < n; ++i )
      in += *payloads[ i ];
    out.resize( outPos ? outPos : 1 );
    zc_ctx * ctx = acquire();
    int rc = zc_lzo_compress_host( ctx, in.data(), payOff.data(), paySize.data(), n, &out[ 0 ], outOff.data(),
                                   outSize.data() );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    release( ctx );
    if ( rc != ZC_OK )
      throw std::runtime_error( "zc_lzo_compress_host: " + err );
    framed.resize( n );
    for ( size_t i = 0; i < n; ++i )
      framed[ i ].assign( out, outOff[ i ], outSize[ i ] );
  }
};

/// Contexts for calls that come from several threads at once: one per thread
/// that is inside a call at the moment, made on first need and reused after
/// (what GpuLzoBundleCompressor keeps for itself, shared by the two classes below).
class ZcContextPool: NoCopy
{
  int device;
  std::mutex poolMutex;
  std::vector< zc_ctx * > idle, all;

public:
  explicit ZcContextPool( int device_ ): device( device_ ) {}
  ~ZcContextPool()
  {
    for ( size_t i = 0; i < all.size(); ++i )
      zc_destroy( all[ i ] );
  }

  zc_ctx * acquire()
  {
    std::lock_guard< std::mutex > lock( poolMutex );
    if ( !idle.empty() )
    {
      zc_ctx * c = idle.back();
      idle.pop_back();
      return c;
    }
    zc_ctx * c = 0;
    zcCheck( zc_create( &c, 65536, device, 0 ), 0, "zc_create" );
    all.push_back( c );
    return c;
  }

  void release( zc_ctx * c )
  {
    std::lock_guard< std::mutex > lock( poolMutex );
    idle.push_back( c );
  }
};

/// The bundle FILE on the GPU, for Bundle::Creator::write (bundle.cc:96-155) in a
/// repository with or without a password: what EncryptedFile::OutputStream makes
/// of the bytes written through it (encrypted_file.cc:239-392) -- the random
/// first block, both Adler-32s, PKCS#7 padding, AES-128-CBC from the zero IV
/// under EncryptionKey::getKey().  write() serializes the two messages as it
/// does today, but into a string, and hands the rest over:
///
///   string prefix, file;
///   if ( key.hasKey() ) prefix.assign( randomBlock, 16 );  // Random::genaratePseudo, as writeRandomIv does
///   { StringOutputStream s( &prefix ); CodedOutputStream c( &s );
///     Message::serialize( header, c ); Message::serialize( info, c ); }
///   sealer.seal( prefix, framed, file );   // framed: GpuLzoBundleCompressor's output
///   UnbufferedFile( fileName, UnbufferedFile::WriteOnly ).write( file.data(), file.size() );
///
/// The key stays inside this process: it goes to the device as eleven round keys
/// in a kernel's arguments, never to a file.
class GpuBundleSealer: NoCopy
{
  ZcContextPool pool;
  bool keyed;
  uint8_t key[ 16 ];

public:
  explicit GpuBundleSealer( EncryptionKey const & encryptionKey, int device = 0 ):
    pool( device ), keyed( encryptionKey.hasKey() )
  {
    memset( key, 0, sizeof( key ) );
    if ( keyed )
      memcpy( key, encryptionKey.getKey(), sizeof( key ) );
  }

  bool hasKey() const { return keyed; }

  void seal( string const & prefix, string const & body, string & file )
  {
    std::vector< string const * > p( 1, &prefix ), b( 1, &body );
    std::vector< string > out;
    sealAll( p, b, out );
    file.swap( out[ 0 ] );
  }

  /// several finished bundles in one device call
  void sealAll( std::vector< string const * > const & prefixes, std::vector< string const * > const & bodies,
                std::vector< string > & files )
  {
    size_t n = prefixes.size();
    if ( bodies.size() != n )
      throw std::logic_error( "GpuBundleSealer: prefixes and bodies differ in number" );
    std::vector< zc_bundle_file > desc( n );
    std::vector< uint64_t > fileSize( n );
    string prefixBlob, bodyBlob, out;
    uint64_t filePos = 0;
    for ( size_t i = 0; i < n; ++i )
    {
      desc[ i ].prefix_off = prefixBlob.size();
      desc[ i ].prefix_len = prefixes[ i ]->size();
      desc[ i ].body_off = bodyBlob.size();
      desc[ i ].body_len = bodies[ i ]->size();
      desc[ i ].file_off = filePos;
      prefixBlob += *prefixes[ i ];
      bodyBlob += *bodies[ i ];
      uint64_t size = zc_bundle_file_size( desc[ i ].prefix_len, desc[ i ].body_len, keyed );
      filePos += ( size + 15 ) / 16 * 16;
    }
    out.resize( filePos ? filePos : 1 );
    zc_ctx * ctx = pool.acquire();
    int rc = zc_bundle_seal_host( ctx, keyed ? key : 0, prefixBlob.data(), desc.data(), n, bodyBlob.data(),
                                  &out[ 0 ], fileSize.data() );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    pool.release( ctx );
    if ( rc != ZC_OK )
      throw std::runtime_error( err );
    files.resize( n );
    for ( size_t i = 0; i < n; ++i )
      files[ i ].assign( out, desc[ i ].file_off, fileSize[ i ] );
  }
};

/// The read side, in front of Bundle::Reader (bundle.cc:157-218): the file's
/// bytes go in (UnbufferedFile::read of the whole file), the two serialized
/// messages and the compressed body come out, decrypted and with both Adler-32s
/// and the padding checked on the GPU.  Reader parses the messages from strings
/// (ArrayInputStream + Message::parse) and feeds `body` to its decoder as before.
/// A file the reference would refuse throws here, under the name the reference
/// throws (exIncorrectFileSize, exBadPadding, exAdlerMismatch, or a parse error).
class GpuBundleUnsealer: NoCopy
{
  ZcContextPool pool;
  bool keyed;
  uint8_t key[ 16 ];

public:
  struct Opened
  {
    string header, info, body;  // BundleFileHeader and BundleInfo (serialized), the compressed body
  };

  explicit GpuBundleUnsealer( EncryptionKey const & encryptionKey, int device = 0 ):
    pool( device ), keyed( encryptionKey.hasKey() )
  {
    memset( key, 0, sizeof( key ) );
    if ( keyed )
      memcpy( key, encryptionKey.getKey(), sizeof( key ) );
  }

  static char const * statusName( int status )
  {
    switch ( status )
    {
      case ZC_BUNDLE_OK: return "ok";
      case ZC_BUNDLE_BAD_SIZE: return "exIncorrectFileSize";
      case ZC_BUNDLE_TRUNCATED: return "the file ends inside its header (Message::parse fails)";
      case ZC_BUNDLE_BAD_ADLER1: return "exAdlerMismatch after BundleInfo";
      case ZC_BUNDLE_BAD_ADLER2: return "exAdlerMismatch after the payload";
      case ZC_BUNDLE_BAD_PADDING: return "exBadPadding";
      default: return "unknown status";
    }
  }

  void unseal( string const & file, Opened & opened )
  {
    std::vector< string const * > f( 1, &file );
    std::vector< Opened > out;
    std::vector< int > status;
    unsealAll( f, out, status );
    if ( status[ 0 ] != ZC_BUNDLE_OK )
      throw std::runtime_error( string( "bundle file: " ) + statusName( status[ 0 ] ) );
    opened.header.swap( out[ 0 ].header );
    opened.info.swap( out[ 0 ].info );
    opened.body.swap( out[ 0 ].body );
  }

  /// several files in one device call (a restore knows the bundles it needs
  /// up front); status[ i ] != ZC_BUNDLE_OK leaves opened[ i ] empty
  void unsealAll( std::vector< string const * > const & files, std::vector< Opened > & opened,
                  std::vector< int > & status )
  {
    size_t n = files.size();
    std::vector< uint64_t > off( n ), size( n );
    std::vector< zc_bundle_layout > layout( n );
    string in, plain;
    for ( size_t i = 0; i < n; ++i )
    {
      off[ i ] = in.size();
      size[ i ] = files[ i ]->size();
      in += *files[ i ];
      in.resize( ( in.size() + 15 ) / 16 * 16 );  // every file at a 16-byte offset
    }
    if ( in.empty() )
      in.resize( 16 );
    plain.resize( in.size() );
    zc_ctx * ctx = pool.acquire();
    int rc = zc_bundle_unseal_host( ctx, keyed ? key : 0, in.data(), off.data(), size.data(), n, &plain[ 0 ],
                                    off.data(), layout.data() );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    pool.release( ctx );
    if ( rc != ZC_OK )
      throw std::runtime_error( err );
    opened.assign( n, Opened() );
    status.resize( n );
    for ( size_t i = 0; i < n; ++i )
    {
      status[ i ] = layout[ i ].status;
      if ( status[ i ] != ZC_BUNDLE_OK )
        continue;
      opened[ i ].header.assign( plain, off[ i ] + layout[ i ].header_off, layout[ i ].header_len );
      opened[ i ].info.assign( plain, off[ i ] + layout[ i ].info_off, layout[ i ].info_len );
      opened[ i ].body.assign( plain, off[ i ] + layout[ i ].body_off, layout[ i ].body_len );
    }
  }
};

/// LZMA bundles (the default compression method) decoded on the GPU, behind
/// GpuBundleUnsealer: the bodies it yields are the xz streams LZMADecoder
/// (compression.cc:99-107) reads under Bundle::Reader (bundle.cc:179-216), and
/// BundleInfo gives each payload's size (the sum of its chunk sizes).  decodeAll
/// returns the payloads as Reader's `payload` strings; decodeToDevice leaves
/// them in a device buffer, back to back at 16-byte aligned offsets, for
/// callers that go on with zc_bundle_scatter, zc_range_set_slot or
/// zc_chunk_meta_compute.  A body that is not exactly its payload -- a stream
/// error, bytes behind the stream's end (where the reference's Adler-32 check
/// fails), another size than BundleInfo's -- throws, naming the bundle.
class GpuXzBundleDecoder: NoCopy
{
  ZcContextPool pool;

  static void judge( size_t n, zc_xz_result const * res, std::vector< string const * > const & bodies,
                     std::vector< uint64_t > const & sizes )
  {
    for ( size_t i = 0; i < n; ++i )
    {
      char msg[ 160 ];
      if ( res[ i ].status != ZC_XZ_OK )
        snprintf( msg, sizeof( msg ), "bundle %zu: xz status %d after %llu bytes", i, (int) res[ i ].status,
                  (unsigned long long) res[ i ].decoded );
      else if ( res[ i ].consumed != bodies[ i ]->size() )
        snprintf( msg, sizeof( msg ), "bundle %zu: the stream ends after %llu of the body's %zu bytes", i,
                  (unsigned long long) res[ i ].consumed, bodies[ i ]->size() );
      else if ( res[ i ].decoded != sizes[ i ] )
        snprintf( msg, sizeof( msg ), "bundle %zu: %llu bytes decoded, its payload has %llu", i,
                  (unsigned long long) res[ i ].decoded, (unsigned long long) sizes[ i ] );
      else
        continue;
      throw std::runtime_error( msg );
    }
  }

  static void layout( std::vector< string const * > const & bodies, std::vector< uint64_t > const & sizes,
                      string & in, std::vector< uint64_t > & inOff, std::vector< uint64_t > & inSize,
                      std::vector< uint64_t > & outOff, uint64_t & outBytes )
  {
    size_t n = bodies.size();
    if ( sizes.size() != n )
      throw std::logic_error( "GpuXzBundleDecoder: bodies and sizes differ in number" );
    inOff.resize( n );
    inSize.resize( n );
    outOff.resize( n );
    outBytes = 0;
    for ( size_t i = 0; i < n; ++i )
    {
      inOff[ i ] = in.size();
      inSize[ i ] = bodies[ i ]->size();
      in += *bodies[ i ];
      in.resize( ( in.size() + 15 ) / 16 * 16 );
      outOff[ i ] = outBytes;
      outBytes += ( sizes[ i ] + 15 ) / 16 * 16;
    }
  }

public:
  /// Payloads in device memory: payload i is `sizes[ i ]` bytes at `data + offsets[ i ]`.
  /// The buffer belongs to this object and goes with it; it must not outlive
  /// the decoder that filled it (it holds one of the decoder's contexts).
  struct DevicePayloads: NoCopy
  {
    zc_ctx * ctx;
    ZcContextPool * pool;
    char * data;
    uint64_t bytes;  // the payloads' extent: offsets[ i ] + sizes[ i ] <= bytes
    std::vector< uint64_t > offsets, sizes;
    DevicePayloads(): ctx( 0 ), pool( 0 ), data( 0 ), bytes( 0 ) {}
    ~DevicePayloads()
    {
      if ( ctx )
      {
        zc_device_free( ctx, data );
        pool->release( ctx );
      }
    }
  };

  explicit GpuXzBundleDecoder( int device = 0 ): pool( device ) {}

  void decode( string const & body, uint64_t size, string & payload )
  {
    std::vector< string const * > b( 1, &body );
    std::vector< uint64_t > s( 1, size );
    std::vector< string > out;
    decodeAll( b, s, out );
    payload.swap( out[ 0 ] );
  }

  /// several bundles in one device call, the payloads back on the host
  void decodeAll( std::vector< string const * > const & bodies, std::vector< uint64_t > const & sizes,
                  std::vector< string > & payloads )
  {
    string in, out;
    std::vector< uint64_t > inOff, inSize, outOff;
    uint64_t outBytes;
    layout( bodies, sizes, in, inOff, inSize, outOff, outBytes );
    size_t n = bodies.size();
    std::vector< zc_xz_result > res( n ? n : 1 );
    if ( in.empty() )
      in.resize( 16 );
    out.resize( outBytes ? outBytes : 1 );
    zc_ctx * ctx = pool.acquire();
    int rc = zc_xz_decode_host( ctx, in.data(), inOff.data(), inSize.data(), n, &out[ 0 ], outOff.data(),
                                sizes.data(), res.data() );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    pool.release( ctx );
    if ( rc != ZC_OK )
      throw std::runtime_error( err );
    judge( n, res.data(), bodies, sizes );
    payloads.resize( n );
    for ( size_t i = 0; i < n; ++i )
      payloads[ i ].assign( out, outOff[ i ], sizes[ i ] );
  }

  /// the same with the payloads left in HBM: only the compressed bodies cross
  void decodeToDevice( std::vector< string const * > const & bodies, std::vector< uint64_t > const & sizes,
                       DevicePayloads & dev )
  {
    if ( dev.ctx )
      throw std::logic_error( "GpuXzBundleDecoder: DevicePayloads is in use" );
    string in;
    std::vector< uint64_t > inOff, inSize, outOff;
    uint64_t outBytes;
    layout( bodies, sizes, in, inOff, inSize, outOff, outBytes );
    size_t n = bodies.size();
    std::vector< zc_xz_result > res( n ? n : 1 );
    zc_ctx * ctx = pool.acquire();
    void * buf = 0;
    int rc = zc_device_alloc( ctx, outBytes + in.size(), &buf );
    if ( rc == ZC_OK )
      rc = zc_upload( ctx, (char *) buf + outBytes, in.data(), in.size() );
    if ( rc == ZC_OK )
      rc = zc_xz_decode( ctx, (char *) buf + outBytes, inOff.data(), inSize.data(), n, buf, outOff.data(),
                         sizes.data(), res.data() );
    if ( rc != ZC_OK )
    {
      string err = zc_last_error( ctx );
      zc_device_free( ctx, buf );
      pool.release( ctx );
      throw std::runtime_error( err );
    }
    dev.ctx = ctx;  // from here on the buffer and the context go with dev
    dev.pool = &pool;
    dev.data = (char *) buf;
    dev.bytes = outBytes;
    dev.offsets = outOff;
    dev.sizes = sizes;
    judge( n, res.data(), bodies, sizes );
  }
};

/// LZMA bundles (the default compression method) written on the GPU: the
/// counterpart of GpuLzoBundleCompressor for compression_method == "lzma", with
/// the same interface.  Bundle::Creator::write (bundle.cc:96-155) hands its
/// payload to LZMAEncoder (compression.cc:78-97); with this class that becomes
///
///   string body;
///   gpuXz.compress( payload, body );    // one payload, or compressAll for a batch
///   os.write( body.data(), body.size() );
///
/// The body is an xz stream (one block, LZMA2, CRC64) that lzma_stream_decoder
/// and GpuXzBundleDecoder read back to the payload; it is not liblzma's bytes
/// (another match finder and parse), and it is a function of the payload alone.
/// A batch pays: the device codes a bundle per wave, some two thousand at once.
/// Contexts come from a pool, as GpuLzoBundleCompressor's do, so compressor
/// threads may call at the same time.
class GpuXzBundleCompressor: NoCopy
{
  ZcContextPool pool;
  uint32_t check;

public:
  /// check: 4 (CRC64, what zbackup writes), 1 (CRC32) or 0 (none)
  explicit GpuXzBundleCompressor( int device = 0, uint32_t check_ = 4 ): pool( device ), check( check_ ) {}

  void compress( string const & payload, string & body )
  {
    std::vector< string const * > one( 1, &payload );
    std::vector< string > out;
    compressAll( one, out );
    body.swap( out[ 0 ] );
  }

  /// several finished bundles in one device call
  void compressAll( std::vector< string const * > const & payloads, std::vector< string > & bodies )
  {
    size_t n = payloads.size();
    std::vector< uint64_t > payOff( n ), paySize( n ), outOff( n ), outCap( n );
    std::vector< zc_xz_enc_result > res( n ? n : 1 );
    string in, out;
    uint64_t inPos = 0, outPos = 0;
    for ( size_t i = 0; i < n; ++i )
    {
      payOff[ i ] = inPos;
      paySize[ i ] = payloads[ i ]->size();
      inPos += paySize[ i ];
      outOff[ i ] = outPos;
      outCap[ i ] = zc_xz_capacity( paySize[ i ] );
      outPos += ( outCap[ i ] + 15 ) / 16 * 16;
    }
    in.reserve( inPos ? inPos : 1 );
    for ( size_t i = 0; i < n; ++i )
      in += *payloads[ i ];
    if ( in.empty() )
      in.resize( 1 );
    out.resize( outPos ? outPos : 1 );
    zc_ctx * ctx = pool.acquire();
    int rc = zc_xz_encode_host( ctx, in.data(), payOff.data(), paySize.data(), n, &out[ 0 ], outOff.data(),
                                outCap.data(), check, res.data() );
    string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
    pool.release( ctx );
    if ( rc != ZC_OK )
      throw std::runtime_error( "zc_xz_encode_host: " + err );
    bodies.resize( n );
    for ( size_t i = 0; i < n; ++i )
    {
      if ( res[ i ].status != ZC_XZ_OK )  // never with zc_xz_capacity's room
      {
        char msg[ 96 ];
        snprintf( msg, sizeof( msg ), "bundle %zu: xz status %d from the encoder", i, (int) res[ i ].status );
        throw std::runtime_error( msg );
      }
      bodies[ i ].assign( out, outOff[ i ], res[ i ].size );
    }
  }
};

/// Adopting a repository stock zbackup wrote: its chunks are known by id only,
/// and ids alone go through the exact screen at every byte.  This computes the
/// chunk metadata (zc_chunk_meta) of every chunk of the bundles handed to it
/// from their decoded payloads -- Bundle::Reader's, bundle.cc:157-251 -- and
/// compares each recomputed ChunkId with the one BundleInfo claims, a check of
/// the bundles zbackup itself does not have.  Payloads are collected and go
/// through zc_chunk_meta_compute_host every 256 MiB; finish() writes the records
/// of the chunks that are chunk.max_size bytes and whose id holds as one
/// GpuChunkMetaSidecar file, which GpuChunkIndex picks up on the next open.
class GpuRepositoryAdopter: NoCopy
{
public:
  struct Mismatch
  {
    Bundle::Id bundle;
    uint32_t chunk;   // index in the bundle's BundleInfo
    uint8_t status;   // ZC_META_BAD_* bits
  };

private:
  zc_ctx * ctx;
  uint32_t maxSize;
  std::string payloads;
  std::vector< uint64_t > off;
  std::vector< uint32_t > size, chunkOf;
  std::vector< zc_seed > expect;
  std::vector< Bundle::Id > bundleOf;
  std::vector< zc_chunk_meta > meta;
  std::vector< Mismatch > bad;
  uint64_t chunks, bytes;

  /// the pending chunks' results into `bad` and `meta`
  void fold( std::vector< zc_chunk_meta > const & out, std::vector< uint8_t > const & status )
  {
    for ( size_t i = 0; i < out.size(); ++i )
      if ( status[ i ] )
      {
        Mismatch m = { bundleOf[ i ], chunkOf[ i ], status[ i ] };
        bad.push_back( m );
      }
      else if ( out[ i ].size == maxSize )
        meta.push_back( out[ i ] );
  }

  /// the chunk records of one bundle whose payload starts at `pos` of the
  /// buffer they will be hashed in; returns the sum of their sizes
  template< class Info >
  uint64_t pushRecords( Bundle::Id const & id, Info const & info, uint64_t pos )
  {
    uint64_t total = 0;
    for ( int i = 0; i < info.chunk_record_size(); ++i )
    {
      std::string const & blob = info.chunk_record( i ).id();
      if ( blob.size() != 24 )
      {
        popRecords( (size_t)i );
        throw std::runtime_error( "adopt: a chunk id that is not 24 bytes" );
      }
      zc_seed s;
      memcpy( s.sha1, blob.data(), 16 );
      memcpy( &s.rolling, blob.data() + 16, 8 );  // ChunkId::setFromBlob, chunk_id.cc:29-38 (little-endian host)
      s.size = info.chunk_record( i ).size();
      s.reserved = 0;
      off.push_back( pos + total );
      size.push_back( s.size );
      chunkOf.push_back( (uint32_t)i );
      expect.push_back( s );
      bundleOf.push_back( id );
      total += s.size;
    }
    return total;
  }

  void popRecords( size_t n )
  {
    off.resize( off.size() - n );
    size.resize( size.size() - n );
    chunkOf.resize( chunkOf.size() - n );
    expect.resize( expect.size() - n );
    bundleOf.resize( bundleOf.size() - n );
  }

  void flush()
  {
    if ( off.empty() )
      return;
    std::vector< zc_chunk_meta > out( off.size() );
    std::vector< uint8_t > status( off.size() );
    size_t nBad = 0;
    zcCheck( zc_chunk_meta_compute_host( ctx, payloads.data(), payloads.size(), off.data(), size.data(), off.size(),
                                         expect.data(), out.data(), status.data(), &nBad ),
             ctx, "zc_chunk_meta_compute_host" );
    fold( out, status );
    payloads.clear();
    off.clear();
    size.clear();
    chunkOf.clear();
    expect.clear();
    bundleOf.clear();
  }

public:
  enum { FlushBytes = 256 << 20 };

  GpuRepositoryAdopter( Config const & config, int device ):
    ctx( 0 ), maxSize( config.GET_STORABLE( chunk, max_size ) ), chunks( 0 ), bytes( 0 )
  {
    zcCheck( zc_create( &ctx, maxSize, device, 0 ), 0, "zc_create" );
  }
  ~GpuRepositoryAdopter() { zc_destroy( ctx ); }

  /// one bundle: its id, its BundleInfo (chunk_record( i ).id() / .size(), as
  /// Bundle::Reader reads them: bundle.cc:220-232) and its decoded payload.
  /// (A template only so that this header asks nothing more of zbackup.pb.h in
  /// translation units that do not adopt.)
  template< class Info >
  void addBundle( Bundle::Id const & id, Info const & info, std::string const & payload )
  {
    uint64_t total = pushRecords( id, info, payloads.size() );
    if ( total != payload.size() )
    {
      popRecords( (size_t)info.chunk_record_size() );
      throw std::runtime_error( "adopt: a bundle's payload is not the sum of its chunk sizes" );
    }
    payloads.append( payload );
    chunks += (uint64_t)info.chunk_record_size();
    bytes += total;
    if ( payloads.size() >= (size_t)FlushBytes )
      flush();
  }

  /// Bundles whose payloads GpuXzBundleDecoder::decodeToDevice left in HBM:
  /// bundle i is ids[ i ] / *infos[ i ] with its payload at dev.data +
  /// dev.offsets[ i ].  They are hashed where they lie, in one device call;
  /// nothing of them crosses to the host.  Everything is checked before
  /// anything is hashed: a refused call leaves nothing behind.
  template< class Info >
  void addBundlesDevice( std::vector< Bundle::Id > const & ids, std::vector< Info const * > const & infos,
                         GpuXzBundleDecoder::DevicePayloads const & dev )
  {
    if ( ids.size() != infos.size() || ids.size() != dev.sizes.size() || !dev.ctx )
      throw std::logic_error( "adopt: ids, infos and device payloads differ in number" );
    flush();  // the host payloads added before keep their place in the order
    uint64_t newChunks = 0, newBytes = 0;
    try
    {
      for ( size_t b = 0; b < ids.size(); ++b )
      {
        uint64_t total = pushRecords( ids[ b ], *infos[ b ], dev.offsets[ b ] );
        if ( total != dev.sizes[ b ] )
          throw std::runtime_error( "adopt: a bundle's payload is not the sum of its chunk sizes" );
        newChunks += (uint64_t)infos[ b ]->chunk_record_size();
        newBytes += total;
      }
    }
    catch ( ... )
    {
      popRecords( off.size() );  // after the flush above every pending record is this call's
      throw;
    }
    if ( !off.empty() )
    {
      std::vector< zc_chunk_meta > out( off.size() );
      std::vector< uint8_t > status( off.size() );
      size_t nBad = 0;
      int rc = zc_chunk_meta_compute( ctx, dev.data, dev.bytes, off.data(), size.data(), off.size(), expect.data(),
                                      out.data(), status.data(), &nBad );
      if ( rc != ZC_OK )
        popRecords( off.size() );
      zcCheck( rc, ctx, "zc_chunk_meta_compute" );
      fold( out, status );
      popRecords( off.size() );
    }
    chunks += newChunks;
    bytes += newBytes;
  }

  /// the rest through the GPU, then one sidecar file in metaDir ("" when no
  /// chunk qualified); returns every chunk whose recomputed id or size differs
  std::vector< Mismatch > finish( std::string const & metaDir, std::string * path = 0 )
  {
    flush();
    std::string p = GpuChunkMetaSidecar::write( metaDir, meta );
    if ( path )
      *path = p;
    meta.clear();
    std::vector< Mismatch > out;
    out.swap( bad );
    return out;
  }

  uint64_t chunksSeen() const { return chunks; }
  uint64_t bytesSeen() const { return bytes; }
};

/// BackupRestorer::IndexedRestorer (backup_restorer.cc:182-316, backup_restorer.hh:55-79)
/// on the GPU: size() and saveData( offset, data, size ) with the reference's
/// signatures, so `zbackup nbd` (zutils.cc:262-297) can serve a backup from it.
/// Built from the backup data, every bundle's ( chunk id blob, size ) list --
/// what Bundle::Reader reads from BundleInfo (bundle.cc:220-232) -- and a source
/// that hands over a bundle's decoded payload on demand.  The payloads a read
/// touches are made resident in HBM (zc_range_needs, zc_range_slot_upload); the
/// least recently used ones leave when the resident bytes pass `budget`.  The
/// bundles of the read being served are always admitted, so the budget bounds
/// what stays between reads; a long read is served in steps of StepBytes to
/// keep one step's bundles few.  Uses the C ABI only.
class GpuIndexedRestorer: NoCopy
{
public:
  typedef std::vector< std::pair< std::string, uint32_t > > ChunkList;  // one bundle: ( ChunkId blob, size ) in order

  /// Bundle::Reader for bundle number `bundle` of the list given: all of its chunks, back to back
  struct PayloadSource
  {
    virtual void getPayload( size_t bundle, std::string & payload ) = 0;
    virtual ~PayloadSource() {}
  };

  struct exOutOfRange: std::runtime_error
  {
    exOutOfRange(): std::runtime_error( "IndexedRestorer: the range is outside the backup" ) {}
  };

  enum { StepBytes = 4 << 20 };

private:
  struct Where
  {
    uint32_t bundle;
    uint64_t off;
    uint32_t size;
  };

  zc_ctx * ctx;
  zc_range_index * index;
  PayloadSource & source;
  uint64_t budget;
  int64_t totalSize;
  std::vector< size_t > bundleOfSlot;  // slot -> bundle number
  std::map< size_t, uint32_t > slotOfBundle;
  std::vector< uint64_t > slotSize;
  std::vector< char > pinned;  // the slot's payload is the caller's device memory (setPayloads): never evicted, outside the budget
  // the cache of resident payloads: saveData is const, as the reference's
  mutable uint64_t residentBytes, tick, fetches, evictions;
  mutable std::vector< uint64_t > lastUse;
  mutable std::vector< char > resident;

  static void check( int rc, char const * what )
  {
    if ( rc != ZC_OK )
      throw std::runtime_error( std::string( what ) + ": " + zc_last_error( 0 ) );
  }

  void evictDownTo( uint64_t room, std::vector< char > const & wanted ) const
  {
    while ( residentBytes > room )
    {
      size_t victim = resident.size();
      for ( size_t s = 0; s < resident.size(); ++s )
        if ( resident[ s ] && !pinned[ s ] && !wanted[ s ] && ( victim == resident.size() || lastUse[ s ] < lastUse[ victim ] ) )
          victim = s;
      if ( victim == resident.size() )
        return;  // only this read's own bundles are left
      check( zc_range_slot_drop( index, (uint32_t)victim ), "zc_range_slot_drop" );
      resident[ victim ] = 0;
      residentBytes -= slotSize[ victim ];
      ++evictions;
    }
  }

  void step( uint64_t offset, char * data, uint64_t size ) const
  {
    std::vector< uint32_t > slots( slotSize.size() + 1 );  // ascending
    size_t n = 0;
    check( zc_range_needs( index, &offset, &size, 1, slots.data(), slots.size(), &n ), "zc_range_needs" );
    if ( n && slots[ n - 1 ] == slotSize.size() )
      --n;  // the instruction stream's slot (the last): always resident, outside the budget
    std::vector< char > wanted( resident.size(), 0 );
    uint64_t missing = 0;
    for ( size_t i = 0; i < n; ++i )
    {
      wanted[ slots[ i ] ] = 1;
      lastUse[ slots[ i ] ] = ++tick;
      if ( !resident[ slots[ i ] ] && !pinned[ slots[ i ] ] )
        missing += slotSize[ slots[ i ] ];
    }
    evictDownTo( budget > missing ? budget - missing : 0, wanted );
    std::string payload;
    for ( size_t i = 0; i < n; ++i )
    {
      uint32_t s = slots[ i ];
      if ( resident[ s ] || pinned[ s ] )
        continue;
      source.getPayload( bundleOfSlot[ s ], payload );
      if ( payload.size() != slotSize[ s ] )
        throw std::runtime_error( "IndexedRestorer: a bundle's payload is not the sum of its chunk sizes" );
      check( zc_range_slot_upload( index, s, payload.data(), payload.size() ), "zc_range_slot_upload" );
      resident[ s ] = 1;
      residentBytes += slotSize[ s ];
      ++fetches;
    }
    uint64_t at = 0;
    zcCheck( zc_range_read_host( ctx, index, &offset, &size, 1, data, &at ), ctx, "zc_range_read_host" );
  }

public:
  GpuIndexedRestorer( std::string const & backupData, std::vector< ChunkList > const & bundles,
                      PayloadSource & source, uint64_t budget, int device = 0 ):
    ctx( 0 ), index( 0 ), source( source ), budget( budget ), totalSize( 0 ), residentBytes( 0 ), tick( 0 ),
    fetches( 0 ), evictions( 0 )
  {
    // Bundle::Reader::Reader's id -> chunk map, per bundle; an id in two bundles keeps the first
    std::map< std::string, Where > ids;
    std::vector< uint64_t > payloadSize( bundles.size(), 0 );
    for ( size_t b = 0; b < bundles.size(); ++b )
      for ( size_t i = 0; i < bundles[ b ].size(); ++i )
      {
        if ( bundles[ b ][ i ].first.size() != 24 )
          throw std::runtime_error( "IndexedRestorer: a chunk id that is not 24 bytes" );
        Where w = { (uint32_t)b, payloadSize[ b ], bundles[ b ][ i ].second };
        ids.insert( std::make_pair( bundles[ b ][ i ].first, w ) );
        payloadSize[ b ] += bundles[ b ][ i ].second;
      }
    // a count pass first (no room given: the call reports the entries it found), so the list
    // takes what the stream holds and not the two-bytes-per-entry worst case
    size_t count = 0;
    zc_parse_instructions( backupData.data(), backupData.size(), 0, 0, &count );
    std::vector< zc_instruction > ins( count + 1 );
    check( zc_parse_instructions( backupData.data(), backupData.size(), ins.data(), ins.size(), &count ),
           "zc_parse_instructions" );
    // slots: the bundles the stream names, in first-use order, then the instruction stream
    std::vector< uint32_t > slot( count );
    std::vector< uint64_t > off( count ), size( count );
    for ( size_t e = 0; e < count; ++e )
      if ( ins[ e ].kind == ZC_INSTR_CHUNK )
      {
        std::map< std::string, Where >::const_iterator it = ids.find( std::string( (char const *)ins[ e ].id, 24 ) );
        if ( it == ids.end() )
          throw std::runtime_error( "IndexedRestorer: the backup names a chunk no bundle holds" );
        std::map< size_t, uint32_t >::const_iterator known = slotOfBundle.find( it->second.bundle );
        if ( known == slotOfBundle.end() )
        {
          known = slotOfBundle.insert( std::make_pair( (size_t)it->second.bundle, (uint32_t)bundleOfSlot.size() ) ).first;
          bundleOfSlot.push_back( it->second.bundle );
          slotSize.push_back( payloadSize[ it->second.bundle ] );
        }
        slot[ e ] = known->second;
        off[ e ] = it->second.off;
        size[ e ] = it->second.size;
      }
    uint32_t instrSlot = (uint32_t)slotSize.size();
    for ( size_t e = 0; e < count; ++e )
      if ( ins[ e ].kind != ZC_INSTR_CHUNK )
      {
        slot[ e ] = instrSlot;
        off[ e ] = ins[ e ].data_off;
        size[ e ] = ins[ e ].size;
      }
    slotSize.push_back( backupData.size() );
    zcCheck( zc_create( &ctx, 65536, device, 0 ), 0, "zc_create" );
    int rc = zc_range_index_create( ctx, slotSize.data(), slotSize.size(), slot.data(), off.data(), size.data(),
                                    count, &index );
    uint64_t total = 0;
    if ( rc == ZC_OK )
      rc = zc_range_index_total( index, &total );
    if ( rc == ZC_OK )
      rc = zc_range_slot_upload( index, instrSlot, backupData.data(), backupData.size() );
    if ( rc != ZC_OK || total > (uint64_t)INT64_MAX )
    {
      std::string err = rc != ZC_OK ? std::string( zc_last_error( index ? 0 : ctx ) ) : "the backup is 2^63 bytes or more";
      if ( index )
        zc_range_index_destroy( index );
      zc_destroy( ctx );
      throw std::runtime_error( "IndexedRestorer: " + err );
    }
    totalSize = (int64_t)total;
    slotSize.pop_back();  // the instruction stream stays resident and outside the budget
    resident.assign( slotSize.size(), 0 );
    lastUse.assign( slotSize.size(), 0 );
    pinned.assign( slotSize.size(), 0 );
  }

  /// Payloads GpuXzBundleDecoder::decodeToDevice left in HBM become the slots
  /// of their bundles: payload i of `dev` is bundle number bundleNumbers[ i ] of
  /// the list given at construction.  Reads are served from them where they
  /// lie; they are never evicted and do not count against the budget, and the
  /// source is not asked for these bundles.  A bundle the backup does not name
  /// is skipped.  `dev` must stay alive until clearPayloads() or this object's
  /// end; a size that is not the bundle's throws before any slot changes.
  void setPayloads( std::vector< size_t > const & bundleNumbers, GpuXzBundleDecoder::DevicePayloads const & dev )
  {
    if ( bundleNumbers.size() != dev.sizes.size() || !dev.ctx )
      throw std::logic_error( "IndexedRestorer: bundle numbers and device payloads differ in number" );
    std::vector< std::pair< uint32_t, size_t > > todo;  // ( slot, payload in dev )
    for ( size_t i = 0; i < bundleNumbers.size(); ++i )
    {
      std::map< size_t, uint32_t >::const_iterator it = slotOfBundle.find( bundleNumbers[ i ] );
      if ( it == slotOfBundle.end() )
        continue;
      if ( dev.sizes[ i ] != slotSize[ it->second ] )
        throw std::runtime_error( "IndexedRestorer: a bundle's payload is not the sum of its chunk sizes" );
      todo.push_back( std::make_pair( it->second, i ) );
    }
    for ( size_t k = 0; k < todo.size(); ++k )
    {
      uint32_t s = todo[ k ].first;
      check( zc_range_set_slot( index, s, dev.data + dev.offsets[ todo[ k ].second ] ), "zc_range_set_slot" );
      if ( resident[ s ] )  // an uploaded copy went with the call above
      {
        resident[ s ] = 0;
        residentBytes -= slotSize[ s ];
      }
      pinned[ s ] = 1;
    }
  }

  /// the slots set by setPayloads are empty again (before their device memory goes)
  void clearPayloads()
  {
    for ( size_t s = 0; s < pinned.size(); ++s )
      if ( pinned[ s ] )
      {
        check( zc_range_set_slot( index, (uint32_t)s, 0 ), "zc_range_set_slot" );
        pinned[ s ] = 0;
      }
  }

  ~GpuIndexedRestorer()
  {
    zc_range_index_destroy( index );
    zc_destroy( ctx );
  }

  int64_t size() const { return totalSize; }

  void saveData( int64_t offset, void * data, size_t size ) const
  {
    if ( offset < 0 || (uint64_t)size > (uint64_t)totalSize || (uint64_t)offset > (uint64_t)totalSize - size )
      throw exOutOfRange();
    for ( uint64_t k = 0; k < size; k += StepBytes )
      step( (uint64_t)offset + k, (char *)data + k, size - k < (uint64_t)StepBytes ? size - k : (uint64_t)StepBytes );
  }

  uint64_t residentPayloadBytes() const { return residentBytes; }
  uint64_t payloadsFetched() const { return fetches; }
  uint64_t payloadsEvicted() const { return evictions; }
};

/// The reader side of ChunkIndex, resident in HBM: loadIndex's table
/// (chunk_index.cc:26-79,163-182) built from the index files' bytes in one
/// device pass (zc_index_load_host, zc_chunk_index_create), findChunk
/// (chunk_index.cc:119-161) for a batch of ids, and the resolve of a whole
/// backup (ChunkStorage::Reader::get for every chunk_to_emit,
/// chunk_storage.cc:214-260, with Bundle::Reader's offsets, bundle.cc:220-251)
/// in one call.  Bundles are numbered in the order loadIndex met them;
/// bundleId( n ) names the file.  A file that cannot be read contributes
/// nothing and keeps its status (fileStatus).  The write-side GpuChunkIndex
/// above is the chunker's seed table and is not touched.  Uses the C ABI only.
class GpuResidentChunkIndex: NoCopy
{
public:
  enum { NoBundle = 0xFFFFFFFFu };

  struct Found
  {
    uint32_t bundle;  // NoBundle: the index has no such chunk
    uint64_t offset;  // in the bundle's decoded payload
    uint32_t size;
  };

  /// a backup resolved: slot k is bundle used[ k ] (ascending), slot used.size() the backup data itself
  struct Plan
  {
    uint64_t length;
    std::vector< uint32_t > used;
    std::vector< uint64_t > usedSize;
    std::vector< uint32_t > slot;
    std::vector< uint64_t > off, size, dst;
  };

  struct exNoSuchChunk: std::runtime_error
  {
    explicit exNoSuchChunk( string const & what ): std::runtime_error( what ) {}
  };
  struct exDuplicateChunks: std::runtime_error
  {
    explicit exDuplicateChunks( string const & what ): std::runtime_error( what ) {}
  };

private:
  zc_ctx * ctx;
  zc_chunk_index * index;
  std::vector< string > bundleIds;
  std::vector< int > status;

  static string hex( uint8_t const * p, size_t n )
  {
    string out;
    char b[ 3 ];
    for ( size_t i = 0; i < n; ++i )
    {
      snprintf( b, sizeof b, "%02x", p[ i ] );
      out += b;
    }
    return out;
  }

public:
  /// indexFiles: the files' bytes, in the order Dir::Listing hands them to loadIndex
  GpuResidentChunkIndex( std::vector< string > const & indexFiles, EncryptionKey const & encryptionKey,
                         int device = 0 ): ctx( 0 ), index( 0 )
  {
    size_t n = indexFiles.size();
    std::vector< uint64_t > off( n ), size( n );
    string in;
    for ( size_t i = 0; i < n; ++i )
    {
      off[ i ] = in.size();
      size[ i ] = indexFiles[ i ].size();
      in += indexFiles[ i ];
      in.resize( ( in.size() + 15 ) / 16 * 16 );  // every file at a 16-byte offset
    }
    if ( in.empty() )
      in.resize( 16 );
    zcCheck( zc_create( &ctx, 65536, device, 0 ), 0, "zc_create" );
    zc_index_set * set = 0;
    uint64_t files = 0, bundles = 0, records = 0;
    int rc = zc_index_load_host( ctx, encryptionKey.hasKey() ? (uint8_t const *)encryptionKey.getKey() : 0, in.data(),
                                 off.data(), size.data(), n, &set );
    string err = rc == ZC_OK ? string() : string( "zc_index_load_host: " ) + zc_last_error( ctx );
    if ( rc == ZC_OK )
    {
      zc_index_set_counts( set, &files, &bundles, &records );
      std::vector< uint8_t > ids( 24 * bundles + 1 );
      std::vector< int32_t > st( files + 1 );
      rc = zc_index_set_fetch( set, 0, 0, 0, ids.data(), 0, st.data() );
      if ( rc != ZC_OK )
        err = string( "zc_index_set_fetch: " ) + zc_last_error( 0 );
      for ( uint64_t b = 0; b < bundles; ++b )
        bundleIds.push_back( string( (char const *)&ids[ 24 * b ], 24 ) );
      status.assign( st.begin(), st.begin() + files );
    }
    if ( rc == ZC_OK )
    {
      rc = zc_chunk_index_create( ctx, set, &index );
      if ( rc != ZC_OK )
        err = string( "zc_chunk_index_create: " ) + zc_last_error( ctx );
    }
    if ( set )
      zc_index_set_destroy( set );  // the index keeps its own copy
    if ( rc != ZC_OK )
    {
      zc_destroy( ctx );
      throw std::runtime_error( err );
    }
  }

  ~GpuResidentChunkIndex()
  {
    zc_chunk_index_destroy( index );
    zc_destroy( ctx );
  }

  size_t bundles() const { return bundleIds.size(); }
  /// the 24 bytes of bundle n's id (Bundle::Id), which name its file
  string const & bundleId( size_t n ) const { return bundleIds.at( n ); }
  /// ZC_INDEX_* per index file given
  std::vector< int > const & fileStatus() const { return status; }

  void counts( uint64_t & records, uint64_t & ids, uint64_t & flaggedBundles ) const
  {
    uint64_t b = 0;
    if ( zc_chunk_index_counts( index, &records, &b, &ids, &flaggedBundles ) != ZC_OK )
      throw std::runtime_error( string( "zc_chunk_index_counts: " ) + zc_last_error( 0 ) );
  }

  /// findChunk for every id (24-byte ChunkId blobs)
  void findChunks( std::vector< string > const & ids, std::vector< Found > & found )
  {
    size_t n = ids.size();
    std::vector< uint8_t > blobs( 24 * n + 1 );
    for ( size_t i = 0; i < n; ++i )
    {
      if ( ids[ i ].size() != 24 )
        throw std::runtime_error( "GpuResidentChunkIndex: a chunk id that is not 24 bytes" );
      memcpy( &blobs[ 24 * i ], ids[ i ].data(), 24 );
    }
    std::vector< uint32_t > bundle( n + 1 ), size( n + 1 );
    std::vector< uint64_t > off( n + 1 );
    zcCheck( zc_chunk_index_lookup( ctx, index, blobs.data(), n, bundle.data(), off.data(), size.data() ), ctx,
             "zc_chunk_index_lookup" );
    found.resize( n );
    for ( size_t i = 0; i < n; ++i )
    {
      Found f = { bundle[ i ], off[ i ], size[ i ] };
      found[ i ] = f;
    }
  }

  /// The whole backup at once.  Throws exNoSuchChunk naming the first chunk no
  /// bundle holds, exDuplicateChunks naming the first used bundle that holds
  /// an id twice (Bundle::Reader would refuse to open it).
  void plan( string const & backupData, Plan & out )
  {
    size_t count = 0;
    zc_parse_instructions( backupData.data(), backupData.size(), 0, 0, &count );
    std::vector< zc_instruction > ins( count + 1 );
    if ( zc_parse_instructions( backupData.data(), backupData.size(), ins.data(), ins.size(), &count ) != ZC_OK )
      throw std::runtime_error( string( "zc_parse_instructions: " ) + zc_last_error( 0 ) );
    zc_restore_plan * p = 0;
    zcCheck( zc_restore_resolve( ctx, index, ins.data(), count, backupData.size(), &p ), ctx, "zc_restore_resolve" );
    uint64_t n = 0, used = 0, missing = 0, firstMissing = 0, dupUsed = 0, firstDup = 0;
    zc_restore_plan_counts( p, &n, &used, &out.length, &missing, &firstMissing, &dupUsed, &firstDup );
    out.used.assign( used + 1, 0 );
    out.usedSize.assign( used + 1, 0 );
    out.slot.assign( n + 1, 0 );
    out.off.assign( n + 1, 0 );
    out.size.assign( n + 1, 0 );
    out.dst.assign( n + 1, 0 );
    zc_restore_plan_fetch( p, out.used.data(), out.usedSize.data(), out.slot.data(), out.off.data(), out.size.data(),
                           out.dst.data() );
    zc_restore_plan_destroy( p );
    out.used.resize( used );
    out.usedSize.resize( used );
    out.slot.resize( n );
    out.off.resize( n );
    out.size.resize( n );
    out.dst.resize( n );
    if ( missing )
      throw exNoSuchChunk( "chunk " + hex( ins[ firstMissing ].id, 24 ) + " is in no bundle of the index" );
    if ( dupUsed )
      throw exDuplicateChunks( "bundle " + hex( (uint8_t const *)bundleIds[ out.used[ out.slot[ firstDup ] ] ].data(), 24 ) +
                               " holds a chunk id twice" );
  }

  friend class GpuBackupRestorer;
};

/// restoreIterations (backup_restorer.cc:109-136) with every intermediate
/// instruction stream kept in HBM: backup_data is uploaded once, then
/// iterations + 1 rounds of zc_parse_instructions_device,
/// zc_restore_resolve_device and zc_restore_replay, each round's output the next
/// round's stream.  Per round the host sees the used bundles and their payload
/// sizes, fetches those payloads from the PayloadSource (each bundle once: a
/// payload stays in HBM for the rounds that follow) and nothing per entry.  The
/// user data comes back in one read at the end.  Throws
/// GpuResidentChunkIndex::exNoSuchChunk and exDuplicateChunks, as
/// GpuResidentChunkIndex::plan does.  Uses the C ABI only.
class GpuBackupRestorer: NoCopy
{
public:
  typedef GpuIndexedRestorer::PayloadSource PayloadSource;  // getPayload( the index's bundle number, payload )

private:
  // device buffers of one call, freed with it
  struct Buffers: NoCopy
  {
    zc_ctx * ctx;
    std::vector< void * > all;
    explicit Buffers( zc_ctx * c ): ctx( c ) {}
    void * get( uint64_t bytes )
    {
      void * p = 0;
      zcCheck( zc_device_alloc( ctx, bytes, &p ), ctx, "zc_device_alloc" );
      all.push_back( p );
      return p;
    }
    void drop( void * p )
    {
      for ( size_t i = 0; i < all.size(); ++i )
        if ( all[ i ] == p )
        {
          zc_device_free( ctx, p );
          all.erase( all.begin() + i );
          return;
        }
    }
    ~Buffers()
    {
      for ( size_t i = 0; i < all.size(); ++i )
        zc_device_free( ctx, all[ i ] );
    }
  };

  struct Handles: NoCopy
  {
    zc_instr_set * set;
    zc_restore_plan * plan;
    Handles(): set( 0 ), plan( 0 ) {}
    ~Handles()
    {
      if ( plan )
        zc_restore_plan_destroy( plan );
      if ( set )
        zc_instr_set_destroy( set );
    }
  };

public:
  /// BackupInfoT: zbackup's BackupInfo, or anything with backup_data() and
  /// iterations().  out: the user data.  roundsOut, if given: the length of
  /// every round's output, the user data's last.
  template< class BackupInfoT >
  static void restoreIterations( BackupInfoT const & info, GpuResidentChunkIndex & index, PayloadSource & source,
                                 string & out, std::vector< uint64_t > * roundsOut = 0 )
  {
    zc_ctx * ctx = index.ctx;
    Buffers bufs( ctx );
    string const & backupData = info.backup_data();
    void * stream = bufs.get( backupData.size() );
    uint64_t n = backupData.size();
    zcCheck( zc_upload( ctx, stream, backupData.data(), n ), ctx, "zc_upload" );
    std::vector< void * > resident( index.bundles(), (void *) 0 );  // bundle -> its payload in HBM
    for ( uint64_t round = 0; round <= (uint64_t) info.iterations(); ++round )
    {
      Handles h;
      zcCheck( zc_parse_instructions_device( ctx, n ? stream : 0, n, &h.set ), ctx, "zc_parse_instructions_device" );
      zcCheck( zc_restore_resolve_device( ctx, index.index, h.set, &h.plan ), ctx, "zc_restore_resolve_device" );
      uint64_t entries = 0, used = 0, length = 0, missing = 0, firstMissing = 0, dupUsed = 0, firstDup = 0;
      zc_restore_plan_counts( h.plan, &entries, &used, &length, &missing, &firstMissing, &dupUsed, &firstDup );
      std::vector< uint32_t > usedBundle( used + 1 );
      std::vector< uint64_t > usedSize( used + 1 );
      zc_restore_plan_used( h.plan, usedBundle.data(), usedSize.data() );
      if ( missing )
      {
        zc_instruction one;  // the one entry the message names
        if ( zc_instr_set_fetch( h.set, firstMissing, 1, &one ) != ZC_OK )
          throw std::runtime_error( string( "zc_instr_set_fetch: " ) + zc_last_error( 0 ) );
        throw GpuResidentChunkIndex::exNoSuchChunk( "chunk " + GpuResidentChunkIndex::hex( one.id, 24 ) +
                                                    " is in no bundle of the index" );
      }
      if ( dupUsed )
      {
        uint32_t slot = 0;
        if ( zc_restore_plan_entry( h.plan, firstDup, &slot, 0, 0, 0 ) != ZC_OK )
          throw std::runtime_error( string( "zc_restore_plan_entry: " ) + zc_last_error( 0 ) );
        throw GpuResidentChunkIndex::exDuplicateChunks(
          "bundle " + GpuResidentChunkIndex::hex( (uint8_t const *) index.bundleIds[ usedBundle[ slot ] ].data(), 24 ) +
          " holds a chunk id twice" );
      }
      std::vector< void const * > slots( used + 1 );
      for ( uint64_t k = 0; k < used; ++k )
      {
        uint32_t b = usedBundle[ k ];
        if ( !resident[ b ] )
        {
          string payload;
          source.getPayload( b, payload );
          if ( payload.size() != usedSize[ k ] )
            throw std::runtime_error( "GpuBackupRestorer: a payload's size differs from the index's" );
          void * p = bufs.get( payload.size() );
          zcCheck( zc_upload( ctx, p, payload.data(), payload.size() ), ctx, "zc_upload" );
          resident[ b ] = p;
        }
        slots[ k ] = resident[ b ];
      }
      slots[ used ] = stream;  // the round's bytes_to_emit runs are read from its own stream
      void * next = bufs.get( length );
      zcCheck( zc_restore_replay( ctx, h.plan, slots.data(), slots.size(), next, length ), ctx, "zc_restore_replay" );
      bufs.drop( stream );  // the replay is complete: nothing reads the round's stream any more
      stream = next;
      n = length;
      if ( roundsOut )
        roundsOut->push_back( length );
    }
    // the user data, one read through the range reader's staging buffer
    out.resize( n );
    if ( n )
    {
      zc_range_index * one = 0;
      uint32_t slot = 0;
      uint64_t zero = 0;
      zcCheck( zc_range_index_create( ctx, &n, 1, &slot, &zero, &n, 1, &one ), ctx, "zc_range_index_create" );
      int rc = zc_range_set_slot( one, 0, stream );
      if ( rc == ZC_OK )
        rc = zc_range_read_host( ctx, one, &zero, &n, 1, &out[ 0 ], &zero );
      string err = rc == ZC_OK ? string() : string( zc_last_error( ctx ) );
      zc_range_index_destroy( one );
      if ( rc != ZC_OK )
        throw std::runtime_error( "GpuBackupRestorer: reading the restored data: " + err );
    }
  }
};

#endif
