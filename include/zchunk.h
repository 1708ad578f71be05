/* zchunk.h -- C ABI of the MI355X rolling-hash chunking engine (libzchunk.so).
 *
 * Drop-in for the inner loop of zbackup's BackupCreator: a byte stream goes
 * in, the backup instruction records come out, bit-exact with
 * /root/reference/backup_creator.cc for the same bytes, chunk.max_size and
 * index contents.  Plain C types only; every call returns an int status
 * (ZC_OK == 0, negative on error; zc_last_error() has the message).  One
 * context per stream per GPU.  Every entry point that takes a context holds a
 * per-context lock for the whole call, so calls on one context from several
 * threads are serialized; give each concurrent thread (a bundle compressor
 * beside the feeding thread, say) a context of its own for concurrency.
 *
 * Reference interfaces each entry point replaces:
 *   zc_create              BackupCreator::BackupCreator(Config const &, ChunkIndex &,
 *                          ChunkStorage::Writer &)        backup_creator.hh:83 / .cc:18-38
 *                          (chunk.max_size = W: zbackup.proto:79, config.cc:266-282)
 *   zc_seed_index          ChunkIndex::loadIndex -> registerNewChunkId, the static
 *                          probe set of an existing repository   chunk_index.cc:26-79,163-182
 *   zc_seed_index_meta     the same, with the content-anchor metadata a sidecar kept for
 *                          the ids (so the anchor probe finds them, not the per-byte
 *                          screen): loadIndex + the sidecar read beside it
 *                                                                chunk_index.cc:26-79,163-182,
 *                                                                zbackup_base.cc:87-100
 *   zc_export_chunk_meta   that metadata for the chunks this context's streams added, for the
 *                          sidecar written at ChunkStorage::Writer::commit
 *                                                                chunk_storage.cc:61-90,
 *                                                                chunk_index.cc:185-202
 *   zc_set_window          the ring of W + page bytes the creator reads through
 *                          (backup_creator.cc:28-37): the stream's bytes held in HBM
 *   zc_get_input_buffer    BackupCreator::getInputBuffer()       backup_creator.hh:78 / .cc:40-43
 *   zc_get_input_buffer_size  BackupCreator::getInputBufferSize() backup_creator.hh:79 / .cc:45-54
 *   zc_handle_more_data    BackupCreator::handleMoreData(unsigned) backup_creator.hh:81 / .cc:56-108
 *   zc_finish              BackupCreator::finish()               backup_creator.hh:85 / .cc:147-172
 *   zc_get_records         BackupCreator::getBackupData(string &) as structured records
 *                          (one per BackupInstruction, zbackup.proto:149-159)
 *                                                                backup_creator.hh:89 / .cc:275-280
 *   zc_take_records        the same, drained as they are cut (outputInstruction,
 *                          backup_creator.cc:267-273, runs during handleMoreData)
 *   zc_chunk_device        the same stream already resident in HBM (feed + finish in one call)
 *   zc_chunk_host          the same stream in host memory, copy overlapped with the scan
 *                          (the read loop of zutils.cc:100-124 + finish in one call)
 *   zc_lzo_frame_info      the frame NoStreamAndUnknownSizeDecoder reads    compression.cc:369-402
 *   zc_bundle_scatter      Bundle::Reader::get for every chunk a restore emits  bundle.cc:235-251
 *   zc_parse_instructions  the Message::parse loop of restore()  backup_restorer.cc:38-107
 *   zc_aes128_cbc_*        Encryption::encrypt / decrypt over whole files          encryption.cc:17-95
 *   zc_bundle_seal         the file Bundle::Creator::write puts through EncryptedFile::OutputStream
 *                                                                bundle.cc:96-155, encrypted_file.cc:239-392
 *   zc_bundle_unseal       the same file read back by Bundle::Reader     bundle.cc:157-218
 *   zc_gc_plan             ZCollector::gc's loadIndex walk through BundleCollector
 *                                                                zutils.cc:450-505, backup_collector.cc:17-144
 *   zc_chunk_meta_compute  no counterpart: the metadata of zc_export_chunk_meta and the full
 *                          ChunkId (chunk_id.hh:16-32, made at backup_creator.cc:127-141) of chunks
 *                          read back out of decoded bundles (Bundle::Reader::get, bundle.cc:235-251)
 *   zc_range_read          BackupRestorer::IndexedRestorer::saveData, a batch of ranges per call
 *                          (zc_range_index_create: its constructor)     backup_restorer.cc:182-316
 *   zc_index_load          ChunkIndex::loadIndex's read of every index file through
 *                          IndexFile::Reader        chunk_index.cc:26-79, index_file.cc:44-76
 *   zc_bundle_info_parse   Message::parse of a bundle file's BundleInfo      bundle.cc:157-218
 *   zc_index_serialize     IndexFile::Writer's messages                     index_file.cc:18-42
 *   zc_xz_decode           LZMADecoder under Bundle::Reader, many bundles a call
 *   zc_xz_encode           LZMAEncoder under Bundle::Creator, many bundles a call
 *                                                      compression.cc:99-107, bundle.cc:179-216
 *   zc_parse_instructions_device, zc_restore_resolve_device, zc_restore_replay
 *                          one round of BackupRestorer::restoreIterations with the stream, its
 *                          entries and the plan in HBM                 backup_restorer.cc:109-136
 *   zc_serialize_records_device
 *                          outputInstruction for every record of a stream that lies in HBM, so
 *                          that the shrink passes of backupFromFileHandle read their input
 *                          where the pass before wrote it    backup_creator.cc:267-273, zutils.cc:137-166
 *   zc_device_alloc, zc_device_free, zc_upload
 *                          no counterpart: device memory for callers that have no HIP binding
 *                          of their own and keep decoded payloads in HBM
 *   zc_last_error          the DEF_EX exceptions / CHECK aborts of the reference
 *                          (backup_creator.cc:112,165-166, chunk_index.hh:88-89)
 */
#ifndef ZCHUNK_H
#define ZCHUNK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZCHUNK_ABI_VERSION 5

enum zc_status {
  ZC_OK = 0,
  ZC_ERR_ARG = -1,      /* bad argument (null pointer, W == 0, misaligned device buffer) */
  ZC_ERR_HIP = -2,      /* HIP runtime error (message in zc_last_error) */
  ZC_ERR_NOMEM = -3,    /* device or host allocation failed */
  ZC_ERR_STATE = -4     /* call out of order (e.g. feeding after zc_finish) */
};

/* context flags */
enum {
  ZC_FLAG_SHA1 = 1u,     /* compute the SHA-1 half of every chunk id (ChunkId::cryptoHash)
                            and register the stream's new chunks in the context's index,
                            so a later stream on the same context can match them */
  ZC_FLAG_TIMING = 2u,   /* record per-stage device timings (zc_get_stats) */
  ZC_FLAG_NO_STAGED_SCREEN = 4u  /* diagnostics: run the exact-hash screen on its lane-per-KiB
                                    kernel only (same records, slower; tests cover both) */
};

/* record kinds: chunk_to_emit of a chunk cut and saved by this stream (NEW),
 * chunk_to_emit of a window matched in the index (DUP), bytes_to_emit (BYTES,
 * fragments under 128 bytes; the bytes are the caller's [offset, offset+size)) */
enum { ZC_CHUNK_NEW = 0, ZC_CHUNK_DUP = 1, ZC_BYTES = 2 };

typedef struct {
  uint64_t offset;   /* stream offset of the first byte the instruction covers */
  uint32_t size;     /* bytes covered */
  uint32_t kind;     /* ZC_CHUNK_NEW / ZC_CHUNK_DUP / ZC_BYTES */
  uint64_t rolling;  /* ChunkId::rollingHash (RollingHash digest); 0 for BYTES */
  uint8_t sha1[16];  /* ChunkId::cryptoHash (SHA-1 prefix) if ZC_FLAG_SHA1, else 0 */
} zc_record;

/* one entry of an existing index: a ChunkId and the chunk size */
typedef struct {
  uint8_t sha1[16];
  uint64_t rolling;
  uint32_t size;
  uint32_t reserved;
} zc_seed;

/* ABI 5: the content-anchor metadata of one W-byte chunk of an index.  The
 * engine finds windows equal to indexed chunks by their first content anchor
 * (DESIGN.md §2); chunks whose bytes it never held (a repository's earlier
 * backups, known to ChunkIndex only by id) are otherwise screened for by key at
 * every byte.  The metadata is a pure function of the chunk's bytes, so it never
 * goes stale: a caller keeps it beside the repository's index, keyed by the
 * ChunkId, and seeds it with the ids (zc_seed_index_meta).  Matches are still
 * confirmed by rolling key + SHA-1 prefix, as ChunkIndex::findChunk confirms
 * them (chunk_index.cc:119-143), whatever the metadata says. */
#define ZC_META_NO_ANCHOR 0xFFFFFFFFu
typedef struct {
  uint8_t sha1[16];      /* ChunkId::cryptoHash */
  uint64_t rolling;      /* ChunkId::rollingHash */
  uint32_t size;         /* chunk size (W for every entry the engine exports) */
  uint32_t anchor_def;   /* zc_anchor_def() of the engine that computed the entry */
  uint32_t anchor;       /* offset of the chunk's first content anchor, ZC_META_NO_ANCHOR: none */
  uint32_t gear;         /* the anchor's key */
  uint64_t fingerprint;  /* the anchor's 64-bit fingerprint */
} zc_chunk_meta;

typedef struct {
  double scan_ms;        /* zc_scan kernel (HIP events on the context stream) */
  double resolve_ms;     /* everything after the scan: total_ms - scan_ms with ZC_FLAG_TIMING */
  double total_ms;       /* whole call, wall clock */
  uint64_t bytes;        /* stream length */
  uint64_t anchors;      /* content anchors found by the scan */
  uint64_t candidates;   /* anchor-probe candidates */
  uint64_t epochs;       /* resolution epochs (1 + grid-shifting matches) */
  uint64_t fscan_runs;   /* screen-hit runs from the exact-hash screen */
  double meta_ms;        /* epoch index + probe batch (first epoch: device time from the scan's end;
                            later ones: wall clock; summed) */
  double probe_ms;       /* anchor table + probe + candidate verification */
  double fscan_ms;       /* exact-hash screen */
  double walk_ms;        /* boundary walk + record assembly on the host */
  double finalize_ms;    /* digests of cut pieces, SHA-1 ids */
  double fbatch_ms;      /* (part of walk_ms) batched key/byte/SHA-1 checks of screen hits */
  uint64_t window_bytes; /* feed window (zc_set_window; 0: unbounded) */
  uint64_t hbm_bytes;    /* device memory the context holds now */
  uint64_t segments;     /* window segments resolved during the feed */
  uint64_t hist_entries; /* historic index entries (chunks whose bytes have left HBM) */
  /* parts of finalize_ms (ZC_FLAG_SHA1): */
  double sha_wait_ms;    /* blocked on the grid chunks' SHA-1 and its copy to the host */
  double sha_fill_ms;    /* after it: SHA-1 prefixes into the records, the new chunks' index entries completed */
  double hist_ms;        /* before it: the stream's new chunks joining the context's index (keys, anchors) */
  uint64_t respeculations; /* streams redone because a speculative key + SHA-1 class join proved wrong */
  /* ABI 4: */
  uint64_t chk_rebuilds;   /* the one-level static screen's check table rebuilt larger for an epoch's own keys */
  /* ABI 5: */
  uint64_t hist_seeded;    /* historic index entries seeded with anchor metadata (zc_seed_index_meta) */
  uint64_t by_value;       /* index entries known by value only (the exact screen's key set) */
} zc_stats;

typedef struct zc_ctx zc_ctx;

int zc_create(zc_ctx** out, uint32_t chunk_max_size, int device, uint32_t flags);
int zc_destroy(zc_ctx* ctx);
/* KNOWN DIVERGENCE from the reference, the only one: the index holds W-byte
 * chunks only.  Entries whose size is not chunk.max_size are skipped by
 * zc_seed_index and zc_seed_index_meta, and the sub-W chunks a context's own
 * streams save (a flush before a match, a stream's tail) are reported as NEW
 * records but never registered.  ChunkIndex::findChunk compares the rolling
 * hash and the 16 SHA-1 bytes and never the size (chunk_index.cc:119-143), so
 * the reference would match a W-byte window with an indexed chunk of another
 * length that had the same 64-bit rolling hash and the same SHA-1 prefix: a
 * collision of both hashes between byte strings of different lengths.
 * Registering such ids would put every sub-W chunk of a repository (each
 * backup's tail) into the by-value set, whose presence sends every stream
 * through the per-byte exact screen instead of the anchor probe.
 * tests/golden/refpin_divergent/ records the reference's verdict on such an
 * index; tests/test_gpu_refpin.py asserts what the engine gives instead. */
int zc_seed_index(zc_ctx* ctx, const zc_seed* seeds, size_t n);
/* ABI 5.  Seed the ids of an existing index (as zc_seed_index) together with the
 * metadata kept for them: an id whose entry in meta[0, nm) matches its full
 * ChunkId and size W and carries this engine's anchor definition joins the
 * historic index (found by the anchor probe); the other ids are seeded by value
 * (the exact screen); meta entries for ids not in seeds are ignored (an id
 * that is not in the index never matches).  Call before the context's first
 * stream adds chunks to its index (or after zc_forget_stream_chunks):
 * ZC_ERR_STATE otherwise. */
int zc_seed_index_meta(zc_ctx* ctx, const zc_seed* seeds, size_t n, const zc_chunk_meta* meta, size_t nm);
/* ABI 5.  The metadata of the W-byte chunks this context's streams added to its
 * index (ZC_FLAG_SHA1: Writer::add -> ChunkIndex::addChunk; in the order they
 * were added; not the seeded ones): *n_out = their count; ZC_ERR_ARG (with
 * *n_out the count) when cap is smaller. */
int zc_export_chunk_meta(const zc_ctx* ctx, zc_chunk_meta* out, size_t cap, size_t* n_out);
/* the anchor definition of this build for chunk.max_size W (it names the gear,
 * the anchor rate for W, the minimum anchor offset and the fingerprint);
 * metadata of another definition is ignored when seeding */
uint32_t zc_anchor_def(uint32_t chunk_max_size);

/* Host feed (zero-copy contract of BackupCreator: fill getInputBuffer() with up
 * to getInputBufferSize() bytes, then report how many were written).
 *
 * The feed streams through a bounded window (default 1 GiB, at least
 * 8 W + 16 MiB; zc_set_window before the stream's first byte, 0 = keep the whole
 * stream in HBM and resolve it at zc_finish): the bytes are copied to HBM as
 * they arrive, each half window is chunked during zc_handle_more_data, and the
 * window then slides, so device and pinned host memory stay at the window's
 * size for a stream of any length.  Chunks whose bytes leave the window stay
 * in the index by {rolling key, SHA-1 prefix, first content anchor} (the
 * historic index), as the reference's index keeps ids, not bytes.
 * Records are complete as soon as they are cut; zc_take_records drains them.
 * The payload bytes of records taken (NEW chunks for Writer::add, BYTES for
 * bytes_to_emit) stay readable with zc_read_stream until the next
 * zc_get_input_buffer / zc_get_input_buffer_size / zc_feed / zc_finish call. */
/* (the window's buffers are made on a helper thread from this call on, joined
 * by the first zc_get_input_buffer: call it early -- before the index load --
 * to overlap the ~0.3 s it takes to pin 1 GiB of host memory) */
int zc_set_window(zc_ctx* ctx, uint64_t bytes);
uint64_t zc_get_window(const zc_ctx* ctx);
void* zc_get_input_buffer(zc_ctx* ctx);
size_t zc_get_input_buffer_size(zc_ctx* ctx);
int zc_handle_more_data(zc_ctx* ctx, size_t added);
/* copying convenience form: n bytes through getInputBuffer / handleMoreData in
 * pieces.  A call of more than getInputBufferSize() bytes may resolve several
 * window halves and slide the window between them, so take the records after
 * every call of at most that size when their payload bytes are needed
 * (bytes_to_emit, Writer::add), as the zero-copy loop does. */
int zc_feed(zc_ctx* ctx, const void* host, size_t n);
int zc_finish(zc_ctx* ctx);

/* device-resident stream: d_data is a device pointer on the context's GPU,
 * 16-byte aligned; the call runs the whole pipeline and fills the records.
 * The context's stream is ordered after work already queued on the legacy
 * default stream (so a buffer just written there is read complete). */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_chunk_device(zc_ctx* ctx, const void* d_data, uint64_t n);

/* stream in host memory (pinned for full speed): copied to HBM in 64 MiB
 * segments on a side stream, each segment scanned as soon as it has landed,
 * then the same pipeline as zc_chunk_device; the end-to-end form of
 * backup_creator.cc's loop, with the feed's copies overlapped with the work */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_chunk_host(zc_ctx* ctx, const void* host, uint64_t n);

size_t zc_record_count(const zc_ctx* ctx);  /* complete records held (cut, ids filled in, not yet taken) */
int zc_get_records(const zc_ctx* ctx, zc_record* out, size_t cap, size_t* n_out);
/* move up to cap complete records out of the context, in stream order */
int zc_take_records(zc_ctx* ctx, zc_record* out, size_t cap, size_t* n_out);
int zc_get_stats(const zc_ctx* ctx, zc_stats* out);
/* Which code paths the context's last stream took, OR-ed over the epochs and passes of the last
 * zc_chunk_device / zc_chunk_host / zc_finish (a fed stream's window segments included); kept
 * across zc_reset.  For tests of a context that lives through many streams (the epoch tables,
 * their "clean" flag and the scan-written key arrays outlive a stream); a caller needs none of
 * it.  ZC_ERR_ARG for a NULL pointer, ZC_ERR_STATE (with a message in zc_last_error) before the
 * context has finished a stream. */
enum {
  ZC_PATH_FUSED_INSERT = 1,            /* the first epoch's index launch took the fused form: tables found
                                        * clear, every grid key from the scan, inserts in the metadata kernel */
  ZC_PATH_SCAN_KEYS = 2,               /* an epoch took grid keys the scan had written (key_from > 0) */
  ZC_PATH_TABLES_REALLOCATED = 4,      /* an epoch table (class table, anchor table, filter) was reallocated */
  ZC_PATH_TABLES_CLEARED_BY_EPOCH = 8  /* an index launch cleared the tables itself (the non-fused form) */
};
int zc_last_stream_paths(const zc_ctx* ctx, uint32_t* bits);
/* What the scan left behind for the context's last stream (tests only; a caller needs none of it):
 * every word the scan kernel, the tail kernel and the exact rescan of overflowed wave-tiles wrote,
 * copied out of the buffers the context keeps.  The call holds the context's lock, waits for its
 * stream and copies; it launches nothing.  Valid after a finished zc_chunk_device / zc_chunk_host
 * (or a zc_finish with the window set to 0); ZC_ERR_STATE with a message before any stream and
 * after a stream through the feed window (the buffers then hold the window); kept across zc_reset.
 * The caller sets the arrays and their capacities (elements), the call sets the counts:
 *   n, blk[0, n_blk)          the stream's length; the 64-bit digest of every 1 KiB span, n_blk =
 *                             ceil(n / 1024), the partial last span included (the Horner value of
 *                             the bytes present)
 *   wt_count / wt_side[0, n_wt)  per 256 KiB wave-tile t < ceil(n / 256 KiB): its anchors, and 1 when
 *                             its directory entry points into the side pool (it was rescanned exactly)
 *   anchor_pos / anchor_gear[0, n_anchors)  the anchors of all wave-tiles in wave-tile order, as the
 *                             directory lists them: stream position and the 32-bit gear word
 *   keys[0, n_keys)           the grid keys the scan wrote (key i: chunk [i W, (i + 1) W) of the full
 *                             2 MiB tiles), while they are still the scan's: a stream of one epoch
 *                             (zc_stats.epochs == 1) whose epoch took them as they were; else n_keys = 0
 *   max_tiles_per_wave        at least one wave walked this many wave-tiles in a scan-kernel launch of the
 *                             stream: ceil(wave-tiles / waves) of the launch (waves claim their wave-tiles)
 * ZC_ERR_ARG with the counts set when an array is missing or too small (all capacities 0 asks for the
 * counts); ZC_ERR_STATE when a wave-tile is still marked overflowed, a directory entry points outside
 * its pool, or the pinned host copy of the keys differs from the device's (errors of the engine). */
typedef struct zc_scan_outputs {
  uint64_t n;
  uint64_t* blk;
  size_t blk_cap, n_blk;
  uint32_t* wt_count;
  uint8_t* wt_side;
  size_t wt_cap, n_wt;
  uint64_t* anchor_pos;
  uint32_t* anchor_gear;
  size_t anchor_cap, n_anchors;
  uint64_t* keys;
  size_t key_cap, n_keys;
  uint32_t max_tiles_per_wave;
  uint32_t reserved;
} zc_scan_outputs;
int zc_debug_scan_outputs(const zc_ctx* ctx, zc_scan_outputs* out);
int zc_reset(zc_ctx* ctx); /* begin a new stream (the seeded index is kept) */
/* drop the index entries this context's streams added (ZC_FLAG_SHA1: Writer::add ->
 * ChunkIndex::addChunk, chunk_storage.cc:31-46), keeping the seeded ones.  Only for streams
 * whose backups are DISCARDED (never committed), or for benchmarking a first backup on warm
 * buffers: a committed backup's chunks are in its index file, which ChunkIndex::loadIndex
 * reads on the next open (chunk_storage.cc:61-80, chunk_index.cc:26-79), so they must stay
 * in the index (keep them, or re-seed them from the written index). */
int zc_forget_stream_chunks(zc_ctx* ctx);
/* copy bytes [offset, offset+n) of the last processed stream to host memory
 * (the payload of BYTES records, for serializing bytes_to_emit, and of NEW
 * chunks, for Writer::add); for a fed stream, the bytes still in its window */
int zc_read_stream(const zc_ctx* ctx, uint64_t offset, size_t n, void* host_out);
/* the same bytes without a copy, for a fed stream: a pointer into the feed
 * window's pinned host mirror, valid until the next zc_get_input_buffer /
 * zc_get_input_buffer_size / zc_feed / zc_finish / zc_reset call; NULL when
 * the range is not in host memory (a device-resident stream: zc_read_stream) */
const void* zc_stream_data(const zc_ctx* ctx, uint64_t offset, size_t n);
/* the records' BackupInstruction stream, as BackupCreator::outputInstruction writes it
 * (Message::serialize, message.cc:16-23: varint32 length + field 1 chunk_to_emit =
 * ChunkId::toBlob (chunk_id.cc:19-27) | field 2 bytes_to_emit, the record's bytes read from
 * the last stream as zc_read_stream does): n records into out (cap bytes); *n_out = the bytes
 * written, or needed (ZC_ERR_ARG) when cap is too small */
int zc_serialize_records(const zc_ctx* ctx, const zc_record* recs, size_t n, void* out, size_t cap,
                         size_t* n_out);
/* (ctx NULL: the message of the calling thread's last failed call that takes no context) */
const char* zc_last_error(const zc_ctx* ctx);

/* synthetic seeded stream on the device (tests / benchmarks): byte k is byte
 * k mod 8 of splitmix64 word k / 8, little-endian */
int zc_fill_splitmix64(void* d_data, uint64_t n, uint64_t seed, int device);

/* Whole-stream SHA-256 of the input, host side (replaces the Sha256 the feed loop
 * keeps beside BackupCreator: sha256.hh:14-35, fed at zutils.cc:119, finished into
 * BackupInfo.sha256 at zutils.cc:134, checked on restore at zutils.cc:225-232).
 * One serial chain, so it runs on the host CPU (SHA extensions when present). */
typedef struct zc_sha256 zc_sha256;
int zc_sha256_create(zc_sha256** out);                           /* Sha256::Sha256  sha256.cc:8-11 */
int zc_sha256_add(zc_sha256* h, const void* data, size_t n);     /* Sha256::add     sha256.cc:13-16 */
int zc_sha256_finish(zc_sha256* h, uint8_t out[32]);             /* Sha256::finish  sha256.cc:18-21; once */
int zc_sha256_destroy(zc_sha256* h);
int zc_sha256_impl(const zc_sha256* h); /* 1: x86 SHA extensions, 0: scalar */

/* ---- Bundle writer offload ----
 * ChunkStorage::Writer::add's bundling rule (chunk_storage.cc:31-46): the chunks that
 * index.addChunk accepted, in order; chunk i joins the current bundle unless the bundle's
 * payload + sizes[i] > max_payload (config bundle.max_payload_size, default 0x200000,
 * zbackup.proto:88), which first finishes the bundle.  bundle_of[i] receives chunk i's
 * bundle, *n_bundles their count.  Host bookkeeping only (no device work). */
int zc_bundle_plan(const uint64_t* sizes, size_t n, uint64_t max_payload, uint32_t* bundle_of,
                   size_t* n_bundles);
/* Bundle::Creator::addChunk's payload (bundle.cc:30-36) on the device: chunk i's bytes
 * d_src[src_off[i] ..+ sizes[i]) appended to d_payload back to back (HBM to HBM). */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_bundle_gather(zc_ctx* ctx, const void* d_src, const uint64_t* src_off, const uint64_t* sizes,
                     size_t n, void* d_payload);
/* The lzo1x_1 compression Bundle::Creator::write runs on each bundle's payload
 * (bundle.cc:120-151 -> LZO1X_1_Encoder::doProcessNoSize, compression.cc:586-606 -> liblzo2
 * lzo1x_1_compress) with zbackup's framing (NoStreamAndUnknownSizeEncoder::doProcess,
 * compression.cc:435-466: LE32 size, "EFGH", LE32 compressed size, "MNOP", the LZO stream):
 * payload i = d_payload[pay_off[i] ..+ pay_size[i]) (pay_size[i] < 2^32), its framed bytes go
 * to d_out + out_off[i], which must leave zc_lzo_capacity(pay_size[i]) bytes; out_size[i]
 * (host) receives their count.  The bytes equal what the reference writes for the payload. */
uint64_t zc_lzo_capacity(uint64_t payload_size); /* LZO1X_1_Encoder::suggestOutputSize + 16 */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_lzo_compress(zc_ctx* ctx, const void* d_payload, const uint64_t* pay_off, const uint64_t* pay_size,
                    size_t n, void* d_out, const uint64_t* out_off, uint64_t* out_size);
/* the same for payloads in host memory (copied to HBM, compressed, copied back to
 * out + out_off[i]): the form Bundle::Creator::write can call per finished bundle (or per
 * batch of them) without device buffers of its own */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_lzo_compress_host(zc_ctx* ctx, const void* payload, const uint64_t* pay_off, const uint64_t* pay_size,
                         size_t n, void* out, const uint64_t* out_off, uint64_t* out_size);
/* Adler-32 (zlib's adler32 from its initial value 1, as Adler32 wraps it: adler32.hh:13-33) of
 * each device range d_base[off[i] ..+ len[i]) -> out[i] (host).  EncryptedFile::OutputStream
 * keeps one running Adler-32 over everything a bundle file holds and writes it after the
 * BundleInfo and after the payload (encrypted_file.cc:248-300,336-340, bundle.cc:116,153):
 * the payload's share comes from here, joined to the running value with zlib's
 * adler32_combine(running, out[i], len[i]). */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_adler32(zc_ctx* ctx, const void* d_base, const uint64_t* off, const uint64_t* len, size_t n,
               uint32_t* out);
/* device time of the last zc_lzo_compress's parse kernel (ms) and its 48 KiB blocks */
int zc_lzo_last_stats(const zc_ctx* ctx, double* parse_ms, uint64_t* blocks);

/* ---- Restore: replaying a BackupInstruction stream over decoded bundles ----
 * restore() (backup_restorer.cc:38-107) parses the instruction stream and, per chunk_to_emit,
 * copies the chunk out of its bundle's decoded payload (Bundle::Reader::get, bundle.cc:235-251);
 * per bytes_to_emit it appends the bytes.  Here: the parse (host), the frame a bundle's lzo1x
 * stream is stored under (host), and the copies on the device, HBM to HBM.  The decoding of
 * the lzo1x stream itself is the caller's (liblzo2's lzo1x_decompress_safe, as the reference
 * calls it: compression.cc:472-490).  Callers detect these entry points by their symbols (the
 * ABI version stays 5).
 *
 * The codes of a framed bundle beside liblzo2's own (-4 .. -8): */
#define ZC_LZO_E_FRAME (-100) /* fewer than 16 bytes, or 16 + csize > in_size */
#define ZC_LZO_E_SIZE  (-101) /* stream ok, but decoded size != the frame's size */
/* the frame's two sizes (host memory; no device work): ZC_OK, or ZC_LZO_E_FRAME */
int zc_lzo_frame_info(const void* framed, size_t avail, uint64_t* payload_size, uint64_t* compressed_size);
/* The inverse of zc_bundle_gather (Bundle::Reader::get, bundle.cc:235-251, for every chunk a
 * restore emits): extent i, d_src[src_off[i] ..+ sizes[i]), goes to d_dst + dst_off[i].  One source
 * extent may go to many destinations (a chunk emitted more than once). */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_bundle_scatter(zc_ctx* ctx, const void* d_src, const uint64_t* src_off, const uint64_t* sizes,
                      size_t n, void* d_dst, const uint64_t* dst_off);
/* One entry per chunk_to_emit / bytes_to_emit of a BackupInstruction stream, in the order
 * restore() acts on them (an instruction's chunk before its bytes). */
enum { ZC_INSTR_CHUNK = 0, ZC_INSTR_BYTES = 1 };
typedef struct {
  uint32_t kind;      /* ZC_INSTR_CHUNK / ZC_INSTR_BYTES */
  uint8_t id[24];     /* CHUNK: ChunkId::toBlob (chunk_id.cc:19-27) */
  uint32_t reserved;
  uint64_t data_off;  /* BYTES: offset of the raw bytes inside the stream given */
  uint64_t size;      /* BYTES: their count */
} zc_instruction;
/* The inverse of zc_serialize_records (Message::parse, message.cc:24-42; zbackup.proto:149-159):
 * each message is a varint32 length plus fields 1 (chunk_to_emit, 24 bytes) and/or 2
 * (bytes_to_emit), in either order, each at most once.  *n_out = the entries found; ZC_ERR_ARG
 * (message in zc_last_error(NULL), per thread) when cap is smaller, or on anything else: a
 * truncated varint, a length past the end, another field number, a chunk blob that is not 24
 * bytes.  Host memory only. */
int zc_parse_instructions(const void* data, size_t n, zc_instruction* out, size_t cap, size_t* n_out);

/* ---- Encrypted repositories: AES-128-CBC and the bundle file around it ----
 * A repository opened with a password writes every bundle file through
 * EncryptedFile::OutputStream (encrypted_file.cc:239-392, bundle.cc:96-155): AES-128 in CBC mode
 * (Encryption::encrypt, encryption.cc:17-54) from a zero IV over a random first block, PKCS#7
 * padding, a running Adler-32; a restore reads it back through EncryptedFile::InputStream and
 * Encryption::decrypt (bundle.cc:157-218, encryption.cc:63-95).  Callers detect these entry
 * points by their symbols (the ABI version stays 5).
 *
 * n independent CBC chains under one 16-byte key: chain i's input is d_in[in_off[i] ..+ len[i]),
 * its output goes to d_out + out_off[i]; iv = n x 16 host bytes, or NULL: the zero IV
 * (Encryption::ZeroIv) for every chain.  ZC_ERR_ARG, with a message in zc_last_error and before
 * any device work: a NULL key or pointer, len[i] == 0 or not a multiple of 16, an offset or base
 * pointer that is not 16-byte aligned, output extents that overlap each other.  Encrypt: chain
 * i's output extent may be exactly its input extent (in place); any other overlap of an output
 * with an input is ZC_ERR_ARG.  Decrypt works on all blocks at once, so ANY overlap between an
 * input and an output extent is ZC_ERR_ARG. */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_aes128_cbc_encrypt(zc_ctx* ctx, const uint8_t key[16], const void* d_in, const uint64_t* in_off,
                          const uint64_t* len, size_t n, const uint8_t* iv, void* d_out, const uint64_t* out_off);
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_aes128_cbc_decrypt(zc_ctx* ctx, const uint8_t key[16], const void* d_in, const uint64_t* in_off,
                          const uint64_t* len, size_t n, const uint8_t* iv, void* d_out, const uint64_t* out_off);
/* the same for buffers in host memory (copied to HBM, run, copied back); the rules above hold
 * for the host extents, but the base pointers need no alignment */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_aes128_cbc_encrypt_host(zc_ctx* ctx, const uint8_t key[16], const void* in, const uint64_t* in_off,
                               const uint64_t* len, size_t n, const uint8_t* iv, void* out,
                               const uint64_t* out_off);
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_aes128_cbc_decrypt_host(zc_ctx* ctx, const uint8_t key[16], const void* in, const uint64_t* in_off,
                               const uint64_t* len, size_t n, const uint8_t* iv, void* out,
                               const uint64_t* out_off);

/* Which CBC kernel the context's last launch dispatched (a chain call, or a seal / unseal with a
 * key).  The library compiles several forms of each kernel and picks one per call from the
 * environment (ZC_AES_TABLE=shared, ZC_AES_ENC=lane, ZC_AES_CPW=<1..64>, ZC_AES_PREFETCH=1: kept
 * for measurements); this reports the one that ran, recorded where it is launched.
 * ZC_ERR_ARG with a message when the context has launched no CBC kernel yet. */
enum {
  ZC_AES_FORM_DECRYPT = 1,       /* the decrypt kernel */
  ZC_AES_FORM_PLAIN_TABLES = 2,  /* plain 1 KiB tables in LDS, not the 32-fold replicated ones */
  ZC_AES_FORM_LANE = 4,          /* the lane-per-chain encrypt kernel, not four lanes per chain */
  ZC_AES_FORM_AHEAD_1 = 8,       /* the lane kernel reads one block ahead, not four */
  ZC_AES_FORM_CPW_SHIFT = 8      /* bits 8-15: chains per wave of the lane kernel, else 0 */
};
int zc_aes_last_form(const zc_ctx* ctx, uint32_t* form);

/* A bundle file's plaintext: [R: 16 random bytes, with a key only] BundleFileHeader message,
 * BundleInfo message (each a varint32 length + that many bytes, message.cc:16-22), A1, the
 * compressed body (zc_lzo_compress's framed bytes), A2 [, PKCS#7 padding of 1..16 bytes with a
 * key].  A1 / A2 = little-endian zlib Adler-32 of everything before them.  With a key the whole
 * file is one CBC chain from the zero IV.  prefix = R + the two messages.
 * Bytes of such a file (host arithmetic): keyed (P + 4 + B + 4) / 16 * 16 + 16, else P + B + 8. */
uint64_t zc_bundle_file_size(uint64_t prefix_len, uint64_t body_len, int keyed);
typedef struct zc_bundle_file {
  uint64_t prefix_off, prefix_len;  /* the bundle's prefix inside the host blob `prefix` */
  uint64_t body_off, body_len;      /* its compressed body inside d_body */
  uint64_t file_off;                /* where its file goes inside d_files (16-byte aligned) */
} zc_bundle_file;
/* Bundle::Creator::write's file (bundle.cc:96-155) for n bundles: builds each plaintext image at
 * d_files + file_off (the prefix bytes -- the caller draws R, so the library stays
 * deterministic --, A1, the body copied HBM to HBM, A2, padding) and, with a key (NULL: none),
 * encrypts it in place.  file_size[i] (host) receives zc_bundle_file_size(...).  ZC_ERR_ARG: a
 * NULL pointer, a misaligned file_off or d_files, files that overlap each other. */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_bundle_seal(zc_ctx* ctx, const uint8_t* key, const void* prefix, const zc_bundle_file* files, size_t n,
                   const void* d_body, void* d_files, uint64_t* file_size);
/* the same with bodies and files in host memory (the files are brought back to files + file_off) */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_bundle_seal_host(zc_ctx* ctx, const uint8_t* key, const void* prefix, const zc_bundle_file* files, size_t n,
                        const void* body, void* files_out, uint64_t* file_size);

/* what a reader finds in one file (the conditions under which the reference throws
 * exIncorrectFileSize, exBadPadding, exAdlerMismatch, or fails to parse); checked in this order */
enum {
  ZC_BUNDLE_OK = 0,
  ZC_BUNDLE_BAD_SIZE = 1,     /* 0 bytes, or not a multiple of 16 with a key */
  ZC_BUNDLE_TRUNCATED = 2,    /* a varint or a message runs past the end, or no room for A1 / A2 */
  ZC_BUNDLE_BAD_ADLER1 = 3,   /* the Adler-32 after BundleInfo */
  ZC_BUNDLE_BAD_ADLER2 = 4,   /* the Adler-32 after the body */
  ZC_BUNDLE_BAD_PADDING = 5   /* last byte not 1..16, or the pad bytes differ (checked first: it
                                 fixes where the body ends) */
};
typedef struct zc_bundle_layout {
  int32_t status;     /* ZC_BUNDLE_*; the fields below are set as far as the file could be read */
  uint32_t reserved;
  uint64_t header_off, header_len;  /* BundleFileHeader's bytes, offsets into this bundle's plaintext */
  uint64_t info_off, info_len;      /* BundleInfo's bytes (zc_bundle_info_parse reads its records) */
  uint64_t body_off, body_len;      /* the compressed body */
} zc_bundle_layout;
/* Bundle::Reader's file (bundle.cc:157-218) for n files d_files[file_off[i] ..+ file_size[i]):
 * decrypts each (key NULL: copies it) to d_plain + plain_off[i] (file_size[i] bytes; no overlap
 * with the files), reads the two lengths, the stored Adler-32s and the padding on the device and
 * checks both Adler-32s (zc_adler32's kernel).  A bad file does not fail the call: it gets its
 * status in layout[i].  ZC_ERR_ARG: NULL pointers, and with a key misaligned offsets / bases. */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_bundle_unseal(zc_ctx* ctx, const uint8_t* key, const void* d_files, const uint64_t* file_off,
                     const uint64_t* file_size, size_t n, void* d_plain, const uint64_t* plain_off,
                     zc_bundle_layout* layout);
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_bundle_unseal_host(zc_ctx* ctx, const uint8_t* key, const void* files, const uint64_t* file_off,
                          const uint64_t* file_size, size_t n, void* plain, const uint64_t* plain_off,
                          zc_bundle_layout* layout);

/* ---- Garbage collection: which chunks are used, which bundles go, what is copied where ----
 * `zbackup gc` (ZCollector::gc, zutils.cc:450-505) puts every chunk_to_emit id of every backup
 * into BundleCollector::usedChunkSet, then ChunkIndex::loadIndex (chunk_index.cc:26-79) walks
 * every chunk record of every index file through the BundleCollector (backup_collector.cc:17-144).
 * zc_gc_plan is that walk for a whole repository in one call: an exact table of the 24-byte ids in
 * HBM (zc_gc_core.h) answers the set lookups, the host takes the per-bundle decisions in order.
 * It plans only: unlinking files, decoding the bundles to repack and writing the new ones
 * (zc_bundle_gather, zc_lzo_compress, zc_bundle_seal) stay with the caller.  Callers detect these
 * entry points by their symbols (the ABI version stays 5).
 *
 * Processing position.  loadIndex and copyUsedChunks walk a bundle's records from the last to the
 * first (chunk_index.cc:55, backup_collector.cc:134): record r of bundle b with k records has
 * position bundle_first[b] + (k-1-r), and "first" below always means the smallest position.
 *
 * Per record (record_flags): COUNTED = processChunk went past its gcDeep test (lines 53-59):
 * always without ZC_GC_DEEP, with it only for the first occurrence of the id over the whole input
 * (overallChunkSet); USED = the id is in `used` (line 62, line 138); COPIED = the record is in
 * the copy list.
 * Per bundle: total = its COUNTED records, used = its COUNTED and USED ones (lines 61-66), and
 * the action finishBundle takes (lines 69-127), decided in bundle order:
 *   REMOVE       used == 0 and total != 0                          (lines 74-80)
 *   REPACK       else used < total, or ZC_GC_REPACK                (lines 81-97)
 *   REMOVE       else deep, total == 0, bundle id not seen before; the id is now seen (100-109)
 *   DROP_RECORD  else deep, total == 0, bundle id seen: the index file is rewritten without the
 *                record, the bundle file is not unlinked           (lines 110-114)
 *   KEEP         else; under deep the bundle id is now seen        (lines 116-124)
 * Per index file: total / used = sums over its bundles (lines 72-73), kept / modified_bundles /
 * removed = its KEEP / REPACK / REMOVE bundles, modified = any bundle not kept, necessary = a
 * COUNTED record of it is USED (line 65), unlink = modified || (deep && !necessary) || concat
 * (finishIndex, lines 24-42).
 * The copy list: for every REPACK bundle in order, its USED records in processing order,
 * COUNTED or not (copyUsedChunks, lines 129-144), except those whose id an earlier entry of the
 * list has (Writer::add -> ChunkIndex::addChunk on the fresh reindex, chunk_storage.cc:31-46,
 * chunk_index.cc:185-202).  copy[k] = the record, copy_bundle[k] = its new bundle by Writer::add's
 * rule with max_payload (zc_bundle_plan), copy_off[k] = its offset in that bundle's payload.
 * finishIndex ends the current new bundle (commit() / reset(), chunk_storage.cc:61-104), so no
 * new bundle spans two index files: new_bundle_index[j] = the index file of new bundle j,
 * new_bundle_size[j] = its payload bytes.
 *
 * ZC_ERR_ARG, with a message in zc_last_error: a NULL pointer; bundle_first / index_first not
 * starting at 0, decreasing, or not ending at n_records / n_bundles; a count of 2^32 - 1 or more;
 * an unknown flag -- all found before the context is looked at --; two records with the same id and
 * different sizes (the reference reads a copied chunk through the old index's first registration,
 * so such an input has no defined result; found on the device, reported after the first phase);
 * copy_cap or new_bundle_cap too small (n_copy / n_new_bundles then hold the counts needed; the
 * other outputs are complete).  Zero records, bundles, index files and used ids are all legal. */
enum { ZC_GC_DEEP = 1u, ZC_GC_REPACK = 2u, ZC_GC_CONCAT = 4u };  /* --gc-deep, gc.repack, gc.concat */
enum { ZC_GC_ACT_KEEP = 0, ZC_GC_ACT_REMOVE = 1, ZC_GC_ACT_REPACK = 2, ZC_GC_ACT_DROP_RECORD = 3 };
enum { ZC_GC_REC_COUNTED = 1u, ZC_GC_REC_USED = 2u, ZC_GC_REC_COPIED = 4u };
typedef struct zc_gc_input {
  const uint8_t* ids;            /* n_records x 24: every chunk record of every index file, in the */
  const uint32_t* sizes;         /*   order read: index file, bundle, BundleInfo.chunk_record(0..k-1) */
  uint64_t n_records;
  const uint64_t* bundle_first;  /* n_bundles + 1: bundle b's records are [bundle_first[b], bundle_first[b+1]) */
  const uint8_t* bundle_ids;     /* n_bundles x 24 */
  uint64_t n_bundles;
  const uint64_t* index_first;   /* n_indexes + 1: index file i's bundles */
  uint64_t n_indexes;
  const uint8_t* used;           /* n_used x 24: the ids the backups emit; duplicates and strangers allowed */
  uint64_t n_used;
  uint32_t flags;                /* ZC_GC_DEEP | ZC_GC_REPACK | ZC_GC_CONCAT */
  uint32_t reserved;
  uint64_t max_payload;          /* bundle.max_payload_size */
} zc_gc_input;
typedef struct zc_gc_index {
  uint64_t total, used;                       /* indexTotalChunks, indexUsedChunks */
  uint32_t kept, modified_bundles, removed;   /* indexKeptBundles, indexModifiedBundles, indexRemovedBundles */
  uint8_t modified, necessary, unlink, reserved;
} zc_gc_index;
typedef struct zc_gc_output {
  uint8_t* record_flags;       /* n_records: ZC_GC_REC_* */
  uint32_t* bundle_total;      /* n_bundles each */
  uint32_t* bundle_used;
  uint8_t* bundle_action;      /* ZC_GC_ACT_* */
  zc_gc_index* indexes;        /* n_indexes */
  uint32_t* copy;              /* copy_cap each */
  uint32_t* copy_bundle;
  uint64_t* copy_off;
  uint64_t copy_cap;
  uint64_t n_copy;             /* out */
  uint32_t* new_bundle_index;  /* new_bundle_cap each */
  uint64_t* new_bundle_size;
  uint64_t new_bundle_cap;
  uint64_t n_new_bundles;      /* out */
} zc_gc_output;
int zc_gc_plan(zc_ctx* ctx, const zc_gc_input* in, zc_gc_output* out);
/* The last zc_gc_plan of the context: device time of the table build (records into processing
 * order, insert) and of the probes (used ids, per-record flags, per-bundle counts), the table's
 * slots (a power of two, at least twice the records; ZC_TEST_GC_BITS=<b> in the environment makes
 * it 2^b when that is smaller and still leaves a free slot: tests only) and the longest probe run
 * any insert or lookup walked. */
int zc_gc_last_stats(const zc_ctx* ctx, double* build_ms, double* probe_ms, uint64_t* table_slots,
                     uint32_t* max_probe);
/* the rest of that call's time: the upload, the host's own steps (the decisions between the
 * phases, the bundling rule over the copy list at the end), the second phase's kernels (candidate
 * insert, compaction), both read-backs with the waits for the device */
int zc_gc_last_times(const zc_ctx* ctx, double* upload_ms, double* host_ms, double* copy_ms, double* readback_ms);

/* ---- Adopting an existing repository: chunk metadata and id check from bundles ----
 * A repository stock zbackup wrote is known by chunk id only, and ids alone go through the exact
 * screen at every byte.  The zc_chunk_meta record that lets an id take the anchor path is a pure
 * function of the chunk's bytes, so it can be computed from the decoded payloads of the
 * repository's bundles (decoding them is the caller's, as for restore; so is reading BundleInfo:
 * the caller passes where each chunk lies).  Chunk i is payload[off[i] ..+ size[i]): any byte
 * offset, any size from 1 up, extents in any order, overlapping or not.  out[i] receives its
 * record under the context's chunk.max_size W (zc_meta_core.h is the definition): the computed
 * ChunkId (SHA-1 prefix + RollingHash digest), its size, zc_anchor_def(W), and -- for size == W
 * only, as zc_export_chunk_meta -- the first content anchor; ZC_META_NO_ANCHOR otherwise.
 * The same pass checks the bundles: with expect[i] the id and size the bundle claims, status[i]
 * receives what differs (ZC_META_BAD_*; 0 without expect) and *n_bad the chunks with a status
 * other than 0.  A mismatch is not an error of the call, and out[i] always carries the computed
 * id.  Records whose status is 0 and whose size is W are what zc_seed_index_meta takes.
 * ZC_ERR_ARG, with a message in zc_last_error and before any device work: a NULL payload, off,
 * size or out with n > 0; size[i] == 0; a chunk that ends past payload_bytes; expect given
 * with neither status nor n_bad.  n == 0 is ZC_OK.  Callers detect these entry points by their
 * symbols (the ABI version stays 5). */
enum { ZC_META_BAD_SHA1 = 1, ZC_META_BAD_ROLLING = 2, ZC_META_BAD_SIZE = 4 };
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_chunk_meta_compute(zc_ctx* ctx, const void* d_payload, uint64_t payload_bytes, const uint64_t* off,
                          const uint32_t* size, size_t n, const zc_seed* expect, zc_chunk_meta* out,
                          uint8_t* status, size_t* n_bad);
/* the same with the payload in host memory (copied to HBM first) */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_chunk_meta_compute_host(zc_ctx* ctx, const void* payload, uint64_t payload_bytes, const uint64_t* off,
                               const uint32_t* size, size_t n, const zc_seed* expect, zc_chunk_meta* out,
                               uint8_t* status, size_t* n_bad);
/* The context's last such call: device time of the rolling-hash / anchor kernel and of the SHA-1
 * kernel, and the whole call's wall clock (uploads, both read-backs and the wait included). */
int zc_meta_last_stats(const zc_ctx* ctx, double* meta_ms, double* sha1_ms, double* total_ms);

/* ---- Random-access restore: any byte range of a backup, from resident bundle payloads ----
 * BackupRestorer::IndexedRestorer (backup_restorer.cc:182-316), which `zbackup nbd` serves a
 * backup through.  The index is made from the stream's entries -- each chunk_to_emit and each
 * bytes_to_emit, in stream order --: entry e is sizes[e] bytes at off[e] of slot[e].  A slot is one
 * resident payload of a size fixed here: a bundle's decoded payload, or the instruction stream
 * itself for the bytes_to_emit runs.  Creation computes the entries' stream positions (the
 * running sum) and checks every entry; ZC_ERR_ARG with a message naming the entry when it names
 * no slot, ends past its slot's size, or takes the sum past 2^64.  ctx gives the device the
 * index's arrays are uploaded to, once; with ctx NULL the index is host only (total, needs and
 * every check work) until the first zc_range_read brings a context.  The index holds no stream
 * state: one context may serve many indices.  Callers detect these entry points by their symbols
 * (the ABI version stays 5). */
typedef struct zc_range_index zc_range_index;
int zc_range_index_create(zc_ctx* ctx, const uint64_t* slot_sizes, size_t n_slots, const uint32_t* slot,
                          const uint64_t* off, const uint64_t* sizes, size_t n, zc_range_index** idx);
int zc_range_index_total(const zc_range_index* idx, uint64_t* bytes);
int zc_range_index_destroy(zc_range_index* idx);
/* A slot's payload: caller-owned device memory of the slot's size (NULL clears it), or a copy the
 * index makes of host bytes and owns (size must equal the slot's); drop clears either.  A pointer
 * may be set, replaced or cleared at any time between calls, so a caller with a bundle cache keeps
 * only part of a large backup in HBM. */
int zc_range_set_slot(zc_range_index* idx, uint32_t slot, const void* d_ptr);
int zc_range_slot_upload(zc_range_index* idx, uint32_t slot, const void* host, uint64_t size);
int zc_range_slot_drop(zc_range_index* idx, uint32_t slot);
/* Host only: the distinct slots the reads [offset[i], offset[i] + size[i]) touch, ascending, into
 * slots_out (room for cap); *n_out receives their number, also when cap is too small (ZC_ERR_ARG). */
int zc_range_needs(const zc_range_index* idx, const uint64_t* offset, const uint64_t* size, size_t n_reads,
                   uint32_t* slots_out, size_t cap, size_t* n_out);
/* One batch of reads: read i's bytes go to d_dst + dst_off[i] (any alignment; destinations must
 * not overlap).  Checked on the host before any device work, ZC_ERR_ARG with a message and nothing
 * written: offset + size > total or wrapping (the reference's exOutOfRange; 0 bytes at offset ==
 * total is allowed, as there); a touched slot without a pointer (the message names the slot); a
 * NULL argument with n_reads > 0.  The reads are cut into pieces of at most 64 KiB, one wave
 * each; every wave checks each source range against its slot's size again (ZC_ERR_STATE if one
 * fails: an internal error). */
int zc_range_read(zc_ctx* ctx, zc_range_index* idx, const uint64_t* offset, const uint64_t* size, size_t n_reads,
                  void* d_dst, const uint64_t* dst_off);
/* Both forms run on the context's stream after the work the caller has queued on the default
 * stream so far, as the other bundle calls do: slots just filled there (a copy, a decode kernel)
 * are read as filled.  Work on other streams is the caller's to finish first.
 * The same to host memory, through a pinned staging buffer of the context: */
int zc_range_read_host(zc_ctx* ctx, zc_range_index* idx, const uint64_t* offset, const uint64_t* size,
                       size_t n_reads, void* host_dst, const uint64_t* dst_off);
/* The context's last such call: device time of the piece list's upload and of the kernel, and
 * the number of pieces. */
int zc_range_last_stats(const zc_ctx* ctx, double* upload_ms, double* kernel_ms, uint64_t* pieces);

/* ---- Index files: a repository's chunk records from the files on disk ----
 * ChunkIndex::loadIndex (chunk_index.cc:26-79) reads every index file through IndexFile::Reader
 * (index_file.cc:44-76, message.cc:24-42, encrypted_file.cc:130-209).  A file's plaintext is
 * [R: 16 random bytes, with a key only], varint32 len + FileHeader{version = 1}, pairs of
 * varint32 len + IndexBundleHeader{id: 24 bytes} and varint32 len + BundleInfo, a varint32 0 (the
 * header without an id), the little-endian Adler-32 of every byte before it [, PKCS#7 padding of
 * 1..16 bytes with a key]; with a key the whole file is one CBC chain from the zero IV.  BundleInfo
 * is repeated 0A <len> ChunkRecord, ChunkRecord is 0A 18 <24-byte id> and 10 <varint32 size> in
 * either order (zbackup.proto:107-145).  Bytes after the Adler-32 of an unkeyed file are ignored.
 * zc_index_load reads n files in one call -- CBC decrypt, frame walk, Adler-32 and record parse all
 * on the device (zc_index_core.h is the reader) -- into flat arrays in zc_gc_input's layout.
 *
 * The reader is strict, as zc_parse_instructions is, and narrower than libprotobuf: a tag is the
 * single byte the writer emits, a field appears at most once, no other field is accepted; a
 * varint32 has at most 5 bytes and fits 32 bits.
 *
 * A bad file does not fail the call: it gets a status, the first failure met reading it front to
 * back (the padding first: it fixes where the file ends; the Adler-32 last, where the reference
 * checks it).  A file whose status is not ZC_INDEX_OK contributes no bundles and no records:
 * index_first[i + 1] == index_first[i].  This departs from loadIndex, which has already handed on
 * the records in front of the failure when the exception reaches it: a backup tool should not act
 * on half a file.
 * Callers detect these entry points by their symbols (the ABI version stays 5). */
enum {
  ZC_INDEX_OK = 0,
  ZC_INDEX_BAD_SIZE = 1,      /* 0 bytes; with a key, not a multiple of 16 */
  ZC_INDEX_BAD_PADDING = 2,   /* last byte not 1..16, or the pad bytes differ */
  ZC_INDEX_TRUNCATED = 3,     /* a message's length varint or the message it announces runs past the
                                 end of the file, or no room for R or the Adler-32 */
  ZC_INDEX_BAD_VERSION = 4,   /* FileHeader.version is not 1 */
  ZC_INDEX_BAD_MESSAGE = 5,   /* the strict rules are broken inside a message: a varint of more than 5
                                 bytes or 32 bits, a field running past its message, another tag, a
                                 repeated field, a missing required field */
  ZC_INDEX_BAD_BUNDLE_ID = 6, /* a bundle id that is not 24 bytes */
  ZC_INDEX_BAD_CHUNK_ID = 7,  /* a chunk id that is not 24 bytes */
  ZC_INDEX_BAD_ADLER = 8      /* the stored Adler-32 does not match */
};
typedef struct zc_index_set zc_index_set;
/* File i is d_files[file_off[i] ..+ file_size[i]) in device memory; key NULL: no encryption.
 * *set receives the loaded arrays (destroy it with zc_index_set_destroy).  ZC_ERR_ARG, with a
 * message and before any device work: NULL pointers, and with a key misaligned offsets / bases
 * (zc_bundle_unseal's rules).  Runs on the context's stream after the work queued on the default
 * stream so far, as the other bundle calls do.  ZC_ERR_STATE: a kernel met one of its own bounds
 * (an internal error).  ZC_TEST_INDEX_TILE=<bytes> and ZC_TEST_INDEX_WAVE_MIN=<bytes> in the
 * environment shrink the LDS tile and the length from which a BundleInfo gets a whole wave: tests
 * only. */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_index_load(zc_ctx* ctx, const uint8_t* key, const void* d_files, const uint64_t* file_off,
                  const uint64_t* file_size, size_t n, zc_index_set** set);
/* the same with the files in host memory (one upload; the base needs no alignment) */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_index_load_host(zc_ctx* ctx, const uint8_t* key, const void* files, const uint64_t* file_off,
                       const uint64_t* file_size, size_t n, zc_index_set** set);
int zc_index_set_counts(const zc_index_set* set, uint64_t* n_files, uint64_t* n_bundles, uint64_t* n_records);
/* Copies out host arrays in zc_gc_input's layout (a NULL pointer skips that array): ids
 * (n_records x 24), sizes (n_records), bundle_first (n_bundles + 1), bundle_ids (n_bundles x 24),
 * index_first (n_files + 1), and status (n_files, ZC_INDEX_*). */
int zc_index_set_fetch(const zc_index_set* set, uint8_t* ids, uint32_t* sizes, uint64_t* bundle_first,
                       uint8_t* bundle_ids, uint64_t* index_first, int32_t* status);
/* the device pointers of ids and sizes (NULL with no records), for consumers that stay in HBM;
 * they live as long as the set */
int zc_index_set_device(const zc_index_set* set, const void** d_ids, const void** d_sizes);
int zc_index_set_destroy(zc_index_set* set);
/* The record kernels alone over the BundleInfo bodies of n unsealed bundle files: bundle i's is
 * d_plain[info_off[i] ..+ info_len[i]) (zc_bundle_layout's info_off is relative to its bundle's
 * plaintext: add plain_off[i]).  status[i] receives ZC_INDEX_OK, _BAD_MESSAGE or _BAD_CHUNK_ID; a bad
 * BundleInfo contributes no records.  ids (cap x 24), sizes (cap) and bundle_first (n + 1) are
 * host arrays; *n_records = the records found, also when cap is too small (ZC_ERR_ARG). */
/* Runs on the context's stream after the work queued on the default stream so far; complete on return. */
int zc_bundle_info_parse(zc_ctx* ctx, const void* d_plain, const uint64_t* info_off, const uint64_t* info_len,
                         size_t n, uint8_t* ids, uint32_t* sizes, uint64_t cap, uint64_t* bundle_first,
                         uint8_t* status, uint64_t* n_records);
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_bundle_info_parse_host(zc_ctx* ctx, const void* plain, const uint64_t* info_off, const uint64_t* info_len,
                              size_t n, uint8_t* ids, uint32_t* sizes, uint64_t cap, uint64_t* bundle_first,
                              uint8_t* status, uint64_t* n_records);
/* Host only, the inverse: the plaintext between R and the Adler-32 (FileHeader, the bundles, the
 * terminator) for n_bundles bundles in zc_gc_input's layout, as IndexFile::Writer emits it.
 * *n_out = the bytes needed, also when cap is too small (ZC_ERR_ARG; message in
 * zc_last_error(NULL), per thread). */
int zc_index_serialize(const uint8_t* ids, const uint32_t* sizes, const uint64_t* bundle_first,
                       const uint8_t* bundle_ids, uint64_t n_bundles, void* out, uint64_t cap, uint64_t* n_out);
/* bytes of the whole file around `body` serialized bytes: keyed (16 + body + 4) / 16 * 16 + 16,
 * else body + 4 */
uint64_t zc_index_file_size(uint64_t body, int keyed);
/* The context's last zc_index_load or zc_bundle_info_parse: time on the stream of the decrypt,
 * the Adler-32 (its read-back included), the frame kernel and the record passes (gather, count,
 * scan, write), and the whole call's wall clock. */
int zc_index_last_stats(const zc_ctx* ctx, double* decrypt_ms, double* adler_ms, double* frame_ms,
                        double* records_ms, double* total_ms);

/* ---- Resident chunk index: a backup's chunk ids resolved on the device ----
 * The reference resolves a restore in three places: ChunkStorage::Reader::get
 * (chunk_storage.cc:214-260) asks ChunkIndex::findChunk (chunk_index.cc:119-161) which bundle holds
 * a chunk id; the table it asks was filled by loadIndex / registerNewChunkId
 * (chunk_index.cc:26-79,163-182); Bundle::Reader (bundle.cc:220-251) then says where the chunk lies
 * in that bundle's payload.  A zc_chunk_index is that table in HBM for a whole repository -- garbage
 * collection's exact id table (zc_gc_core.h) with every record's location beside it -- and
 * zc_restore_resolve turns a parsed BackupInstruction stream into a restore plan against it
 * (zc_resolve_core.h has the steps).  Callers detect these entry points by their symbols (the ABI
 * version stays 5).
 *
 * Input is zc_gc_input's layout: ids (n_records x 24), sizes, bundle_first (n_bundles + 1).
 * Owner of an id: the record with the smallest processing position (zc_gc_plan's comment: bundles
 * in input order, a bundle's records from the last to the first, chunk_index.cc:55) among the
 * records with that id; so the first bundle in input order that holds the id wins, as in
 * registerNewChunkId.  A file of a zc_index_set whose status is not ZC_INDEX_OK has contributed
 * nothing already.
 * Location: record r of bundle b lies at payload offset = the sum of the sizes of b's records in
 * front of it, in BundleInfo order (bundle.cc:221-232), 64 bits; b's payload size is the sum over
 * all of b's records.
 * Duplicate inside a bundle: a bundle whose records hold one id twice cannot be opened
 * (exDuplicateChunks, bundle.cc:229-230).  The index flags exactly those bundles, whatever other
 * bundles hold the same id (a second table keyed by (id, bundle number)); a flagged bundle is an
 * error only when a resolve uses it.
 *
 * zc_chunk_index_create reads a live set's device arrays (no host trip) during the call; the index
 * keeps its own copy in processing order, so it does not depend on the set afterwards.
 * zc_chunk_index_create_arrays takes host arrays (what zc_bundle_info_parse gives a caller who
 * holds only bundle files) and uploads them.  Both run on the context's stream and return with the
 * index complete; after that it is read-only, holds no stream state, and serves any number of
 * lookups and resolves from any context of its device.  ZC_ERR_ARG, with a message in zc_last_error
 * and before any device work: a NULL pointer; 2^32 - 1 or more records or bundles; bundle_first
 * malformed by zc_gc_plan's rules (not starting at 0, decreasing, not ending at n_records).  Zero
 * records and zero bundles are legal.  Table sizes follow zc_gc_plan's (a power of two, at least
 * twice the records); ZC_TEST_RESOLVE_BITS=<b> in the environment shrinks both tables as
 * ZC_TEST_GC_BITS does: tests only. */
typedef struct zc_chunk_index zc_chunk_index;
int zc_chunk_index_create(zc_ctx* ctx, const zc_index_set* set, zc_chunk_index** idx);
int zc_chunk_index_create_arrays(zc_ctx* ctx, const uint8_t* ids, const uint32_t* sizes, uint64_t n_records,
                                 const uint64_t* bundle_first, uint64_t n_bundles, zc_chunk_index** idx);
/* records, bundles, distinct ids, flagged bundles (a NULL pointer skips that count) */
int zc_chunk_index_counts(const zc_chunk_index* idx, uint64_t* n_records, uint64_t* n_bundles, uint64_t* n_ids,
                          uint64_t* n_flagged);
/* per bundle: its payload size and 1 when it holds an id twice (n_bundles each; NULL skips) */
int zc_chunk_index_bundles(const zc_chunk_index* idx, uint64_t* payload_size, uint8_t* dup);
/* Batch findChunk: for each of n ids (host, n x 24) the owner's bundle number, payload offset and
 * size, into host arrays; bundle 0xffffffff (offset and size 0) when the index has no such id. */
#define ZC_NO_BUNDLE 0xFFFFFFFFu
int zc_chunk_index_lookup(zc_ctx* ctx, const zc_chunk_index* idx, const uint8_t* ids, size_t n, uint32_t* bundle,
                          uint64_t* off, uint32_t* size);
int zc_chunk_index_destroy(zc_chunk_index* idx);
/* Resolve: ins is the array zc_parse_instructions produced (host; zc_restore_resolve_device below
 * takes the entries of a stream parsed in HBM), instr_bytes the stream's length.  Entry e of kind CHUNK gets (bundle, off,
 * size) by lookup; an entry of kind BYTES refers to the instruction stream itself at data_off.
 * Used bundles are the distinct bundles of CHUNK entries in ascending bundle number; slot k is the
 * k-th used bundle and slot n_used the instruction stream (zc_range_index_create's convention).
 * dst[e] is the exclusive running sum of the entry sizes, length the total.  A missing id is not a
 * failed call: its entry has slot ZC_NO_BUNDLE and size 0, the plan reports n_missing and the
 * smallest entry that missed (exNoSuchChunk is the caller's to raise, naming ins[first_missing].id).
 * A used bundle that is flagged duplicate is reported the same way: n_dup_used entries, the first
 * of them first_dup.  ZC_ERR_ARG before any device work: a NULL pointer; 2^32 - 1 or more entries;
 * an entry kind other than the two; a BYTES entry that runs past instr_bytes; BYTES sizes whose sum
 * wraps 2^64.  A length that wraps 2^64 only with the chunk sizes, which the device knows, is
 * ZC_ERR_ARG after the probe.  Zero entries are legal. */
typedef struct zc_restore_plan zc_restore_plan;
int zc_restore_resolve(zc_ctx* ctx, const zc_chunk_index* idx, const zc_instruction* ins, size_t n,
                       uint64_t instr_bytes, zc_restore_plan** plan);
/* a NULL pointer skips that count; first_missing / first_dup are 0 when there is none */
int zc_restore_plan_counts(const zc_restore_plan* plan, uint64_t* n_entries, uint64_t* n_used, uint64_t* length,
                           uint64_t* n_missing, uint64_t* first_missing, uint64_t* n_dup_used, uint64_t* first_dup);
/* host arrays (a NULL pointer skips that array): used and used_size (n_used each: the bundle
 * number and its payload size), and per entry slot, off, size and dst (28 bytes an entry) */
int zc_restore_plan_fetch(const zc_restore_plan* plan, uint32_t* used, uint64_t* used_size, uint32_t* slot,
                          uint64_t* off, uint64_t* size, uint64_t* dst);
int zc_restore_plan_destroy(zc_restore_plan* plan);
/* The context's last calls: device time of the last index build's kernels and of the last
 * resolve's or lookup's, and of whichever call came last the table's slots and the longest probe
 * run an insert or lookup walked. */
int zc_resolve_last_stats(const zc_ctx* ctx, double* build_ms, double* resolve_ms, uint64_t* table_slots,
                          uint32_t* max_probe);

/* ---- Restore iterations: the instruction stream parsed, resolved and replayed in HBM ----
 * zbackup stores a backup's instruction stream as a backup of itself (backupFromFileHandle,
 * zutils.cc:137-166) and restoreIterations (backup_restorer.cc:109-136) undoes that: the restored
 * bytes of iteration k are the instruction stream of iteration k - 1.  Here those bytes land in HBM,
 * and these calls keep them there: the parse, the resolve and the replay take and leave their
 * per-entry data on the device.  What comes to the host is the list of used bundles with their
 * sizes (the caller fetches those files) and a handful of counters.  Callers detect these entry
 * points by their symbols (the ABI version stays 5).
 *
 * zc_parse_instructions_device is zc_parse_instructions for a stream in device memory: the same
 * entries in the same order (kind, id, data_off, size) in a zc_instr_set, or ZC_ERR_ARG with *out
 * NULL and zc_last_error "zc_parse_instructions_device: <what> at byte <N>", <what> and <N> the
 * host parser's for its first error.  The frame walk is not made message by message (zc_instr_core.h
 * has the steps); only true message starts are parsed, so whatever a bytes_to_emit payload spells
 * -- a whole instruction stream, in an iteration -- adds no entry and raises no error.  The call
 * runs on the context's stream after the work queued on the default stream so far and is complete
 * on return.  ZC_ERR_ARG before any device work: a NULL pointer with n > 0 (a NULL or zero-length
 * stream is legal and gives zero entries), a NULL out, 2^32 - 1 bytes or more.
 * ZC_TEST_INSTR_TILE=<positions> in the environment, a power of two from 64 up to the default,
 * shrinks the tile, read per call as ZC_TEST_RESOLVE_BITS is: tests only. */
typedef struct zc_instr_set zc_instr_set; /* n entries x zc_instruction, in HBM */
int zc_parse_instructions_device(zc_ctx* ctx, const void* d_data, uint64_t n, zc_instr_set** out);
/* a NULL pointer skips that count; bytes_total: the sum of the BYTES entries' sizes */
int zc_instr_set_counts(const zc_instr_set* set, uint64_t* n_entries, uint64_t* n_messages, uint64_t* bytes_total);
/* entries [first, first + count) to a host array: for tests and for naming one entry in an error */
int zc_instr_set_fetch(const zc_instr_set* set, uint64_t first, uint64_t count, zc_instruction* out);
int zc_instr_set_destroy(zc_instr_set* set);
/* The last parse's device times by step (the hop of a position is computed inside the exit
 * kernel, so hop_ms is 0 and exit_ms holds both; emit_ms: count, scan and write), its tiles and
 * the steps of the chain walk. */
int zc_instr_last_stats(const zc_ctx* ctx, double* hop_ms, double* exit_ms, double* chain_ms, double* emit_ms,
                        uint64_t* tiles, uint64_t* chain_hops);
/* zc_restore_resolve from a zc_instr_set: the same kernels, nothing per entry uploaded, and the
 * plan keeps slot, off, size and dst in HBM; used, used_size and the counters come to the host.
 * zc_restore_plan_counts answers as before; zc_restore_plan_fetch downloads such a plan's lists on
 * demand; zc_restore_plan_entry gives one entry of either kind of plan (a NULL pointer skips that
 * field), to name first_missing or first_dup.  The parser has checked what zc_restore_resolve
 * checks of its array (kinds, BYTES bounds and sum). */
int zc_restore_resolve_device(zc_ctx* ctx, const zc_chunk_index* idx, const zc_instr_set* set,
                              zc_restore_plan** plan);
int zc_restore_plan_entry(const zc_restore_plan* plan, uint64_t e, uint32_t* slot, uint64_t* off, uint64_t* size,
                          uint64_t* dst);
/* used and used_size alone (n_used each; a NULL pointer skips that array): what a caller needs to
 * fetch the bundles, from host memory whichever way the plan was made */
int zc_restore_plan_used(const zc_restore_plan* plan, uint32_t* used, uint64_t* used_size);
/* The plan's copies, HBM to HBM: entry e's size bytes from slot_base[slot[e]] + off[e] to
 * d_out + dst[e].  slot_base is a host array of n_used + 1 device pointers: slot k the decoded
 * payload of used[k], slot n_used the instruction stream the plan was parsed from.  A plan made
 * by zc_restore_resolve works too: its lists are uploaded on its first replay and kept.  An entry
 * longer than 64 KiB is split over waves.  Runs on the context's stream after the work queued on
 * the default stream so far; complete on return.  ZC_ERR_ARG with a message, before any device
 * work: n_slots != n_used + 1, a NULL base for a slot the plan uses, length > out_cap, a plan with
 * missing ids or duplicate-flagged used bundles. */
int zc_restore_replay(zc_ctx* ctx, const zc_restore_plan* plan, const void* const* slot_base, size_t n_slots,
                      void* d_out, uint64_t out_cap);

/* ---- LZMA bundles: xz streams decoded on the device ----
 * zbackup's default compression method: Bundle::Creator writes a bundle's payload through
 * lzma_easy_encoder(6, LZMA_CHECK_CRC64) (compression.cc:78-97) and Bundle::Reader decodes the body
 * zc_bundle_unseal points at (zc_bundle_layout.body_off / body_len) with lzma_stream_decoder
 * (compression.cc:99-107, bundle.cc:179-216).  zc_xz_decode does that for n bundles in one call,
 * a wave per bundle (zc_xz_core.h is the decoder), and the payloads land where zc_bundle_scatter,
 * zc_range_read and zc_chunk_meta_compute read them.
 *
 * The decoder reads the complete LZMA2 / LZMA format and checks the container as the xz format asks,
 * but is narrower than liblzma on purpose: one stream of zero or one block whose only filter is
 * LZMA2, check id 0 (none), 1 (CRC32) or 4 (CRC64).  More blocks, another filter chain, check id 10
 * (SHA-256) and a second stream behind stream padding are ZC_XZ_E_UNSUPPORTED; liblzma reads them,
 * zbackup writes none of them.  liblzma's classes: LZMA_FORMAT_ERROR = E_FORMAT; LZMA_DATA_ERROR =
 * E_HEADER, E_DATA, E_CHECK; LZMA_BUF_ERROR = E_INPUT, E_OUTPUT (lzma_stream_buffer_decode itself
 * reports input that ends early as LZMA_DATA_ERROR).
 * Bytes after the stream's footer are not an error of the decode (liblzma returns LZMA_OK with
 * in_pos at the stream's end): `consumed` says where it ended, for the caller to compare with the
 * body's length, where the reference's Adler-32 check would fail.
 * Callers detect these entry points by their symbols (the ABI version stays 5). */
enum {
  ZC_XZ_OK = 0,
  ZC_XZ_E_FORMAT = 1,      /* not an xz stream */
  ZC_XZ_E_UNSUPPORTED = 2, /* see above; also reserved bits in the stream or block flags */
  ZC_XZ_E_HEADER = 3,      /* a CRC32 of header, block header, index or footer is wrong, or block
                              header, index or footer disagree with the block */
  ZC_XZ_E_DATA = 4,        /* LZMA2 or LZMA data error, block padding not zero */
  ZC_XZ_E_INPUT = 5,       /* the stream runs past in_size */
  ZC_XZ_E_OUTPUT = 6,      /* more output than out_cap: the reference's exTooMuchData */
  ZC_XZ_E_CHECK = 7,       /* the stored CRC32 / CRC64 does not match the output */
  ZC_XZ_E_BUDGET = 8       /* the walk's trip count ran out: never, in a correct build */
};
typedef struct zc_xz_result {
  int32_t status;    /* ZC_XZ_* */
  uint32_t info;     /* bits 0-3: the stream's check id; bit 8: decoded by the wide form */
  uint64_t decoded;  /* bytes written to the output */
  uint64_t consumed; /* bytes of input up to and including the stream footer (status 0 only) */
} zc_xz_result;
/* LZMADecoder (compression.cc:99-107) under Bundle::Reader (bundle.cc:179-216), for n bundles:
 * stream i, d_in[in_off[i] ..+ in_size[i]), decodes to d_out + out_off[i], room out_cap[i].
 * A bad stream does not fail the call: it gets its status.  Nothing outside
 * [out_off[i], out_off[i] + out_cap[i]) is written; on a status other than ZC_XZ_OK the first
 * `decoded` bytes of the range are unspecified.  ZC_ERR_ARG with a message, before any device work:
 * NULL pointers, output ranges that overlap.  No input range may touch an output range.  n == 0 is
 * ZC_OK and launches nothing.  Runs on the context's stream after the work queued on the default
 * stream so far, as the other bundle calls do; complete on return. */
int zc_xz_decode(zc_ctx* ctx, const void* d_in, const uint64_t* in_off, const uint64_t* in_size, size_t n,
                 void* d_out, const uint64_t* out_off, const uint64_t* out_cap, zc_xz_result* res);
/* the same with streams and payloads in host memory (one upload; the decoded bytes are copied back) */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_xz_decode_host(zc_ctx* ctx, const void* in, const uint64_t* in_off, const uint64_t* in_size, size_t n,
                      void* out, const uint64_t* out_off, const uint64_t* out_cap, zc_xz_result* res);
/* The context's last zc_xz_decode: time on the stream of the decode kernels (both forms) and of
 * the check kernel, the whole call's wall clock, and how many bundles the wide form decoded. */
int zc_xz_last_stats(const zc_ctx* ctx, double* decode_ms, double* check_ms, double* total_ms, uint64_t* n_wide);
/* For callers without a HIP binding of their own (the Python wrappers and the adapter's
 * GpuXzBundleDecoder keep decoded payloads in HBM with these).  They are part of the ABI like
 * every other entry point (detected by symbol; the ABI version stays 5).
 * zc_device_alloc: *d_ptr = a buffer of `bytes` bytes (0: a valid pointer to no bytes) on the
 * context's device; on any failure *d_ptr is NULL (ZC_ERR_NOMEM when the device has no room).
 * zc_device_free: waits for the work on the context's stream, then frees; NULL is ZC_OK.
 * zc_upload: n host bytes to device memory on the context's stream, after the work queued on the
 * default stream so far, complete on return; n == 0 is ZC_OK and touches nothing.
 * ZC_ERR_ARG with a message (zc_last_error(NULL) without a context): a NULL context, a NULL d_ptr
 * for zc_device_alloc, a NULL d_dst or host with n > 0. */
int zc_device_alloc(zc_ctx* ctx, uint64_t bytes, void** d_ptr);
int zc_device_free(zc_ctx* ctx, void* d_ptr);
int zc_upload(zc_ctx* ctx, void* d_dst, const void* host, uint64_t n);

/* ---- LZMA bundles: xz streams encoded on the device ----
 * The write side of the above: Bundle::Creator's lzma_easy_encoder(6, LZMA_CHECK_CRC64)
 * (compression.cc:78-97) for n bundles in one call (zc_xzenc_core.h is the encoder).  An xz stream is
 * defined by its decoder: the streams are not liblzma's bytes, they are streams lzma_stream_decoder
 * and zc_xz_decode read back to the payload -- one block, LZMA2 alone, lc=3 lp=0 pb=2, the smallest
 * dictionary size that covers the payload, a greedy parse over hash-table candidates.  The bytes
 * are a function of the payload and the check id alone (not of the batch, the grid or the room).
 * Callers detect these entry points by their symbols (the ABI version stays 5). */
/* Room that always suffices: the stream with every LZMA2 chunk stored (container + 3 bytes per
 * 64 KiB + payload); the encoder never writes more.  32 for an empty payload. */
uint64_t zc_xz_capacity(uint64_t payload_size);
typedef struct zc_xz_enc_result {
  int32_t status; /* ZC_XZ_OK, or ZC_XZ_E_OUTPUT: out_cap[i] is too small */
  uint32_t info;  /* bits 0-3: the check id; from bit 8: the count of LZMA2 chunks written stored */
  uint64_t size;  /* the stream's length (status 0 only) */
} zc_xz_enc_result;
/* Payload i, d_payload[pay_off[i] ..+ pay_size[i]), as an xz stream at d_out + out_off[i], room
 * out_cap[i]; check = 0 (none), 1 (CRC32) or 4 (CRC64, what zbackup writes).  Nothing outside
 * [out_off[i], out_off[i] + out_cap[i]) is written; with out_cap[i] >= zc_xz_capacity(pay_size[i])
 * the status is ZC_XZ_OK; on ZC_XZ_E_OUTPUT the range's bytes are unspecified.  ZC_ERR_ARG with a
 * message, before any device work: NULL pointers, another check id, output ranges that overlap
 * each other or touch a payload, a payload of more than 64 MiB.  n == 0 is ZC_OK and launches
 * nothing.  Runs on the context's stream after the work queued on the default stream so far;
 * complete on return. */
int zc_xz_encode(zc_ctx* ctx, const void* d_payload, const uint64_t* pay_off, const uint64_t* pay_size, size_t n,
                 void* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint32_t check,
                 zc_xz_enc_result* res);
/* the same with payloads and streams in host memory (one upload; the streams are copied back) */
/* A host form: it touches no caller device memory and is not ordered after the default stream;
 * complete on return. */
int zc_xz_encode_host(zc_ctx* ctx, const void* payload, const uint64_t* pay_off, const uint64_t* pay_size, size_t n,
                      void* out, const uint64_t* out_off, const uint64_t* out_cap, uint32_t check,
                      zc_xz_enc_result* res);
/* The context's last zc_xz_encode: time on the stream of the match kernel, the coding kernel and
 * the check kernel (summed over the call's batches), and the whole call's wall clock. */
int zc_xz_encode_last_stats(const zc_ctx* ctx, double* match_ms, double* code_ms, double* check_ms,
                            double* total_ms);
/* Tests only.  The context's last zc_xz_encode: how many batches it was cut into (a launch of the
 * match and of the coding kernel each), the most payloads a wave took in one launch (its rounds), and
 * the hash tables' generation after it; all 0 before the first call.  A NULL output is skipped.
 * Detected by symbol (the ABI version stays 5).  Two environment variables reach the schedule's
 * edges, tests only as ZC_TEST_GC_BITS is: ZC_TEST_XZENC_POOL=<bytes>, read at every call, stands
 * for the share of the free memory in a batch's room for candidates, which stays at least the
 * largest payload (a batch is the longest run of payloads whose sizes fit it; anything that does
 * not parse to at least 1 is ignored); ZC_TEST_XZENC_GEN0=<u32>, read when the context's encoder
 * state is made (its first zc_xz_encode) and used only inside [0, 0xfffffffe], is the generation a
 * fresh or regrown table starts from, so that the 32-bit generation's end is a few calls away;
 * a table cleared because the generations ran out starts from 0 again. */
int zc_xz_encode_last_schedule(const zc_ctx* ctx, uint64_t* batches, uint64_t* max_rounds, uint32_t* generation);

/* ---- the records serialized on the device ----
 * zc_serialize_records for a stream that lies in HBM, its output left in HBM: the same bytes (one
 * message per record: 0x12 and the stream's bytes [offset, offset + size) for kind ZC_BYTES, 0x0a
 * and the 24-byte chunk id for every other kind value), without a host copy per bytes_to_emit.
 * The output is a stream zc_chunk_device can chunk where it lies, which is the input of
 * backupFromFileHandle's shrink passes (zutils.cc:137-166).  Callers detect these entry points by
 * their symbols (the ABI version stays 5). */
/* The length of the records' stream: what zc_serialize_records reports as needed, with no
 * context and no stream.  Host bookkeeping only.  ZC_ERR_ARG with a message in
 * zc_last_error(NULL): NULL bytes, NULL recs with n > 0. */
int zc_serialized_size(const zc_record* recs, size_t n, uint64_t* bytes);
/* recs: n records in host memory (uploaded in one copy); d_stream: the device buffer of
 * stream_len bytes their offsets refer to (given here, not taken from the context's last
 * stream); d_out: room for out_cap bytes in device memory, which must not overlap d_stream.
 * *n_out = the bytes written.  Only [d_out, d_out + *n_out) is written.  ZC_ERR_ARG with a
 * message, before any device work and with the output untouched: NULL n_out, NULL recs with
 * n > 0, NULL d_stream with stream_len > 0, NULL d_out with out_cap > 0, n >= 2^32 - 1, a
 * ZC_BYTES record with offset + size > stream_len (the message names the record's index), and
 * out_cap smaller than the stream, when *n_out = the bytes needed.  n == 0 is ZC_OK, writes
 * nothing and sets *n_out = 0.  Runs on the context's stream after the work queued on the default
 * stream so far; complete on return. */
int zc_serialize_records_device(zc_ctx* ctx, const zc_record* recs, size_t n, const void* d_stream,
                                uint64_t stream_len, void* d_out, uint64_t out_cap, uint64_t* n_out);
/* The context's last zc_serialize_records_device: time on the stream of the records' upload, of
 * the length kernel with its scans, and of the write and copy kernels; the messages assembled
 * whole in LDS and the 64 KiB copies the longer payloads took.  A NULL output is skipped. */
int zc_serialize_last_stats(const zc_ctx* ctx, double* upload_ms, double* size_ms, double* write_ms,
                            uint64_t* staged_msgs, uint64_t* copy_pieces);

int zc_abi_version(void);
/* digest of the sources this library was built from (zbackup_amd/_build.py
 * source_digest(): sha256 of every source and header, first 16 hex digits).
 * Loaders compare it with the checked-out tree and refuse a stale binary. */
const char* zc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
