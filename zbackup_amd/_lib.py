"""ctypes binding of libzchunk.so (include/zchunk.h).

The library is built in-tree (zbackup_amd/libzchunk.so).  Loading fails loudly
if it is missing: there is no CPU fallback for the product path.
"""
import ctypes
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libzchunk.so")

ZC_OK, ZC_ERR_ARG, ZC_ERR_HIP, ZC_ERR_NOMEM, ZC_ERR_STATE = 0, -1, -2, -3, -4
ZC_FLAG_SHA1, ZC_FLAG_TIMING, ZC_FLAG_NO_STAGED_SCREEN = 1, 2, 4
ZC_CHUNK_NEW, ZC_CHUNK_DUP, ZC_BYTES = 0, 1, 2

# every symbol include/zchunk.h declares
EXPORTS = ["zc_create", "zc_destroy", "zc_seed_index", "zc_get_input_buffer",
           "zc_get_input_buffer_size", "zc_handle_more_data", "zc_feed", "zc_finish",
           "zc_chunk_device", "zc_record_count", "zc_get_records", "zc_get_stats", "zc_reset",
           "zc_last_error", "zc_fill_splitmix64", "zc_abi_version", "zc_read_stream", "zc_chunk_host",
           "zc_forget_stream_chunks", "zc_set_window", "zc_get_window", "zc_take_records", "zc_sha256_create", "zc_sha256_add", "zc_sha256_finish", "zc_sha256_destroy", "zc_sha256_impl",
           "zc_bundle_plan", "zc_bundle_gather", "zc_lzo_capacity", "zc_lzo_compress", "zc_lzo_compress_host", "zc_lzo_last_stats", "zc_adler32", "zc_serialize_records", "zc_stream_data", "zc_build_id",
           "zc_seed_index_meta", "zc_export_chunk_meta", "zc_anchor_def",
           "zc_lzo_frame_info", "zc_bundle_scatter", "zc_parse_instructions",
           "zc_aes128_cbc_encrypt", "zc_aes128_cbc_decrypt", "zc_aes128_cbc_encrypt_host",
           "zc_aes128_cbc_decrypt_host", "zc_bundle_file_size", "zc_bundle_seal", "zc_bundle_seal_host",
           "zc_bundle_unseal", "zc_bundle_unseal_host", "zc_aes_last_form", "zc_last_stream_paths",
           "zc_gc_plan", "zc_gc_last_stats", "zc_gc_last_times",
           "zc_chunk_meta_compute", "zc_chunk_meta_compute_host", "zc_meta_last_stats",
           "zc_range_index_create", "zc_range_index_total", "zc_range_index_destroy", "zc_range_set_slot",
           "zc_range_slot_upload", "zc_range_slot_drop", "zc_range_needs", "zc_range_read", "zc_range_read_host",
           "zc_range_last_stats", "zc_debug_scan_outputs",
           "zc_index_load", "zc_index_load_host", "zc_index_set_counts", "zc_index_set_fetch", "zc_index_set_device",
           "zc_index_set_destroy", "zc_bundle_info_parse", "zc_bundle_info_parse_host", "zc_index_serialize",
           "zc_index_file_size", "zc_index_last_stats",
           "zc_xz_decode", "zc_xz_decode_host", "zc_xz_last_stats", "zc_device_alloc", "zc_device_free", "zc_upload",
           "zc_xz_capacity", "zc_xz_encode", "zc_xz_encode_host", "zc_xz_encode_last_stats", "zc_xz_encode_last_schedule",
           "zc_chunk_index_create", "zc_chunk_index_create_arrays", "zc_chunk_index_counts", "zc_chunk_index_bundles",
           "zc_chunk_index_lookup", "zc_chunk_index_destroy", "zc_restore_resolve", "zc_restore_plan_counts",
           "zc_restore_plan_fetch", "zc_restore_plan_destroy", "zc_resolve_last_stats",
           "zc_parse_instructions_device", "zc_instr_set_counts", "zc_instr_set_fetch", "zc_instr_set_destroy",
           "zc_instr_last_stats", "zc_restore_resolve_device", "zc_restore_plan_entry", "zc_restore_plan_used",
           "zc_restore_replay", "zc_serialized_size", "zc_serialize_records_device", "zc_serialize_last_stats"]
(ZC_INDEX_OK, ZC_INDEX_BAD_SIZE, ZC_INDEX_BAD_PADDING, ZC_INDEX_TRUNCATED, ZC_INDEX_BAD_VERSION, ZC_INDEX_BAD_MESSAGE,
 ZC_INDEX_BAD_BUNDLE_ID, ZC_INDEX_BAD_CHUNK_ID, ZC_INDEX_BAD_ADLER) = range(9)
INDEX_STATUS_NAMES = {0: "ok", 1: "bad file size", 2: "bad padding", 3: "truncated", 4: "unsupported version",
                      5: "malformed message", 6: "bundle id is not 24 bytes", 7: "chunk id is not 24 bytes",
                      8: "Adler-32 mismatch"}
ZC_META_BAD_SHA1, ZC_META_BAD_ROLLING, ZC_META_BAD_SIZE = 1, 2, 4
ZC_GC_DEEP, ZC_GC_REPACK, ZC_GC_CONCAT = 1, 2, 4
ZC_GC_ACT_KEEP, ZC_GC_ACT_REMOVE, ZC_GC_ACT_REPACK, ZC_GC_ACT_DROP_RECORD = 0, 1, 2, 3
ZC_GC_REC_COUNTED, ZC_GC_REC_USED, ZC_GC_REC_COPIED = 1, 2, 4
ZC_AES_FORM_DECRYPT, ZC_AES_FORM_PLAIN_TABLES, ZC_AES_FORM_LANE, ZC_AES_FORM_AHEAD_1 = 1, 2, 4, 8
ZC_AES_FORM_CPW_SHIFT = 8
ZC_PATH_FUSED_INSERT, ZC_PATH_SCAN_KEYS, ZC_PATH_TABLES_REALLOCATED, ZC_PATH_TABLES_CLEARED_BY_EPOCH = 1, 2, 4, 8
ZC_BUNDLE_OK, ZC_BUNDLE_BAD_SIZE, ZC_BUNDLE_TRUNCATED = 0, 1, 2
ZC_BUNDLE_BAD_ADLER1, ZC_BUNDLE_BAD_ADLER2, ZC_BUNDLE_BAD_PADDING = 3, 4, 5
BUNDLE_STATUS_NAMES = {0: "ok", 1: "bad file size", 2: "truncated", 3: "Adler-32 mismatch after BundleInfo",
                       4: "Adler-32 mismatch after the body", 5: "bad padding"}
ZC_LZO_E_FRAME, ZC_LZO_E_SIZE = -100, -101
ZC_INSTR_CHUNK, ZC_INSTR_BYTES = 0, 1
ZC_META_NO_ANCHOR = 0xFFFFFFFF
ZC_NO_BUNDLE = 0xFFFFFFFF


class ZcRecord(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("rolling", ctypes.c_uint64), ("sha1", ctypes.c_uint8 * 16)]


class ZcSeed(ctypes.Structure):
    _fields_ = [("sha1", ctypes.c_uint8 * 16), ("rolling", ctypes.c_uint64),
                ("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ZcChunkMeta(ctypes.Structure):
    _fields_ = [("sha1", ctypes.c_uint8 * 16), ("rolling", ctypes.c_uint64), ("size", ctypes.c_uint32),
                ("anchor_def", ctypes.c_uint32), ("anchor", ctypes.c_uint32), ("gear", ctypes.c_uint32),
                ("fingerprint", ctypes.c_uint64)]


class ZcInstruction(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("id", ctypes.c_uint8 * 24), ("reserved", ctypes.c_uint32),
                ("data_off", ctypes.c_uint64), ("size", ctypes.c_uint64)]


class ZcBundleFile(ctypes.Structure):
    _fields_ = [("prefix_off", ctypes.c_uint64), ("prefix_len", ctypes.c_uint64), ("body_off", ctypes.c_uint64),
                ("body_len", ctypes.c_uint64), ("file_off", ctypes.c_uint64)]


class ZcBundleLayout(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_uint32), ("header_off", ctypes.c_uint64),
                ("header_len", ctypes.c_uint64), ("info_off", ctypes.c_uint64), ("info_len", ctypes.c_uint64),
                ("body_off", ctypes.c_uint64), ("body_len", ctypes.c_uint64)]


class ZcXzResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("info", ctypes.c_uint32), ("decoded", ctypes.c_uint64),
                ("consumed", ctypes.c_uint64)]


class ZcXzEncResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("info", ctypes.c_uint32), ("size", ctypes.c_uint64)]


ZC_XZ_OK = 0
ZC_XZ_E_OUTPUT = 6
XZ_STATUS_NAMES = {0: "ZC_XZ_OK", 1: "ZC_XZ_E_FORMAT", 2: "ZC_XZ_E_UNSUPPORTED", 3: "ZC_XZ_E_HEADER",
                   4: "ZC_XZ_E_DATA", 5: "ZC_XZ_E_INPUT", 6: "ZC_XZ_E_OUTPUT", 7: "ZC_XZ_E_CHECK",
                   8: "ZC_XZ_E_BUDGET"}


class ZcGcInput(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("sizes", ctypes.c_void_p), ("n_records", ctypes.c_uint64),
                ("bundle_first", ctypes.c_void_p), ("bundle_ids", ctypes.c_void_p), ("n_bundles", ctypes.c_uint64),
                ("index_first", ctypes.c_void_p), ("n_indexes", ctypes.c_uint64),
                ("used", ctypes.c_void_p), ("n_used", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("max_payload", ctypes.c_uint64)]


class ZcGcIndex(ctypes.Structure):
    _fields_ = [("total", ctypes.c_uint64), ("used", ctypes.c_uint64), ("kept", ctypes.c_uint32),
                ("modified_bundles", ctypes.c_uint32), ("removed", ctypes.c_uint32), ("modified", ctypes.c_uint8),
                ("necessary", ctypes.c_uint8), ("unlink", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class ZcGcOutput(ctypes.Structure):
    _fields_ = [("record_flags", ctypes.c_void_p), ("bundle_total", ctypes.c_void_p),
                ("bundle_used", ctypes.c_void_p), ("bundle_action", ctypes.c_void_p), ("indexes", ctypes.c_void_p),
                ("copy", ctypes.c_void_p), ("copy_bundle", ctypes.c_void_p), ("copy_off", ctypes.c_void_p),
                ("copy_cap", ctypes.c_uint64), ("n_copy", ctypes.c_uint64),
                ("new_bundle_index", ctypes.c_void_p), ("new_bundle_size", ctypes.c_void_p),
                ("new_bundle_cap", ctypes.c_uint64), ("n_new_bundles", ctypes.c_uint64)]


class ZcScanOutputs(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("blk", ctypes.c_void_p), ("blk_cap", ctypes.c_size_t),
                ("n_blk", ctypes.c_size_t), ("wt_count", ctypes.c_void_p), ("wt_side", ctypes.c_void_p),
                ("wt_cap", ctypes.c_size_t), ("n_wt", ctypes.c_size_t), ("anchor_pos", ctypes.c_void_p),
                ("anchor_gear", ctypes.c_void_p), ("anchor_cap", ctypes.c_size_t), ("n_anchors", ctypes.c_size_t),
                ("keys", ctypes.c_void_p), ("key_cap", ctypes.c_size_t), ("n_keys", ctypes.c_size_t),
                ("max_tiles_per_wave", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ZcStats(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_double), ("resolve_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("bytes", ctypes.c_uint64),
                ("anchors", ctypes.c_uint64), ("candidates", ctypes.c_uint64),
                ("epochs", ctypes.c_uint64), ("fscan_runs", ctypes.c_uint64),
                ("meta_ms", ctypes.c_double), ("probe_ms", ctypes.c_double),
                ("fscan_ms", ctypes.c_double), ("walk_ms", ctypes.c_double),
                ("finalize_ms", ctypes.c_double), ("fbatch_ms", ctypes.c_double),
                ("window_bytes", ctypes.c_uint64), ("hbm_bytes", ctypes.c_uint64),
                ("segments", ctypes.c_uint64), ("hist_entries", ctypes.c_uint64),
                ("sha_wait_ms", ctypes.c_double), ("sha_fill_ms", ctypes.c_double), ("hist_ms", ctypes.c_double),
                ("respeculations", ctypes.c_uint64), ("chk_rebuilds", ctypes.c_uint64),
                ("hist_seeded", ctypes.c_uint64), ("by_value", ctypes.c_uint64)]


class ZcError(RuntimeError):
    pass


_lib = None


def load(path=LIB_PATH):
    """Load libzchunk.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ZcError(f"{path} not built (run zbackup_amd/_build.py or __graft_entry__.build())")
    from . import _build
    if os.path.abspath(path) == LIB_PATH:
        # the in-tree library must be the one the checked-out sources build
        have, want = _build.lib_build_id(path), _build.source_digest()
        if have != want:
            raise ZcError(f"{path} has build id {have}, the sources give {want}: stale binary "
                          "(run zbackup_amd/_build.py)")
    L = ctypes.CDLL(path)
    vp, u32, u64, sz, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    sig = {
        "zc_create": (i32, [ctypes.POINTER(vp), u32, i32, u32]),
        "zc_destroy": (i32, [vp]),
        "zc_seed_index": (i32, [vp, ctypes.POINTER(ZcSeed), sz]),
        "zc_get_input_buffer": (vp, [vp]),
        "zc_get_input_buffer_size": (sz, [vp]),
        "zc_handle_more_data": (i32, [vp, sz]),
        "zc_feed": (i32, [vp, vp, sz]),
        "zc_finish": (i32, [vp]),
        "zc_chunk_device": (i32, [vp, vp, u64]),
        "zc_record_count": (sz, [vp]),
        "zc_get_records": (i32, [vp, ctypes.POINTER(ZcRecord), sz, ctypes.POINTER(sz)]),
        "zc_get_stats": (i32, [vp, ctypes.POINTER(ZcStats)]),
        "zc_last_stream_paths": (i32, [vp, ctypes.POINTER(u32)]),
        "zc_debug_scan_outputs": (i32, [vp, ctypes.POINTER(ZcScanOutputs)]),
        "zc_reset": (i32, [vp]),
        "zc_last_error": (ctypes.c_char_p, [vp]),
        "zc_fill_splitmix64": (i32, [vp, u64, u64, i32]),
        "zc_abi_version": (i32, []),
        "zc_read_stream": (i32, [vp, u64, sz, vp]),
        "zc_chunk_host": (i32, [vp, vp, u64]),
        "zc_forget_stream_chunks": (i32, [vp]),
        "zc_set_window": (i32, [vp, u64]),
        "zc_get_window": (u64, [vp]),
        "zc_take_records": (i32, [vp, ctypes.POINTER(ZcRecord), sz, ctypes.POINTER(sz)]),
        "zc_sha256_create": (i32, [ctypes.POINTER(vp)]),
        "zc_sha256_add": (i32, [vp, vp, sz]),
        "zc_sha256_finish": (i32, [vp, ctypes.c_char_p]),
        "zc_sha256_destroy": (i32, [vp]),
        "zc_sha256_impl": (i32, [vp]),
        # bundle writer offload (host arrays as pointers: numpy .ctypes.data)
        "zc_bundle_plan": (i32, [vp, sz, u64, vp, ctypes.POINTER(sz)]),
        "zc_bundle_gather": (i32, [vp, vp, vp, vp, sz, vp]),
        "zc_lzo_capacity": (u64, [u64]),
        "zc_lzo_compress": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_lzo_compress_host": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_adler32": (i32, [vp, vp, vp, vp, sz, vp]),
        "zc_serialize_records": (i32, [vp, vp, sz, vp, sz, ctypes.POINTER(sz)]),
        "zc_lzo_last_stats": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]),
        "zc_stream_data": (vp, [vp, u64, sz]),
        "zc_build_id": (ctypes.c_char_p, []),
        "zc_seed_index_meta": (i32, [vp, vp, sz, vp, sz]),
        "zc_export_chunk_meta": (i32, [vp, vp, sz, ctypes.POINTER(sz)]),
        "zc_anchor_def": (u32, [u32]),
        # restore: the bundle frame, chunk scatter, instruction parsing
        "zc_lzo_frame_info": (i32, [vp, sz, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "zc_bundle_scatter": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "zc_parse_instructions": (i32, [vp, sz, vp, sz, ctypes.POINTER(sz)]),
        # encrypted repositories: (ctx, key, in, in_off, len, n, iv, out, out_off)
        "zc_aes128_cbc_encrypt": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_aes128_cbc_decrypt": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_aes128_cbc_encrypt_host": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_aes128_cbc_decrypt_host": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_bundle_file_size": (u64, [u64, u64, i32]),
        # (ctx, key, prefix, files, n, body, files_out, file_size)
        "zc_bundle_seal": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_bundle_seal_host": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        # (ctx, key, files, file_off, file_size, n, plain, plain_off, layout)
        "zc_bundle_unseal": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_bundle_unseal_host": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "zc_aes_last_form": (i32, [vp, ctypes.POINTER(u32)]),
        # garbage collection
        "zc_gc_plan": (i32, [vp, ctypes.POINTER(ZcGcInput), ctypes.POINTER(ZcGcOutput)]),
        "zc_gc_last_stats": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        "zc_gc_last_times": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 4),
        # adoption: (ctx, payload, payload_bytes, off, size, n, expect, out, status, n_bad)
        "zc_chunk_meta_compute": (i32, [vp, vp, u64, vp, vp, sz, vp, vp, vp, ctypes.POINTER(sz)]),
        "zc_chunk_meta_compute_host": (i32, [vp, vp, u64, vp, vp, sz, vp, vp, vp, ctypes.POINTER(sz)]),
        "zc_meta_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 3),
        # random-access restore: (ctx, slot_sizes, n_slots, slot, off, sizes, n, &idx)
        "zc_range_index_create": (i32, [vp, vp, sz, vp, vp, vp, sz, ctypes.POINTER(vp)]),
        "zc_range_index_total": (i32, [vp, ctypes.POINTER(u64)]),
        "zc_range_index_destroy": (i32, [vp]),
        "zc_range_set_slot": (i32, [vp, u32, vp]),
        "zc_range_slot_upload": (i32, [vp, u32, vp, u64]),
        "zc_range_slot_drop": (i32, [vp, u32]),
        # (idx, offset, size, n_reads, slots_out, cap, &n_out)
        "zc_range_needs": (i32, [vp, vp, vp, sz, vp, sz, ctypes.POINTER(sz)]),
        # (ctx, idx, offset, size, n_reads, dst, dst_off)
        "zc_range_read": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "zc_range_read_host": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "zc_range_last_stats": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(u64)]),
        # index files: (ctx, key, files, file_off, file_size, n, &set)
        "zc_index_load": (i32, [vp, vp, vp, vp, vp, sz, ctypes.POINTER(vp)]),
        "zc_index_load_host": (i32, [vp, vp, vp, vp, vp, sz, ctypes.POINTER(vp)]),
        "zc_index_set_counts": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        # (set, ids, sizes, bundle_first, bundle_ids, index_first, status)
        "zc_index_set_fetch": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "zc_index_set_device": (i32, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]),
        "zc_index_set_destroy": (i32, [vp]),
        # (ctx, plain, info_off, info_len, n, ids, sizes, cap, bundle_first, status, &n_records)
        "zc_bundle_info_parse": (i32, [vp, vp, vp, vp, sz, vp, vp, u64, vp, vp, ctypes.POINTER(u64)]),
        "zc_bundle_info_parse_host": (i32, [vp, vp, vp, vp, sz, vp, vp, u64, vp, vp, ctypes.POINTER(u64)]),
        # (ids, sizes, bundle_first, bundle_ids, n_bundles, out, cap, &n_out)
        "zc_index_serialize": (i32, [vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64)]),
        "zc_index_file_size": (u64, [u64, i32]),
        "zc_index_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 5),
        # LZMA bundles: (ctx, in, in_off, in_size, n, out, out_off, out_cap, res)
        "zc_xz_decode": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "zc_xz_decode_host": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "zc_xz_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(u64)]),
        "zc_xz_capacity": (u64, [u64]),
        "zc_xz_encode": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, u32, vp]),
        "zc_xz_encode_host": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, u32, vp]),
        "zc_xz_encode_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 4),
        "zc_xz_encode_last_schedule": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        # resident chunk index: (ctx, set, &idx); (ctx, ids, sizes, n_records, bundle_first, n_bundles, &idx)
        "zc_chunk_index_create": (i32, [vp, vp, ctypes.POINTER(vp)]),
        "zc_chunk_index_create_arrays": (i32, [vp, vp, vp, u64, vp, u64, ctypes.POINTER(vp)]),
        "zc_chunk_index_counts": (i32, [vp] + [ctypes.POINTER(u64)] * 4),
        "zc_chunk_index_bundles": (i32, [vp, vp, vp]),
        # (ctx, idx, ids, n, bundle, off, size)
        "zc_chunk_index_lookup": (i32, [vp, vp, vp, sz, vp, vp, vp]),
        "zc_chunk_index_destroy": (i32, [vp]),
        # (ctx, idx, ins, n, instr_bytes, &plan)
        "zc_restore_resolve": (i32, [vp, vp, vp, sz, u64, ctypes.POINTER(vp)]),
        "zc_restore_plan_counts": (i32, [vp] + [ctypes.POINTER(u64)] * 7),
        # (plan, used, used_size, slot, off, size, dst)
        "zc_restore_plan_fetch": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "zc_restore_plan_destroy": (i32, [vp]),
        "zc_resolve_last_stats": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        # restore iterations: (ctx, d_data, n, &set); (set, first, count, out)
        "zc_parse_instructions_device": (i32, [vp, vp, u64, ctypes.POINTER(vp)]),
        "zc_instr_set_counts": (i32, [vp] + [ctypes.POINTER(u64)] * 3),
        "zc_instr_set_fetch": (i32, [vp, u64, u64, vp]),
        "zc_instr_set_destroy": (i32, [vp]),
        "zc_instr_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 4 + [ctypes.POINTER(u64)] * 2),
        # (ctx, idx, set, &plan); (plan, e, &slot, &off, &size, &dst); (ctx, plan, slot_base, n_slots, d_out, out_cap)
        "zc_restore_resolve_device": (i32, [vp, vp, vp, ctypes.POINTER(vp)]),
        "zc_restore_plan_entry": (i32, [vp, u64, ctypes.POINTER(u32)] + [ctypes.POINTER(u64)] * 3),
        "zc_restore_plan_used": (i32, [vp, vp, vp]),
        "zc_restore_replay": (i32, [vp, vp, vp, sz, vp, u64]),
        # the records serialized in HBM: (recs, n, &bytes); (ctx, recs, n, d_stream, stream_len, d_out, out_cap, &n_out)
        "zc_serialized_size": (i32, [vp, sz, ctypes.POINTER(u64)]),
        "zc_serialize_records_device": (i32, [vp, vp, sz, vp, u64, vp, u64, ctypes.POINTER(u64)]),
        "zc_serialize_last_stats": (i32, [vp] + [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(u64)] * 2),
        "zc_device_alloc": (i32, [vp, u64, ctypes.POINTER(vp)]),
        "zc_device_free": (i32, [vp, vp]),
        "zc_upload": (i32, [vp, vp, vp, u64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def build_id():
    """The build id of the loaded library (the digest of its sources)."""
    return load().zc_build_id().decode()
