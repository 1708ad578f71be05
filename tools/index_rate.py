"""Rates of the index-file loader (zc_index.hip), beside libprotobuf and
libcrypto on one host core.

  python tools/index_rate.py [--records 16] [--calls 5] [--warmup 1] [--no-host] [--no-sweep]

Builds --records million (2^20) chunk records as index files and loads them:

  * in 32-record bundles (the usual bundle of 64 KiB chunks: a BundleInfo of
    1 KiB), as 1,024 index files and as one file, each with and without a key;
  * in 512-record bundles (a BundleInfo of 16 KiB), 1,024 files, without a key.

Per case one JSON line: the call from HBM-resident files (zc_index_load) and
from host memory (zc_index_load_host), wall clock, with the call's own times
from zc_index_last_stats (decrypt, Adler-32, frame, records); beside the
HBM-resident figure `load_plan_ms`, load + Collector.plan_index together, since
that is what `zbackup gc` waits for.  For the one-file case the frame walk is
serial: `frame_us_per_hop` is its time per bundle.

The sweeps (a quarter of the records, 1,024 files, no key): ZC_TEST_INDEX_TILE
over 1 / 4 / 16 KiB and ZC_TEST_INDEX_WAVE_MIN from "every BundleInfo takes a
wave" to "none does", for both bundle sizes.  The defaults in zc_index.hip are
read off these lines.

The baseline is measured here on one core, never against the code under test:
the Python protobuf runtime's ParseFromString (upb, libprotobuf's parser) over
the same BundleInfo bytes, and libcrypto's CBC decrypt (as tools/aes_rate.py).

The files are built with numpy (every size 65536, so every record is 32 bytes),
their Adler-32 by zlib; the keyed ones are encrypted on the GPU by the
library's own CBC encrypt, which tests/test_gpu_aes.py holds to libcrypto."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEY = bytes(range(16))


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def build_plain(rng, n_bundles, per_bundle, keyed):
    """One file's plaintext with n_bundles bundles of per_bundle 32-byte records."""
    rec = np.zeros((n_bundles, per_bundle, 32), dtype=np.uint8)
    rec[:, :, 0:4] = [0x0A, 30, 0x0A, 24]
    rec[:, :, 4:28] = rng.integers(0, 256, (n_bundles, per_bundle, 24), dtype=np.uint8)
    rec[:, :, 28:32] = [0x10, 0x80, 0x80, 0x04]  # size 65536
    head = np.frombuffer(b"\x1a\x0a\x18" + bytes(24) + varint(32 * per_bundle), dtype=np.uint8)
    b = np.zeros((n_bundles, len(head) + 32 * per_bundle), dtype=np.uint8)
    b[:, :len(head)] = head
    b[:, 3:27] = rng.integers(0, 256, (n_bundles, 24), dtype=np.uint8)
    b[:, len(head):] = rec.reshape(n_bundles, -1)
    p = (rng.integers(0, 256, 16, dtype=np.uint8).tobytes() if keyed else b"") + b"\x02\x08\x01" + b.tobytes() + b"\0"
    p += zlib.adler32(p).to_bytes(4, "little")
    if keyed:
        k = 16 - len(p) % 16
        p += bytes([k]) * k
    return p


def build_files(torch, comp, records, n_files, per_bundle, keyed, seed=1):
    """(device image, file_off, file_size, host image) of n_files files holding `records` records."""
    rng = np.random.default_rng(seed)
    per_file = records // per_bundle // n_files
    plains = [build_plain(rng, per_file, per_bundle, keyed) for _ in range(n_files)]
    size = np.array([len(p) for p in plains], dtype=np.uint64)
    cap = (size + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    off = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    img = np.zeros(int(cap.sum()), dtype=np.uint8)
    for o, p in zip(off, plains):
        img[int(o):int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    d = torch.from_numpy(img).to("cuda:0")
    if keyed:
        comp.aes_encrypt(KEY, d.data_ptr(), off, size, d.data_ptr(), off)
        torch.cuda.synchronize()
        img = d.cpu().numpy()
    return d, off, size, img, per_file * n_files * per_bundle


def run_case(torch, comp, name, records, n_files, per_bundle, keyed, calls, warmup, plan=True, env=None):
    from zbackup_amd import Collector, IndexLoader
    d, off, size, img, n = build_files(torch, comp, records, n_files, per_bundle, keyed)
    for k, v in (env or {}).items():
        os.environ[k] = str(v)
    try:
        ld = IndexLoader(ctx=comp._ctx, key=KEY if keyed else None)
        L, ctx = ld._L, ld._ctx
        import ctypes
        dev, host, parts, both = [], [], [], []
        for k in range(warmup + calls):
            h = ctypes.c_void_p()
            t = time.perf_counter()
            rc = L.zc_index_load(ctx, ld._key, ctypes.c_void_p(d.data_ptr()), off.ctypes.data, size.ctypes.data,
                                 len(size), ctypes.byref(h))
            ms = (time.perf_counter() - t) * 1e3
            assert rc == 0, L.zc_last_error(ctx)
            st = ld.last_stats()
            cnt = [ctypes.c_uint64() for _ in range(3)]
            L.zc_index_set_counts(h, *[ctypes.byref(c) for c in cnt])
            assert cnt[2].value == n and cnt[1].value == n // per_bundle, [c.value for c in cnt]
            L.zc_index_set_destroy(h)
            if k >= warmup:
                dev.append(ms)
                parts.append(st)
        for k in range(warmup + min(calls, 3)):
            h = ctypes.c_void_p()
            t = time.perf_counter()
            rc = L.zc_index_load_host(ctx, ld._key, img.ctypes.data, off.ctypes.data, size.ctypes.data, len(size),
                                      ctypes.byref(h))
            ms = (time.perf_counter() - t) * 1e3
            assert rc == 0, L.zc_last_error(ctx)
            L.zc_index_set_destroy(h)
            if k >= warmup:
                host.append(ms)
        if plan:
            col = Collector(ctx=comp._ctx)
            rng = np.random.default_rng(2)
            for k in range(1 + min(calls, 3)):
                t = time.perf_counter()
                iset = ld.load_device(d.data_ptr(), off, size)
                if k == 0:
                    col.mark_ids(iset.ids[rng.integers(0, n, n // 2)])
                col.plan_index(iset)
                if k:
                    both.append((time.perf_counter() - t) * 1e3)
            assert (iset.status == 0).all()
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
    med = statistics.median(dev)
    r = {"case": name, "records": n, "files": n_files, "records_per_bundle": per_bundle, "keyed": keyed,
         "file_bytes": int(size.sum()), "hbm_ms": round(med, 2), "hbm_min_ms": round(min(dev), 2),
         "hbm_records_per_s": round(n / (med / 1e3)), "hbm_GBps": round(int(size.sum()) / med / 1e6, 1),
         "host_ms": round(statistics.median(host), 2)}
    for key in ("decrypt_ms", "adler_ms", "frame_ms", "records_ms"):
        r[key] = round(statistics.median(p[key] for p in parts), 3)
    if n_files == 1:  # one wave walks every bundle: the frame kernel's time is the hops, one after the other
        r["frame_us_per_hop"] = round(r["frame_ms"] * 1e3 / (n // per_bundle), 3)
    if both:
        r["load_plan_ms"] = round(statistics.median(both), 2)
    if env:
        r["env"] = env
    return r


def host_baseline(per_bundle, bundles=2000):
    """One core: upb's ParseFromString over BundleInfo bodies, libcrypto's CBC decrypt."""
    out = {}
    try:
        from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
        F = descriptor_pb2.FieldDescriptorProto
        fd = descriptor_pb2.FileDescriptorProto(name="index_rate.proto", package="index_rate", syntax="proto2")
        m = fd.message_type.add(name="BundleInfo")
        c = m.nested_type.add(name="ChunkRecord")
        c.field.add(name="id", number=1, type=F.TYPE_BYTES, label=F.LABEL_REQUIRED)
        c.field.add(name="size", number=2, type=F.TYPE_UINT32, label=F.LABEL_REQUIRED)
        m.field.add(name="chunk_record", number=1, type=F.TYPE_MESSAGE, label=F.LABEL_REPEATED,
                    type_name=".index_rate.BundleInfo.ChunkRecord")
        pool = descriptor_pool.DescriptorPool()
        pool.Add(fd)
        cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("index_rate.BundleInfo"))
        rng = np.random.default_rng(3)
        p = build_plain(rng, bundles, per_bundle, False)
        step = 27 + len(varint(32 * per_bundle)) + 32 * per_bundle
        infos = [p[3 + k * step + step - 32 * per_bundle:3 + (k + 1) * step] for k in range(bundles)]
        best = None
        for _ in range(3):
            t = time.perf_counter()
            n = 0
            for b in infos:
                msg = cls()
                msg.ParseFromString(b)
                n += len(msg.chunk_record)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        assert n == bundles * per_bundle
        from google.protobuf.internal import api_implementation
        out.update(protobuf_impl=api_implementation.Type(), protobuf_records_per_s=round(n / best),
                   protobuf_MBps=round(sum(len(b) for b in infos) / best / 1e6, 1))
    except ImportError:
        out["protobuf"] = "not installed"
    from tests import aes_ref
    if aes_ref.have_libcrypto():
        data = bytes(64 << 20)
        t = time.perf_counter()
        aes_ref.cbc_decrypt(KEY, bytes(16), data)
        out["libcrypto_decrypt_MBps"] = round(len(data) / (time.perf_counter() - t) / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=16, help="millions (2^20) of records")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    import torch

    from zbackup_amd import _build
    from zbackup_amd.bundle import BundleCompressor
    n = int(a.records * (1 << 20))
    print(json.dumps({"build_id": _build.source_digest(), "device": torch.cuda.get_device_name(0)}), flush=True)
    if not a.no_host:
        for per in (32, 512):
            print(json.dumps({"case": "one host core", "records_per_bundle": per, **host_baseline(per)}), flush=True)
    with BundleCompressor() as comp:
        for name, files, per, keyed in (("1024 files", 1024, 32, False), ("1024 files", 1024, 32, True),
                                        ("one file", 1, 32, False), ("one file", 1, 32, True),
                                        ("1024 files, 512-record bundles", 1024, 512, False)):
            print(json.dumps(run_case(torch, comp, name, n, files, per, keyed, a.calls, a.warmup)), flush=True)
        if not a.no_sweep:
            for per in (32, 512):
                for tile in (1024, 4096, 16384):
                    print(json.dumps(run_case(torch, comp, "sweep tile", n // 4, 1024, per, False, 3, 1, plan=False,
                                              env={"ZC_TEST_INDEX_TILE": tile})), flush=True)
                for wave_min in (1, 512, 2048, 8192, 1 << 30):
                    print(json.dumps(run_case(torch, comp, "sweep wave_min", n // 4, 1024, per, False, 3, 1,
                                              plan=False, env={"ZC_TEST_INDEX_WAVE_MIN": wave_min})), flush=True)


if __name__ == "__main__":
    main()
