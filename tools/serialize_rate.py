"""Rates of the backup data that stays in HBM (zc_ser.hip): records serialized on
the device and the shrink loop of backupFromFileHandle run there, beside the only
route the host serializer leaves from a device-resident stream.

  python tools/serialize_rate.py [--calls 5] [--sweep 1] [--only NAME] [--routes ab|a|b]
                                 [--out profiles/serialize_rate_<build>.jsonl]

The records are hand-built over a stream of random bytes in HBM (a chunk
record's id is random; a BYTES record's range lies in the stream), so a shape is
its record list.  Per shape, the median of --calls runs after one warm-up of

  (a) serialize_device, then the shrink loop on the device (reset, chunk_device
      on the serialized buffer, the records, serialize_device again, until a
      pass is no shorter), and the final stream's download: each part's wall
      time, the loop's by part (summed over its passes), and the first
      serialization's device time by step (zc_serialize_last_stats);
  (b) zc_serialize_records -- one synchronous copy per bytes_to_emit -- then the
      same loop with the stream uploaded (zc_upload), zc_chunk_device and
      zc_serialize_records again.

Both routes run in one process, on one context, alternating, each from an index
that holds the data stream's chunks alone, with the data stream as the
context's last stream; their final streams, iterations and pass lengths are
compared in every run.
--sweep adds record counts from 16 up, chunk records only and with every other
record a BYTES of 1 to 127 bytes, to find where (b) stops being faster.  No
counter profile belongs in the same run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = 65536


def chunk_records(rng, n):
    from zbackup_amd import RECORD_DTYPE
    recs = np.zeros(n, dtype=RECORD_DTYPE)
    recs["kind"] = rng.integers(0, 2, n)
    recs["size"] = W
    recs["rolling"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    recs["sha1"] = rng.integers(0, 256, (n, 16))
    return recs


def with_bytes(rng, chunks, n_bytes, stream_len):
    """n_bytes BYTES records of 1 to 127 bytes spread evenly between the chunk records."""
    from zbackup_amd import RECORD_DTYPE, ZC_BYTES
    raw = np.zeros(n_bytes, dtype=RECORD_DTYPE)
    raw["kind"] = ZC_BYTES
    raw["size"] = rng.integers(1, 128, n_bytes)
    raw["offset"] = rng.integers(0, stream_len - 128, n_bytes)
    n = len(chunks) + n_bytes
    out = np.zeros(n, dtype=RECORD_DTYPE)
    at = np.zeros(n, dtype=bool)
    at[np.linspace(0, n - 1, n_bytes).astype(np.int64)] = True
    assert int(at.sum()) == n_bytes
    out[at], out[~at] = raw, chunks
    return out


def one_bytes(size):
    from zbackup_amd import RECORD_DTYPE, ZC_BYTES
    recs = np.zeros(1, dtype=RECORD_DTYPE)
    recs["kind"], recs["size"] = ZC_BYTES, size
    return recs


def med(xs):
    return round(statistics.median(xs), 3)


class Parts(dict):
    """Wall time by part, in seconds: add(name, t0) adds the time since t0 and returns now."""

    def add(self, name, t0):
        t = time.perf_counter()
        self[name] = self.get(name, 0.0) + t - t0
        return t


def route_a(bc, recs, d_stream, stream_len):
    t, lp = Parts(), Parts()  # the route's parts; the loop's parts, summed over its passes
    t0 = time.perf_counter()
    cur, cur_n = bc.serialize_device(recs, d_stream, stream_len)
    t.add("serialize", t0)
    stats = bc.serialize_stats()
    lengths, it = [cur_n], 0
    t2 = time.perf_counter()
    while True:
        t3 = time.perf_counter()
        bc.reset()
        bc.chunk_device(cur, cur_n)
        t3 = lp.add("chunk", t3)
        got = bc.records()
        t3 = lp.add("records", t3)
        nxt, nxt_n = bc.serialize_device(got, cur, cur_n)
        t3 = lp.add("serialize", t3)
        lengths.append(nxt_n)
        shorter = nxt_n < cur_n
        bc.free_device(cur if shorter else nxt)
        lp.add("free", t3)
        if not shorter:
            break
        cur, cur_n, it = nxt, nxt_n, it + 1
    t4 = t.add("shrink", t2)
    data = bc._download(cur, cur_n)
    t.add("download", t4)
    bc.reset()
    bc.free_device(cur)
    return data, it, lengths, t, lp, stats


def route_b(bc, recs, d_buf, cap):
    L, ctx = bc._L, bc._ctx
    t, lp = Parts(), Parts()
    t0 = time.perf_counter()
    cur = bc._serialize(recs)
    t1 = t.add("serialize", t0)
    lengths, it = [len(cur)], 0
    while True:
        assert len(cur) <= cap
        t3 = time.perf_counter()
        host = np.frombuffer(cur or b"\0", dtype=np.uint8)
        assert L.zc_upload(ctx, ctypes.c_void_p(d_buf), host.ctypes.data, len(cur)) == 0
        t3 = lp.add("upload", t3)
        bc.reset()
        bc.chunk_device(d_buf, len(cur))
        t3 = lp.add("chunk", t3)
        got = bc.records()
        t3 = lp.add("records", t3)
        nxt = bc._serialize(got)
        lp.add("serialize", t3)
        lengths.append(len(nxt))
        if len(nxt) >= len(cur):
            break
        cur, it = nxt, it + 1
    t.add("shrink", t1)
    bc.reset()
    return cur, it, lengths, t, lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sweep", type=int, default=1)
    ap.add_argument("--only", default="", help="the shapes whose name contains this")
    ap.add_argument("--routes", default="ab", choices=["ab", "a", "b"],
                    help="one route alone: what the other leaves behind in the process is then not in its times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from zbackup_amd import BackupCreator, _build, serialized_size
    assert torch.cuda.is_available(), "serialize_rate.py measures on the GPU"
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="setup", build_id=_build.source_digest(), device=torch.cuda.get_device_name(0), W=W, calls=a.calls)
    rng = np.random.default_rng(17)
    stream_len = (64 << 20) + 4096
    stream = torch.empty(stream_len, dtype=torch.uint8, device="cuda:0")
    stream.random_(0, 256)
    torch.cuda.synchronize()
    d_stream = stream.data_ptr()
    shapes = [("131072 chunk records", chunk_records(rng, 131072)),
              ("1048576 chunk records", chunk_records(rng, 1048576)),
              ("131072 chunk records, 100000 BYTES of 1..127", with_bytes(rng, chunk_records(rng, 131072), 100000,
                                                                          stream_len)),
              ("one BYTES of 64 MiB", one_bytes(64 << 20)),
              ("1024 chunk records", chunk_records(rng, 1024))]
    if a.sweep:
        for n in (16, 64, 256, 4096, 16384):
            shapes.append((f"sweep: {n} chunk records", chunk_records(rng, n)))
        for n in (16, 64, 256, 1024, 4096, 16384):
            shapes.append((f"sweep: {n} records, every other a BYTES of 1..127",
                           with_bytes(rng, chunk_records(rng, n // 2), n // 2, stream_len)))
    shapes = [sh for sh in shapes if a.only in sh[0]]
    with BackupCreator(W) as bc:
        for name, recs in shapes:
            need = serialized_size(recs)
            d_up = ctypes.c_void_p()
            assert bc._L.zc_device_alloc(bc._ctx, need, ctypes.byref(d_up)) == 0
            t_a = {k: [] for k in ("serialize", "shrink", "download", "upload_ms", "size_ms", "write_ms")}
            t_b = {k: [] for k in ("serialize", "shrink")}
            loop_a = {k: [] for k in ("chunk", "records", "serialize", "free")}
            loop_b = {k: [] for k in ("upload", "chunk", "records", "serialize")}
            for k in range(a.calls + 1):
                results = []
                for route in a.routes:
                    # untimed, the same for both routes: an index that holds the data stream's chunks
                    # alone, the data stream as the context's last stream (zc_serialize_records reads it)
                    bc.reset()
                    bc.forget_stream_chunks()
                    bc.chunk_device(d_stream, stream_len)
                    torch.cuda.synchronize()
                    if route == "a":
                        data, it, lengths, t, lp, st = route_a(bc, recs, d_stream, stream_len)
                    else:
                        data, it, lengths, t, lp = route_b(bc, recs, d_up.value, need)
                    results.append((data, it, lengths))
                    if k == 0:
                        continue
                    for key, v in t.items():
                        (t_a if route == "a" else t_b)[key].append(v * 1e3)
                    for key, v in lp.items():
                        (loop_a if route == "a" else loop_b)[key].append(v * 1e3)
                    if route == "a":
                        for key in ("upload_ms", "size_ms", "write_ms"):
                            t_a[key].append(st[key])
                assert len(results) < 2 or results[0] == results[1], f"{name}: the routes differ"
            bc._L.zc_device_free(bc._ctx, d_up)
            big = (recs["kind"] == 2) & (recs["size"] > 128)
            row = dict(what="shape", shape=name, routes=a.routes, records=len(recs),
                       bytes_records=int((recs["kind"] == 2).sum()), stream_bytes=need, iterations=results[0][1],
                       pass_lengths=results[0][2], staged_msgs=int(len(recs) - big.sum()),
                       copy_pieces=int(sum((int(x) + 65535) // 65536 for x in recs["size"][big])))
            if "a" in a.routes:
                total_a = med([sum(v) for v in zip(t_a["serialize"], t_a["shrink"], t_a["download"])])
                row.update(a_serialize_ms=med(t_a["serialize"]), a_shrink_ms=med(t_a["shrink"]),
                           a_download_ms=med(t_a["download"]), a_total_ms=total_a,
                           a_dev_upload_ms=med(t_a["upload_ms"]), a_dev_size_ms=med(t_a["size_ms"]),
                           a_dev_write_ms=med(t_a["write_ms"]), a_loop_ms={k: med(v) for k, v in loop_a.items()})
            if "b" in a.routes:
                total_b = med([sum(v) for v in zip(t_b["serialize"], t_b["shrink"])])
                row.update(b_serialize_ms=med(t_b["serialize"]), b_shrink_ms=med(t_b["shrink"]), b_total_ms=total_b,
                           b_loop_ms={k: med(v) for k, v in loop_b.items()})
            if a.routes == "ab":
                row.update(b_over_a=round(total_b / total_a, 2))
            emit(**row)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
