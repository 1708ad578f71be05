"""Rates of the garbage-collection plan (zc_gc.hip), beside the reference's
method on one host core.

  python tools/gc_rate.py [--records 1,4,16] [--calls 20] [--warmup 2] [--no-host]

Times whole zc_gc_plan calls (host arrays in, host arrays out: wall clock, with
the call's own device times from zc_gc_last_stats / zc_gc_last_times) at
--records million records with half as many used ids, with and without
ZC_GC_DEEP, after --warmup calls, over --calls calls, and prints one JSON line
per case: the median wall time, the ids (records + used) per second, and the
share of the call in the upload, the table build, the probes, the host's
decisions, the second phase and the read-backs.

Beside it: tools/gc_host/gc_host_walk.cpp, compiled -O3 here, walks the same
input once on one core with the containers the reference declares
(std::set<ChunkId> for usedChunkSet and overallChunkSet): `host_mark_ms` fills
usedChunkSet, `host_walk_ms` is loadIndex's walk with the copies' addChunk.
Its counts must equal the plan's.

The input: records drawn from a pool of 0.7 N ids (so ids repeat), bundles of
0..64 records, 8 index files; the used ids are 3/4 from the pool, 1/4 strangers."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(n, seed=3):
    rng = np.random.default_rng(seed)
    pool_n = max(1, n * 7 // 10)
    pool = rng.integers(0, 256, (pool_n, 24), dtype=np.uint8)
    pool_size = rng.integers(1, 65537, pool_n).astype(np.uint32)
    draw = rng.integers(0, pool_n, n)
    ids, sizes = pool[draw], pool_size[draw]
    lens = rng.integers(0, 65, n // 24 + 8)
    first = np.concatenate([[0], np.minimum(np.cumsum(lens), n)])
    bundle_first = np.concatenate([first[first < n], [n]]).astype(np.uint64)
    nb = len(bundle_first) - 1
    bundle_ids = rng.integers(0, 256, (nb, 24), dtype=np.uint8)
    index_first = (np.arange(9, dtype=np.uint64) * np.uint64(nb)) // np.uint64(8)
    u = n // 2
    used = np.concatenate([pool[rng.integers(0, pool_n, u - u // 4)], rng.integers(0, 256, (u // 4, 24), dtype=np.uint8)])
    return ids, sizes, bundle_first, bundle_ids, index_first, used


def host_lib(tmp):
    src = os.path.join(ROOT, "tools", "gc_host", "gc_host_walk.cpp")
    so = os.path.join(tmp, "libgc_host_walk.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.gc_host_walk.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, ctypes.c_uint32, u64,
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), vp]
    return L


def host_case(L, inp, deep, max_payload):
    ids, sizes, bundle_first, bundle_ids, index_first, used = inp
    mark, walk = ctypes.c_double(), ctypes.c_double()
    counts = np.zeros(5, dtype=np.uint64)
    L.gc_host_walk(ids.ctypes.data, sizes.ctypes.data, len(ids), bundle_first.ctypes.data, bundle_ids.ctypes.data,
                   len(bundle_ids), index_first.ctypes.data, len(index_first) - 1, used.ctypes.data, len(used),
                   1 if deep else 0, max_payload, ctypes.byref(mark), ctypes.byref(walk), counts.ctypes.data)
    return mark.value, walk.value, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1,4,16", help="millions (2^20) of records, comma separated")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch

    from zbackup_amd import Collector
    max_payload = 1 << 21
    with tempfile.TemporaryDirectory() as tmp, Collector() as col:
        L = None if a.no_host else host_lib(tmp)
        for m in [float(x) for x in a.records.split(",")]:
            n = int(m * (1 << 20))
            inp = make_input(n)
            ids, sizes, bundle_first, bundle_ids, index_first, used = inp
            col._used = [used]
            for deep in (False, True):
                wall, parts = [], []
                for k in range(a.warmup + a.calls):
                    plan = col.plan_arrays(ids, sizes, bundle_first, bundle_ids, index_first, deep=deep,
                                           max_payload=max_payload)
                    if k >= a.warmup:
                        parts.append(col.last_stats())
                        wall.append(parts[-1]["call_ms"])  # the C call alone, not this wrapper's arrays
                med = statistics.median(wall)
                r = {"records": n, "used": len(used), "deep": deep, "calls": a.calls, "wall_ms": round(med, 2),
                     "wall_min_ms": round(min(wall), 2), "ids_per_s": round((n + len(used)) / (med / 1e3)),
                     "table_slots": parts[0]["table_slots"], "max_probe": max(p["max_probe"] for p in parts),
                     "copies": int(plan.copy.size), "new_bundles": int(plan.new_bundle_size.size),
                     "device": torch.cuda.get_device_name(0)}
                for key in ("upload_ms", "build_ms", "probe_ms", "host_ms", "copy_ms", "readback_ms"):
                    v = statistics.median(p[key] for p in parts)
                    r[key] = round(v, 3)
                    r[key.replace("_ms", "_share")] = round(v / med, 3)
                if L is not None:
                    mark, walk, counts = host_case(L, inp, deep, max_payload)
                    want = [int(plan.bundle_total.sum()), int(plan.bundle_used.sum()), plan.copy.size,
                            plan.new_bundle_size.size]
                    assert counts[:4].tolist() == want, (counts, want)
                    r.update(host_mark_ms=round(mark, 1), host_walk_ms=round(walk, 1),
                             host_ids_per_s=round((n + len(used)) / ((mark + walk) / 1e3)),
                             speedup=round((mark + walk) / med, 1))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
