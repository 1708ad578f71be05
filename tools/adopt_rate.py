"""Rates of repository adoption (zc_meta.hip): chunk metadata and id check from
bundle payloads, beside the same definition on one host core.

  python tools/adopt_rate.py [--bundles 8,64,256] [--calls 5] [--warmup 1] [--no-host]

The input is what stock zbackup leaves behind at its defaults' scale: bundles of
2 MiB payload, each 32 chunks of 64 KiB (chunk.max_size 65536), random bytes,
laid back to back; the expected ids are the chunks' own (a first call's
records), so the comparison runs and finds nothing.  Per --bundles count it
times, after --warmup calls, over --calls calls, and prints one JSON line:

  call_gibs       the whole zc_chunk_meta_compute call, payload resident in HBM
                  (extents and ids up, three kernels, records and statuses back;
                  wall clock of the C call, median)
  host_call_gibs  zc_chunk_meta_compute_host: the same plus the payload's upload
                  from pageable host memory
  meta_gibs       zc_extent_meta_kernel alone (rolling hash + first anchor), device time
  sha1_gibs       the existing zc_sha1_kernel alone over the same extents, device time
  other_ms        the call's time outside the two kernels

Beside them `host_core_gibs`: tests/meta/meta_core_check.cpp (zc_meta_core.h, the
scalar definition: SHA-1, rolling hash and anchor search per chunk) compiled -O2
here and run once over 16 MiB of the same chunks on one core."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = 65536
BUNDLE = 2 << 20
GIB = float(1 << 30)


def host_core_rate(tmp, sample):
    exe = os.path.join(tmp, "meta_core_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
                    os.path.join(ROOT, "tests", "meta", "meta_core_check.cpp"), "-o", exe], check=True)
    path = os.path.join(tmp, "sample")
    sample.tofile(path)
    out = subprocess.run([exe, "--time", str(W), str(W), path], capture_output=True, text=True, check=True).stdout
    chunks, nbytes, sec, _ = out.split()
    return int(nbytes) / float(sec) / GIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bundles", default="8,64,256", help="bundles of 2 MiB, comma separated")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch

    from zbackup_amd import Adopter, fill_splitmix64
    from zbackup_amd.chunker import SEED_DTYPE
    counts = [int(x) for x in a.bundles.split(",")]
    total = max(counts) * BUNDLE
    t = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill_splitmix64(t.data_ptr(), total, 41)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp, Adopter(W) as ad:
        core = None if a.no_host else host_core_rate(tmp, host[:16 << 20])
        for nb in counts:
            nbytes = nb * BUNDLE
            n = nbytes // W
            off = np.arange(n, dtype=np.uint64) * np.uint64(W)
            size = np.full(n, W, dtype=np.uint32)
            meta, _ = ad.chunk_meta(t.data_ptr(), nbytes, off, size)
            expect = np.zeros(n, dtype=SEED_DTYPE)
            expect["sha1"], expect["rolling"], expect["size"] = meta["sha1"], meta["rolling"], meta["size"]
            rows = {"device": [], "host": []}
            for form in ("device", "host"):
                for k in range(a.warmup + a.calls):
                    if form == "device":
                        got, status = ad.chunk_meta(t.data_ptr(), nbytes, off, size, expect=expect)
                    else:
                        got, status = ad.chunk_meta_host(host[:nbytes], off, size, expect=expect)
                    assert ad.n_bad == 0 and not status.any() and got.tobytes() == meta.tobytes()
                    if k >= a.warmup:
                        rows[form].append(ad.last_stats())
            med = lambda form, key: statistics.median(r[key] for r in rows[form])  # noqa: E731
            call, meta_ms, sha1_ms = med("device", "call_ms"), med("device", "meta_ms"), med("device", "sha1_ms")
            r = {"bundles": nb, "chunks": n, "bytes": nbytes, "calls": a.calls,
                 "anchored": int((meta["anchor"] != 0xFFFFFFFF).sum()),
                 "call_ms": round(call, 3), "call_gibs": round(nbytes / GIB / (call / 1e3), 1),
                 "host_call_ms": round(med("host", "call_ms"), 3),
                 "host_call_gibs": round(nbytes / GIB / (med("host", "call_ms") / 1e3), 2),
                 "meta_ms": round(meta_ms, 3), "meta_gibs": round(nbytes / GIB / (meta_ms / 1e3), 1),
                 "sha1_ms": round(sha1_ms, 3), "sha1_gibs": round(nbytes / GIB / (sha1_ms / 1e3), 1),
                 "other_ms": round(call - meta_ms - sha1_ms, 3),
                 "device": torch.cuda.get_device_name(0)}
            if core is not None:
                r.update(host_core_gibs=round(core, 3), speedup=round(r["call_gibs"] / core, 1))
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
