"""Rates of the resident chunk index (zc_resolve.hip): the build, and the
resolve of a backup against it, beside Restorer.plan's Python dict.

  python tools/resolve_rate.py [--records 1,16] [--entries 1024,131072,1048576] [--calls 5]
                               [--plan-limit 60] [--out profiles/resolve_rate_<build>.jsonl]

The input: --records million (2^20) records of random ids in bundles of 512
records, sizes 1..65,536, with 0 % and with 1 % of the records repeating the id
of a record 600 places earlier (another bundle: two bundles hold the id).  One
JSON line per build -- zc_chunk_index_create_arrays from pageable host arrays:
the median wall time of --calls calls after one warm-up and the device time of
its kernels (zc_resolve_last_stats) -- and one per (build, entries): a
BackupInstruction stream of that many chunk_to_emit entries drawn from the
records, resolved --calls times: `resolve_wall_ms` is the zc_restore_resolve
call with its upload and read-back, `resolve_device_ms` its kernels,
`plan_index_ms` the whole Restorer.plan_index (parse, resolve, fetch, numpy).

Beside it `plan_ms`: Restorer.plan on the same stream and the same bundles as
Python lists (making the lists is timed apart, `lists_s`), run once, and no
more after a run took longer than --plan-limit seconds or at more than 2^20
records; the lines say where it was not run."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUNDLE = 512


def make_input(n, dup_share, seed=5):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    sizes = rng.integers(1, 65537, n).astype(np.uint32)
    if dup_share:
        j = 600 + rng.choice(n - 600, int(n * dup_share), replace=False)
        ids[j], sizes[j] = ids[j - 600], sizes[j - 600]  # from the values as drawn: a copy's source may itself change
    first = np.concatenate([np.arange(0, n, BUNDLE), [n]]).astype(np.uint64)
    return ids, sizes, first


def make_stream(ids, e, seed=9):
    """e BackupInstructions of one chunk_to_emit each: 1A 0A 18 <24-byte id>."""
    rng = np.random.default_rng(seed)
    s = np.zeros((e, 27), dtype=np.uint8)
    s[:, 0], s[:, 1], s[:, 2] = 26, 0x0A, 24
    s[:, 3:] = ids[rng.integers(0, len(ids), e)]
    return s.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1,16", help="millions (2^20) of records, comma separated")
    ap.add_argument("--entries", default="1024,131072,1048576")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--plan-limit", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from zbackup_amd import ChunkIndex, Restorer, _build, parse_backup_data
    from zbackup_amd.bundle import BundleCompressor
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="setup", build_id=_build.source_digest(), device=torch.cuda.get_device_name(0), bundle_records=BUNDLE,
         calls=a.calls)
    plan_stopped = None
    with BundleCompressor() as comp:
        for m in [float(x) for x in a.records.split(",")]:
            n = int(m * (1 << 20))
            for dup_share in (0.0, 0.01):
                ids, sizes, first = make_input(n, dup_share)
                wall, dev = [], []
                cx = None
                for k in range(a.calls + 1):
                    if cx is not None:
                        cx.close()
                    t = time.perf_counter()
                    cx = ChunkIndex.from_arrays(ids, sizes, first, ctx=comp._ctx)
                    if k:
                        wall.append((time.perf_counter() - t) * 1e3)
                        dev.append(cx.last_stats()["build_ms"])
                st, counts = cx.last_stats(), cx.counts()
                emit(what="build", records=n, bundles=len(first) - 1, dup_share=dup_share, ids=counts["ids"],
                     flagged=counts["flagged"], build_wall_ms=round(statistics.median(wall), 2),
                     build_device_ms=round(statistics.median(dev), 3), table_slots=st["table_slots"],
                     max_probe=st["max_probe"],
                     records_per_s_device=round(n / (statistics.median(dev) / 1e3)))
                bundles, lists_s = None, None
                if n <= 1 << 20 and plan_stopped is None:
                    t = time.perf_counter()
                    blobs = [ids[r].tobytes() for r in range(n)]
                    bundles = [[(blobs[r], int(sizes[r])) for r in range(int(first[b]), int(first[b + 1]))]
                               for b in range(len(first) - 1)]
                    lists_s = time.perf_counter() - t
                for e in [int(x) for x in a.entries.split(",")]:
                    stream = make_stream(ids, e)
                    ins = parse_backup_data(stream)
                    rw, rd, pw = [], [], []
                    for k in range(a.calls + 1):
                        t = time.perf_counter()
                        r = cx.resolve(ins, len(stream))
                        t1 = time.perf_counter()
                        if k:
                            rw.append((t1 - t) * 1e3)
                            rd.append(cx.last_stats()["resolve_ms"])
                        t = time.perf_counter()
                        plan = Restorer.plan_index(stream, cx)
                        if k:
                            pw.append((time.perf_counter() - t) * 1e3)
                    assert r.n_missing == 0 and r.n_entries == e and plan.length == r.length
                    line = dict(what="resolve", records=n, dup_share=dup_share, entries=e, used_bundles=r.n_used,
                                resolve_wall_ms=round(statistics.median(rw), 3),
                                resolve_device_ms=round(statistics.median(rd), 3),
                                plan_index_ms=round(statistics.median(pw), 2), max_probe=cx.last_stats()["max_probe"])
                    if bundles is not None and plan_stopped is None:
                        t = time.perf_counter()
                        old = Restorer.plan(stream, bundles)
                        plan_s = time.perf_counter() - t
                        assert old.length == plan.length and sorted(old.used) == plan.used
                        line.update(plan_ms=round(plan_s * 1e3, 1), lists_s=round(lists_s, 1),
                                    speedup_over_plan=round(plan_s * 1e3 / statistics.median(pw), 1))
                        if plan_s > a.plan_limit:
                            plan_stopped = f"a run took {plan_s:.0f} s"
                    else:
                        line.update(plan_ms=None, plan_not_run=plan_stopped or f"{n} records as Python lists")
                    emit(**line)
                cx.close()
                del bundles
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
