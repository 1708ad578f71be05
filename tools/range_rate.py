"""Rates of the random-access restore (zc_range_read) on one GPU.

  python tools/range_rate.py [--gib 8] [--out FILE]

Two streams over the same resident payloads (2 MiB slots filled on the device):
  chunks  64 KiB chunks in shuffled order;
  tiny    4 KiB chunks, each followed by a 16-byte bytes_to_emit run, so a
          64 KiB piece walks 32 entries and a 4 KiB read almost always two.
Per stream: batches of 1 / 64 / 4,096 reads of 4 KiB / 128 KiB / 1 MiB at random
offsets, each batch timed on the host around the whole call (first pass: the
first call of that shape; then the median of the repeats) beside the call's
own kernel time; `Restorer.replay` of the whole stream on the same process and
data, which is how a range is obtained without the index; and a one-core CPU
walk: IndexedRestorer::saveData restated in numpy over host memory (every slot
read from one 2 MiB host buffer: the walk and the copies are what is timed).
Prints one JSON object per line."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOT = 2 << 20
READS = (1, 64, 4096)
SIZES = (4 << 10, 128 << 10, 1 << 20)


def streams(total, rng):
    """name -> (slot sizes, slot, off, sizes); the last slot of `tiny` is the run bytes."""
    n_slots = total // SLOT
    out = {}
    n = total // 65536
    order = rng.permutation(n)
    out["chunks"] = ([SLOT] * n_slots, (order // 32).astype(np.uint32), (order % 32).astype(np.uint64) * 65536,
                     np.full(n, 65536, dtype=np.uint64))
    n = total // 4096
    order = rng.permutation(n)
    slot = np.empty(2 * n, dtype=np.uint32)
    off = np.empty(2 * n, dtype=np.uint64)
    sizes = np.empty(2 * n, dtype=np.uint64)
    slot[0::2], off[0::2], sizes[0::2] = order // 512, (order % 512) * 4096, 4096
    slot[1::2], off[1::2], sizes[1::2] = n_slots, np.arange(n, dtype=np.uint64) * 16, 16
    out["tiny"] = ([SLOT] * n_slots + [16 * n], slot, off, sizes)
    return out


def cpu_walk(pos, slot, off, host_slot, reads, out):
    """saveData per read, one core: upper_bound, one step back, the clipped copies."""
    at = 0
    for o, n in reads:
        e = int(np.searchsorted(pos, np.uint64(o), side="right")) - 1
        end = o + n
        while n:
            a, b = int(pos[e]), int(pos[e + 1])
            lo, hi = max(a, o), min(b, end)
            if hi > lo:
                s = int(off[e]) % (len(host_slot) - 65536) + lo - a
                out[at:at + hi - lo] = host_slot[s:s + hi - lo]
                at += hi - lo
                n -= hi - lo
                o = hi
            e += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from zbackup_amd import RangeIndex, Restorer, _lib, fill_splitmix64
    from zbackup_amd.bundle import BundleCompressor
    from zbackup_amd.restore import RestorePlan
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    total = int(args.gib * (1 << 30)) // SLOT * SLOT
    rng = np.random.default_rng(31)
    d_pay = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill_splitmix64(d_pay.data_ptr(), total, 7)
    d_dst = torch.empty(max(READS) * max(SIZES), dtype=torch.uint8, device="cuda")
    host_slot = d_pay[:SLOT].cpu().numpy()
    emit(what="setup", build_id=_lib.build_id(), device=torch.cuda.get_device_name(0), payload_bytes=total)
    with BundleCompressor() as comp:
        for name, (slot_sizes, slot, off, sizes) in streams(total, rng).items():
            t0 = time.perf_counter()
            index = RangeIndex(slot_sizes, slot, off, sizes, comp=comp)
            create_ms = (time.perf_counter() - t0) * 1e3
            n_slots = total // SLOT
            for k in range(n_slots):
                index.set_slot(k, d_pay.data_ptr() + k * SLOT)
            if len(slot_sizes) > n_slots:  # the run bytes
                d_runs = torch.empty(slot_sizes[-1], dtype=torch.uint8, device="cuda")
                fill_splitmix64(d_runs.data_ptr(), slot_sizes[-1], 8)
                index.set_slot(n_slots, d_runs.data_ptr())
            emit(what="index", stream=name, entries=len(sizes), stream_bytes=index.total, create_ms=round(create_ms, 2))
            pos = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
            for size in SIZES:
                for count in READS:
                    offs = rng.integers(0, index.total - size, count)
                    reads = [(int(o), size) for o in offs]
                    dst_off = np.arange(count, dtype=np.uint64) * size
                    wall, kern, up = [], [], []
                    gc.collect()
                    gc.disable()  # as timeit does: no collector pass inside a timed call
                    for _ in range(1 + args.repeats):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        index.read(reads, d_dst.data_ptr(), dst_off)  # returns when the bytes are there
                        wall.append((time.perf_counter() - t0) * 1e3)
                        u, k, pieces = index.last_stats()
                        kern.append(k)
                        up.append(u)
                    gc.enable()
                    med = float(np.median(wall[1:]))
                    emit(what="batch", stream=name, reads=count, size=size, pieces=pieces,
                         first_ms=round(wall[0], 3), first_kernel_ms=round(kern[0], 3),
                         first_upload_ms=round(up[0], 3), wall_ms=round(med, 3), kernel_ms=round(float(np.median(kern[1:])), 3),
                         upload_ms=round(float(np.median(up[1:])), 3), us_per_read=round(med * 1e3 / count, 2),
                         gb_s=round(count * size / med / 1e6, 2),
                         kernel_gb_s=round(count * size / max(float(np.median(kern[1:])), 1e-6) / 1e6, 2))
                    if count == 64:  # the CPU walk on the same reads
                        out = np.empty(count * size, dtype=np.uint8)
                        t0 = time.perf_counter()
                        cpu_walk(pos, slot, off, host_slot, reads, out)
                        ms = (time.perf_counter() - t0) * 1e3
                        emit(what="cpu_walk", stream=name, reads=count, size=size, wall_ms=round(ms, 3),
                             us_per_read=round(ms * 1e3 / count, 2), gb_s=round(count * size / ms / 1e6, 2))
            # today's alternative: the whole stream through Restorer.replay (the runs' slot sits
            # outside the payload buffer, so the plan covers the chunk entries: all but 0.4 % of the bytes;
            # their places in the output stay unwritten)
            keep = slot < n_slots
            plan = RestorePlan()
            plan.src_off = slot[keep].astype(np.uint64) * SLOT + off[keep]
            plan.sizes = sizes[keep]
            plan.dst_off = pos[:-1][keep]
            plan.length = int(index.total)
            d_out = torch.empty(plan.length, dtype=torch.uint8, device="cuda")
            with Restorer(ctx=comp._ctx) as rs:
                wall = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rs.replay(plan, d_pay.data_ptr(), d_out.data_ptr(), plan.length)
                    wall.append((time.perf_counter() - t0) * 1e3)
            emit(what="replay", stream=name, stream_bytes=plan.length, extents=int(keep.sum()),
                 first_ms=round(wall[0], 2), wall_ms=round(float(np.median(wall[1:])), 2),
                 gb_s=round(plan.length / float(np.median(wall[1:])) / 1e6, 2))
            del d_out
            index.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
