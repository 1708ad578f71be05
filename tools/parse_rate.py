"""Rates of the restore that stays in HBM (zc_instr.hip, zc_resolve.hip): a
BackupInstruction stream that lies in device memory, parsed, resolved and
replayed there, beside the only route the host parser leaves.

  python tools/parse_rate.py [--entries 1024,131072,1048576] [--calls 5]
                             [--out profiles/parse_rate_<build>.jsonl]

The index: 2^20 records of random ids in bundles of 512 records, sizes 1..1,024
(short chunks, so that a million entries restore to half a GiB and not to 32).
The streams: that many chunk_to_emit entries drawn from the records; 8 MiB of
zero bytes (every position an empty message); one bytes_to_emit of 64 MiB.  The
payloads and the stream lie in one device buffer.  Per stream, the median of
--calls runs after one warm-up of

  (a) zc_parse_instructions_device, zc_restore_resolve_device, zc_restore_replay:
      each call's wall time, and the parse's device time by step
      (zc_instr_last_stats);
  (b) the stream copied to the host, zc_parse_instructions, zc_restore_resolve
      with zc_restore_plan_fetch, and zc_bundle_scatter over the fetched lists:
      each step's wall time.

Both routes run in one process on the same data and write the same bytes (the
outputs are compared once).  No counter profile belongs in the same run."""
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
RECORDS = 1 << 20


def chunk_stream(ids, e, seed=9):
    """e BackupInstructions of one chunk_to_emit each: 1A 0A 18 <24-byte id>."""
    rng = np.random.default_rng(seed)
    s = np.zeros((e, 27), dtype=np.uint8)
    s[:, 0], s[:, 1], s[:, 2] = 26, 0x0A, 24
    s[:, 3:] = ids[rng.integers(0, len(ids), e)]
    return s.tobytes()


def one_bytes_message(n):
    def varint(v):
        out = b""
        while v >= 0x80:
            out += bytes([v & 0x7f | 0x80])
            v >>= 7
        return out + bytes([v])
    body = b"\x12" + varint(n)
    return varint(len(body) + n) + body + bytes(np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8))


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1024,131072,1048576")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from zbackup_amd import ChunkIndex, Restorer, _build, parse_backup_data
    from zbackup_amd.bundle import BundleCompressor
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="setup", build_id=_build.source_digest(), device=torch.cuda.get_device_name(0), records=RECORDS,
         bundle_records=BUNDLE, calls=a.calls)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 256, (RECORDS, 24), dtype=np.uint8)
    sizes = rng.integers(1, 1025, RECORDS).astype(np.uint32)
    first = np.concatenate([np.arange(0, RECORDS, BUNDLE), [RECORDS]]).astype(np.uint64)
    streams = [(f"{e} chunk entries", chunk_stream(ids, e)) for e in (int(x) for x in a.entries.split(","))]
    streams += [("8 MiB of zeros", bytes(8 << 20)), ("one bytes_to_emit of 64 MiB", one_bytes_message(64 << 20))]
    with BundleCompressor() as comp, Restorer(ctx=comp._ctx) as rs, \
            ChunkIndex.from_arrays(ids, sizes, first, ctx=comp._ctx) as cx:
        pay_size, _ = cx.bundles()
        pay_off = np.concatenate([[0], np.cumsum((pay_size + np.uint64(15)) & ~np.uint64(15))]).astype(np.uint64)
        for name, stream in streams:
            n = len(stream)
            instr_off = int(pay_off[-1])
            work = torch.empty(instr_off + n + 16, dtype=torch.uint8, device="cuda:0")
            work[:instr_off].random_(0, 256)
            work[instr_off:instr_off + n] = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy())
            d_work = work.data_ptr()
            d_stream = d_work + instr_off
            t_a = {k: [] for k in ("parse", "resolve", "replay", "hop", "exit", "chain", "emit")}
            t_b = {k: [] for k in ("download", "parse", "resolve_fetch", "scatter")}
            out_a = out_b = None
            for k in range(a.calls + 1):
                torch.cuda.synchronize()
                # (a)
                t0 = time.perf_counter()
                ins = rs.parse_device(d_stream, n)
                t1 = time.perf_counter()
                plan = rs.plan_device(ins, cx)
                t2 = time.perf_counter()
                if out_a is None:
                    out_a = torch.zeros(plan.length + 16, dtype=torch.uint8, device="cuda:0")
                    out_b = torch.zeros(plan.length + 16, dtype=torch.uint8, device="cuda:0")
                ptrs = [d_work + int(pay_off[int(b)]) for b in plan.used] + [d_stream]
                t3 = time.perf_counter()
                rs.replay_device(plan, ptrs, out_a.data_ptr(), plan.length)
                t4 = time.perf_counter()
                st = rs.parse_last_stats()
                entries, messages, used, length = ins.n_entries, ins.n_messages, plan.n_used, plan.length
                plan.close()
                ins.close()
                # (b)
                t5 = time.perf_counter()
                host = work[instr_off:instr_off + n].cpu().numpy().tobytes()
                t6 = time.perf_counter()
                hins = parse_backup_data(host)
                t7 = time.perf_counter()
                r = cx.resolve(hins, n)
                t8 = time.perf_counter()
                base = np.concatenate([pay_off[r.used.astype(np.int64)], [instr_off]]).astype(np.uint64)
                keep = r.size > 0
                src = (base[r.slot] + r.off)[keep]
                t9 = time.perf_counter()
                if keep.any():
                    comp.scatter(d_work, src, r.size[keep], out_b.data_ptr(), r.dst[keep])
                t10 = time.perf_counter()
                if k == 0:
                    assert r.length == length and torch.equal(out_a, out_b), name
                    continue
                for key, v in (("parse", t1 - t0), ("resolve", t2 - t1), ("replay", t4 - t3)):
                    t_a[key].append(v * 1e3)
                for key in ("hop", "exit", "chain", "emit"):
                    t_a[key].append(st[key + "_ms"])
                for key, v in (("download", t6 - t5), ("parse", t7 - t6), ("resolve_fetch", t8 - t7),
                               ("scatter", t10 - t8)):
                    t_b[key].append(v * 1e3)
            total_a = med([x + y + z for x, y, z in zip(t_a["parse"], t_a["resolve"], t_a["replay"])])
            total_b = med([sum(v) for v in zip(*t_b.values())])
            emit(what="stream", stream=name, bytes=n, entries=entries, messages=messages, used_bundles=used,
                 restored_bytes=length, tiles=st["tiles"], chain_hops=st["chain_hops"],
                 a_parse_ms=med(t_a["parse"]), a_resolve_ms=med(t_a["resolve"]), a_replay_ms=med(t_a["replay"]),
                 a_total_ms=total_a, a_exit_ms=med(t_a["exit"]), a_chain_ms=med(t_a["chain"]),
                 a_emit_ms=med(t_a["emit"]), b_download_ms=med(t_b["download"]), b_parse_ms=med(t_b["parse"]),
                 b_resolve_fetch_ms=med(t_b["resolve_fetch"]), b_scatter_ms=med(t_b["scatter"]), b_total_ms=total_b,
                 b_over_a=round(total_b / total_a, 2))
            del work, out_a, out_b
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
