"""Rates of the LZMA bundle encode (zc_xz_encode) on one GPU, beside liblzma on
one host core over the same payloads.

  python tools/xzenc_rate.py [--distinct 16] [--counts 1,8,64,512,4096] [--out FILE]

Payloads of 2 MiB (bundle.max_payload_size) of three kinds -- random, the
text-like generator of tests/lzo_inputs.py, half-duplicated.  A call of n
bundles repeats the `distinct` payloads of its kind.  Per kind: liblzma
(Python's lzma.compress, one core) at preset 6, what Bundle::Creator runs, and
at preset 0, on `--cpu-samples` payloads (seconds per bundle and ratio), and
the framed lzo1x_1 size where liblzo2 is here.  Per kind and n: the call from
device-resident payloads (first call, then the median of the repeats: wall ms,
payload GiB/s, the match, coding and check kernels' ms, the ratio) and, up to
`--host-max` bundles, from host memory (zc_xz_encode_host: payloads up,
streams back).  The first stream of every step is decoded with lzma and
compared.  Each GPU step is a process of its own under a time limit; a step
that fails ends the run.  Prints one JSON object per line."""
import argparse
import json
import lzma
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAYLOAD = 2 << 20
KINDS = ("random", "text", "halfdup")


def payload(kind, seed):
    from tests import lzo_inputs
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes()
    if kind == "text":
        return lzo_inputs.text(PAYLOAD, rng).tobytes()
    h = rng.integers(0, 256, PAYLOAD // 2, dtype=np.uint8)
    return np.concatenate([h, h]).tobytes()


def step(path, count, repeats, host_max):
    """One GPU step (a child process): n bundles of the payloads in `path`."""
    import torch

    from zbackup_amd.bundle import BundleCompressor
    with np.load(path) as z:
        distinct = [z[k] for k in sorted(z.files)]
    d_distinct = torch.from_numpy(np.concatenate(distinct)).cuda()
    reps = (count + len(distinct) - 1) // len(distinct)
    d_pay = d_distinct.repeat(reps)[:count * PAYLOAD].contiguous()
    del d_distinct
    res = {"n": count}
    with BundleCompressor() as bc:
        cap = (bc.xz_capacity(PAYLOAD) + 15) & ~15
        d_out = torch.empty(count * cap, dtype=torch.uint8, device="cuda")
        pay_off = np.arange(count, dtype=np.uint64) * PAYLOAD
        out_off = np.arange(count, dtype=np.uint64) * cap
        wall, stats, sizes = [], [], None
        for _ in range(1 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sizes = bc.compress_xz(d_pay.data_ptr(), pay_off, [PAYLOAD] * count, d_out.data_ptr(), out_off)
            wall.append((time.perf_counter() - t0) * 1e3)
            stats.append(bc.xz_last_stats())
        first = d_out[:int(sizes[0])].cpu().numpy().tobytes()
        assert lzma.decompress(first) == distinct[0].tobytes()
        med = float(np.median(wall[1:])) if repeats else wall[0]
        tail = stats[1:] if repeats else stats
        res.update(first_ms=round(wall[0], 2), wall_ms=round(med, 2),
                   gib_s=round(count * PAYLOAD / med / 1e-3 / (1 << 30), 4),
                   ratio=round(float(sizes.sum()) / (count * PAYLOAD), 4),
                   match_ms=round(float(np.median([s["match_ms"] for s in tail])), 2),
                   code_ms=round(float(np.median([s["code_ms"] for s in tail])), 2),
                   check_ms=round(float(np.median([s["check_ms"] for s in tail])), 3))
        del d_pay, d_out
        torch.cuda.empty_cache()
        if count <= host_max:
            host = [distinct[i % len(distinct)].tobytes() for i in range(count)]
            t0 = time.perf_counter()
            bodies = bc.compress_xz_host(host)
            ms = (time.perf_counter() - t0) * 1e3
            assert bodies[0] == first
            res.update(host_ms=round(ms, 2), host_gib_s=round(count * PAYLOAD / ms / 1e-3 / (1 << 30), 4))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--counts", default="1,8,64,512,4096")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cpu-samples", type=int, default=2)
    ap.add_argument("--host-max", type=int, default=512)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args.step[0], int(args.step[1]), args.repeats, args.host_max)
    from zbackup_amd import _build
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(what="setup", build_id=_build.source_digest(), payload_bytes=PAYLOAD, distinct=args.distinct)
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        for kind in KINDS:
            datas = [payload(kind, 100 + i) for i in range(args.distinct)]
            cpu = {}
            for preset in (6, 0):
                t0 = time.perf_counter()
                out = [lzma.compress(d, check=lzma.CHECK_CRC64, preset=preset) for d in datas[:args.cpu_samples]]
                s = time.perf_counter() - t0
                cpu["preset%d_s_per_bundle" % preset] = round(s / len(out), 3)
                cpu["preset%d_ratio" % preset] = round(sum(map(len, out)) / (len(out) * PAYLOAD), 4)
            try:
                from oracle import lzo_oracle
                cpu["lzo1x_1_framed_ratio"] = round(len(lzo_oracle.frame(datas[0])) / PAYLOAD, 4)
            except Exception as e:
                cpu["lzo1x_1_framed_ratio"] = None
                cpu["lzo_note"] = str(e)[:80]
            emit(what="liblzma", kind=kind, samples=args.cpu_samples, **cpu)
            path = os.path.join(tmp, kind + ".npz")
            np.savez(path, **{"p%04d" % i: np.frombuffer(d, dtype=np.uint8) for i, d in enumerate(datas)})
            for count in [int(c) for c in args.counts.split(",")]:
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--host-max",
                       str(args.host_max), "--step", path, str(count)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    emit(what="gpu", kind=kind, n=count, error=f"no result within {args.limit} s")
                    failed = True
                    break
                if out.returncode != 0:
                    emit(what="gpu", kind=kind, n=count, error=f"exit status {out.returncode}", stderr=out.stderr[-800:])
                    failed = True
                    break
                emit(what="gpu", kind=kind, **json.loads(out.stdout.strip().split("\n")[-1]))
            if failed:
                break
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
