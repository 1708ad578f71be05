"""Rates of the LZMA bundle decode (zc_xz_decode) on one GPU, beside liblzma on
one host core over the same streams.

  python tools/xz_rate.py [--distinct 64] [--counts 1,8,64,512,4096] [--out FILE]

Payloads of 2 MiB (bundle.max_payload_size) of three kinds -- random (stored
chunks), the text-like generator of tests/lzo_inputs.py, half-duplicated --
compressed here with Python's lzma as Bundle::Creator does (preset 6, CRC64).
A call of n bundles repeats the `distinct` streams of its kind.  Per kind and
n: the call from device-resident bodies (first call, then the median of the
repeats: wall ms, payload GiB/s, the decode and check kernels' ms) and from
host memory (zc_xz_decode_host: bodies up, payloads back).  Each GPU step is
a process of its own under a time limit; a step that fails ends the run.
Prints one JSON object per line."""
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


def step(path, count, repeats):
    """One GPU step (a child process): n bundles of the streams in `path`."""
    import torch

    from zbackup_amd.bundle import BundleDecompressor
    with np.load(path) as z:
        bodies = [z[k].tobytes() for k in sorted(z.files)]
    bodies = [bodies[i % len(bodies)] for i in range(count)]
    in_size = [len(b) for b in bodies]
    in_off = np.concatenate([[0], np.cumsum([(n + 15) & ~15 for n in in_size])[:-1]]).astype(np.uint64)
    img = np.zeros(int(in_off[-1]) + ((in_size[-1] + 15) & ~15), dtype=np.uint8)
    for o, b in zip(in_off, bodies):
        img[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.empty(count * PAYLOAD, dtype=torch.uint8, device="cuda")
    out_off = np.arange(count, dtype=np.uint64) * PAYLOAD
    res = {"n": count, "body_bytes": int(sum(in_size))}
    with BundleDecompressor() as dec:
        wall, stats = [], []
        for _ in range(1 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode(d_in.data_ptr(), in_off, in_size, d_out.data_ptr(), out_off, [PAYLOAD] * count)
            wall.append((time.perf_counter() - t0) * 1e3)
            stats.append(dec.last_stats())
        med = float(np.median(wall[1:]))
        res.update(first_ms=round(wall[0], 2), wall_ms=round(med, 2),
                   gib_s=round(count * PAYLOAD / med / 1e-3 / (1 << 30), 3),
                   decode_ms=round(float(np.median([s["decode_ms"] for s in stats[1:]])), 2),
                   check_ms=round(float(np.median([s["check_ms"] for s in stats[1:]])), 3))
        del d_in, d_out
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        dec.decode_host(bodies, [PAYLOAD] * count)
        ms = (time.perf_counter() - t0) * 1e3
        res.update(host_ms=round(ms, 2), host_gib_s=round(count * PAYLOAD / ms / 1e-3 / (1 << 30), 3))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--counts", default="1,8,64,512,4096")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args.step[0], int(args.step[1]), args.repeats)
    from zbackup_amd import _build
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="setup", build_id=_build.source_digest(), payload_bytes=PAYLOAD, distinct=args.distinct)
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        for kind in KINDS:
            datas = [payload(kind, 100 + i) for i in range(args.distinct)]
            t0 = time.perf_counter()
            bodies = [lzma.compress(d, check=lzma.CHECK_CRC64, preset=6) for d in datas]
            enc_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            for b, d in zip(bodies, datas):
                assert lzma.decompress(b) == d
            dec_s = time.perf_counter() - t0
            emit(what="liblzma", kind=kind, streams=len(bodies), ratio=round(sum(map(len, bodies)) / (len(bodies) * PAYLOAD), 4),
                 encode_mb_s=round(len(bodies) * PAYLOAD / enc_s / 1e6, 1),
                 decode_ms_per_bundle=round(dec_s * 1e3 / len(bodies), 2),
                 decode_mb_s=round(len(bodies) * PAYLOAD / dec_s / 1e6, 1))
            path = os.path.join(tmp, kind + ".npz")
            np.savez(path, **{"b%04d" % i: np.frombuffer(b, dtype=np.uint8) for i, b in enumerate(bodies)})
            for count in [int(c) for c in args.counts.split(",")]:
                if failed:
                    break
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--step", path,
                       str(count)]
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
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
