"""Rates of the AES-128-CBC kernels (zc_aes.hip), beside libcrypto on one core.

  python tools/aes_rate.py [--chain-mib 2] [--chains 4096] [--calls 20] [--variants]

Times whole zc_aes128_cbc_encrypt / _decrypt calls with device events (recorded
on the default stream around each call, which the library orders its own
stream after; the call returns once its kernel has finished), after a warm-up,
over --calls calls, and prints one JSON line per case with the median and the
best rate in GiB/s of plaintext:

  decrypt and encrypt on --chains chains of --chain-mib MiB,
  encrypt on 64 chains and on one chain (the single-file latency),
  libcrypto's AES-128-CBC on one host core in 64 MiB calls.

Decrypt reads and writes every byte once, so its bound is half the HBM copy
rate; the line carries that fraction for --hbm-gibs (default 4000, a device
copy's read + write rate on the MI355X).  --variants repeats the device cases
with the plain 1 KiB table (ZC_AES_TABLE=shared) and with the lane-per-chain
encrypt kernel (ZC_AES_ENC=lane) in its launch shapes (ZC_AES_CPW chains per
wave, ZC_AES_PREFETCH=1 for one block of read-ahead)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_case(torch, comp, decrypt, d_in, d_out, n, length, calls, warmup, pad=0):
    off = np.arange(n, dtype=np.uint64) * np.uint64(length + pad)
    lens = np.full(n, length, dtype=np.uint64)
    key = bytes(range(16))
    fn = comp.aes_decrypt if decrypt else comp.aes_encrypt
    ms = []
    for k in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(key, d_in.data_ptr(), off, lens, d_out.data_ptr(), off)
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    gib = n * length / 2.0**30
    return {"median_gibs": round(gib / (statistics.median(ms) / 1e3), 3), "max_gibs": round(gib / (min(ms) / 1e3), 3),
            "median_ms": round(statistics.median(ms), 3), "chains": n, "chain_bytes": length, "gap_bytes": pad,
            "calls": calls}


def host_case(calls):
    from tests import aes_ref
    if not aes_ref.have_libcrypto():
        return None
    data = np.random.default_rng(1).integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
    key, iv = bytes(range(16)), bytes(16)
    out = {}
    for name, fn in (("encrypt", aes_ref.cbc_encrypt), ("decrypt", aes_ref.cbc_decrypt)):
        fn(key, iv, data[:1 << 20])
        s = []
        for _ in range(calls):
            t = time.perf_counter()
            fn(key, iv, data)
            s.append(time.perf_counter() - t)
        out[name] = {"median_gibs": round(len(data) / 2.0**30 / statistics.median(s), 3),
                     "max_gibs": round(len(data) / 2.0**30 / min(s), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain-mib", type=float, default=2.0)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-gibs", type=float, default=4000.0)
    ap.add_argument("--pad", type=int, default=4112,
                    help="bytes between chains (a multiple of 16): bundle files have no power-of-two sizes")
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch

    from zbackup_amd import fill_splitmix64
    from zbackup_amd.bundle import BundleCompressor
    length = int(a.chain_mib * (1 << 20)) // 16 * 16
    total = a.chains * (length + a.pad)
    d_in = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    fill_splitmix64(d_in.data_ptr(), total, 7)
    torch.cuda.synchronize()
    variants = [("replicated", {})]
    if a.variants:
        lane = {"ZC_AES_ENC": "lane"}  # the lane-per-chain encrypt kernel and its launch shapes
        variants += [("shared-table", {"ZC_AES_TABLE": "shared"}), ("lane-per-chain", lane),
                     ("lane-per-chain, 16 per wave", dict(lane, ZC_AES_CPW="16")),
                     ("lane-per-chain, 4 per wave", dict(lane, ZC_AES_CPW="4")),
                     ("lane-per-chain, 4 per wave, one block ahead", dict(lane, ZC_AES_CPW="4", ZC_AES_PREFETCH="1"))]
    with BundleCompressor() as comp:
        for vname, env in variants:
            os.environ.update(env)
            cases = [("decrypt", True, a.chains), ("encrypt", False, a.chains), ("encrypt", False, min(64, a.chains)),
                     ("encrypt", False, 1)]
            for name, dec, n in cases:
                if vname not in ("replicated", "shared-table") and (dec or n == 1):
                    continue  # the variant changes the encrypt launch only
                r = device_case(torch, comp, dec, d_in, d_out, n, length, a.calls, a.warmup, a.pad)
                r.update(case=name, variant=vname, device=torch.cuda.get_device_name(0))
                if dec:
                    r["of_hbm_bound"] = round(r["median_gibs"] / (a.hbm_gibs / 2), 3)
                print(json.dumps(r), flush=True)
            for k in env:
                del os.environ[k]
    if not a.no_host:
        h = host_case(max(3, a.calls // 4))
        print(json.dumps({"case": "libcrypto one core", "result": h}), flush=True)


if __name__ == "__main__":
    main()
