"""CPU tests of repository adoption (chunk metadata from bundle payloads):

* zc_meta_core.h -- the scalar definition of a chunk's record the kernels of
  zc_meta.hip are checked against -- compiled for the host (under ASan + UBSan
  where that links) with a main of its own, run over chunk files written here
  and compared with the plain-Python restatement tests/meta_ref.py;
* the sidecar file: write_sidecar -> read_sidecar -> the zbackup-side binding's
  own reader (tests/adapter/sidecar_read.cpp);
* AdoptReport's bookkeeping and the bundle layout on hand-made inputs;
* the new symbols, and the argument errors zc_chunk_meta_compute finds before
  it looks at its context: they need no device."""
import ctypes
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import meta_ref
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zc_chunk_meta_compute", "zc_chunk_meta_compute_host", "zc_meta_last_stats"]
SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 1023, 1024, 1025, 4095, 4096]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path_factory.mktemp("meta") / "meta_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "meta", "meta_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


def anchored(W, positions, size=None):
    """Zeros with the single byte 0xFF at q - 14 for each q: st(q) = 0x7F80, the
    only positions at or above the threshold of W = 4096."""
    b = bytearray(W if size is None else size)
    for q in positions:
        b[q - 14] = 0xFF
    return bytes(b)


def core_records(exe, tmp_path, W, chunks):
    paths = []
    for i, c in enumerate(chunks):
        p = tmp_path / f"c{W}_{i}"
        p.write_bytes(c)
        paths.append(str(p))
    out = subprocess.run([exe, str(W)] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = np.zeros(len(chunks), dtype=meta_ref.META_DTYPE)
    lines = out.stdout.split("\n")[:len(chunks)]
    for i, line in enumerate(lines):
        sha, rolling, size, adef, anchor, gear, fp = line.split()
        rec["sha1"][i] = np.frombuffer(bytes.fromhex(sha), dtype=np.uint8)
        rec[i]["rolling"], rec[i]["size"], rec[i]["anchor_def"] = int(rolling), int(size), int(adef)
        rec[i]["anchor"], rec[i]["gear"], rec[i]["fingerprint"] = int(anchor), int(gear), int(fp)
    return rec


def test_reference_helper_on_known_values():
    """meta_ref against values that do not come from it."""
    assert meta_ref.rolling(b"") == 1 and meta_ref.rolling(b"\x05") == 257 + 5
    assert meta_ref.rolling(b"\x01\x02") == 257 * 257 + 257 + 2
    assert meta_ref.anchor_lo(4096) == 0x7F00 and meta_ref.anchor_lo(65536) == 0x7FF0
    assert meta_ref.anchor_lo(64) == meta_ref.anchor_lo(63) == 0x7000
    b = anchored(4096, [700])
    assert meta_ref.st(b, 700) == 0x7F80 and meta_ref.st(b, 699) == 0 and meta_ref.st(b, 702) == 0xFF00
    assert meta_ref.first_anchor(b, 4096) == (700, 0x7F80 << 16, 0)
    assert meta_ref.first_anchor(anchored(4096, [62]), 4096) == (meta_ref.NO_ANCHOR, 0, 0)
    assert meta_ref.first_anchor(anchored(4096, [62, 700]), 4096)[0] == 700
    assert meta_ref.first_anchor(anchored(4096, [100, 101]), 4096)[0] == 100
    assert meta_ref.first_anchor(anchored(4096, [500], size=4095), 4096) == (meta_ref.NO_ANCHOR, 0, 0)
    header = open(os.path.join(ROOT, "include", "zchunk.h")).read()
    for name, ref in (("ZC_META_BAD_SHA1", meta_ref.BAD_SHA1), ("ZC_META_BAD_ROLLING", meta_ref.BAD_ROLLING),
                      ("ZC_META_BAD_SIZE", meta_ref.BAD_SIZE)):
        assert int(re.search(r"\b%s = (\d+)" % name, header).group(1)) == ref == getattr(_lib, name)


def test_core_matches_the_reference_on_the_edge_set(check_exe, tmp_path):
    exe, sanitized = check_exe
    print("sanitized" if sanitized else "NOT sanitized")
    rng = np.random.default_rng(5)
    W = 4096
    chunks = []
    for n in SIZES:
        chunks += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n), b"\xff" * n]
    for q in (62, 63, 64, 1023, 1024, 1025, 1039, 1040, 4094, 4095):
        chunks.append(anchored(W, [q]))
    chunks += [anchored(W, [62, 700]), anchored(W, [100, 101]), anchored(W, [500], size=4095)]
    got = core_records(exe, tmp_path, W, chunks)
    want = meta_ref.records(chunks, W)
    assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0]
    found = got["anchor"][-13:].tolist()
    assert found == [meta_ref.NO_ANCHOR, 63, 64, 1023, 1024, 1025, 1039, 1040, 4094, 4095, 700, 100,
                     meta_ref.NO_ANCHOR]
    assert (got["anchor_def"] == _lib.load().zc_anchor_def(W)).all()


@pytest.mark.parametrize("W", [63, 64, 65536])
def test_core_at_other_chunk_sizes(check_exe, tmp_path, lib, W):
    exe, _ = check_exe
    rng = np.random.default_rng(W)
    chunks = [rng.integers(0, 256, W, dtype=np.uint8).tobytes() for _ in range(40 if W < 100 else 3)]
    chunks += [bytes(W), rng.integers(0, 256, W - 1, dtype=np.uint8).tobytes()]
    got = core_records(exe, tmp_path, W, chunks)
    want = meta_ref.records(chunks, W)
    assert got.tobytes() == want.tobytes()
    assert (got["anchor_def"] == lib.zc_anchor_def(W)).all()
    if W == 63:
        assert (got["anchor"] == meta_ref.NO_ANCHOR).all()  # no position at or past 63
    if W == 64:
        assert set(got["anchor"].tolist()) <= {63, meta_ref.NO_ANCHOR}  # the one position there is


def test_core_compare(check_exe):
    out = subprocess.run([check_exe[0], "--compare"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert not set(NEW_SYMBOLS) - exported
    assert not set(NEW_SYMBOLS) - set(_lib.EXPORTS)
    assert lib.zc_abi_version() == 5  # detected by symbol, not by version
    import zbackup_amd
    for name in ("Adopter", "AdoptReport", "write_sidecar", "read_sidecar"):
        assert getattr(zbackup_amd, name) is not None
    names = {os.path.basename(p) for p in _build.SOURCES + _build.HEADERS}
    assert {"zc_meta.hip", "zc_meta_core.h"} <= names  # the build id covers the new sources


def _call(lib, fn="zc_chunk_meta_compute", n=2, payload_bytes=100, off=(0, 10), size=(10, 20), payload=True,
          has_off=True, has_size=True, has_out=True, expect=False, status=True, n_bad=True):
    """One call with no context: every fault below is found before the context is looked at."""
    keep = [np.zeros(max(payload_bytes, 1), dtype=np.uint8), np.array(off, dtype=np.uint64),
            np.array(size, dtype=np.uint32), np.zeros(max(n, 1), dtype=meta_ref.META_DTYPE),
            np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1) * 32, dtype=np.uint8)]
    bad = ctypes.c_size_t(77)
    rc = getattr(lib, fn)(None, keep[0].ctypes.data if payload else None, payload_bytes,
                          keep[1].ctypes.data if has_off else None, keep[2].ctypes.data if has_size else None, n,
                          keep[5].ctypes.data if expect else None, keep[3].ctypes.data if has_out else None,
                          keep[4].ctypes.data if status else None, ctypes.byref(bad) if n_bad else None)
    return rc, lib.zc_last_error(None).decode()


@pytest.mark.parametrize("fn", ["zc_chunk_meta_compute", "zc_chunk_meta_compute_host"])
@pytest.mark.parametrize("kw, text", [
    (dict(payload=False), "null payload, off, size or out with n > 0"),
    (dict(has_off=False), "null payload, off, size or out with n > 0"),
    (dict(has_size=False), "null payload, off, size or out with n > 0"),
    (dict(has_out=False), "null payload, off, size or out with n > 0"),
    (dict(size=(10, 0)), "size[1] is 0"),
    (dict(off=(0, 81)), "chunk 1 [81, +20) ends past the payload's 100 bytes"),
    (dict(off=(0, 1 << 63), size=(10, 1)), "ends past the payload's 100 bytes"),
    (dict(off=(0, (1 << 64) - 5), size=(10, 20)), "ends past the payload's 100 bytes"),  # off + size wraps
    (dict(expect=True, status=False, n_bad=False), "expected ids given, but neither status nor n_bad"),
    (dict(), "null context"),
    (dict(off=(0, 80)), "null context"),  # ends exactly at payload_bytes: legal
    (dict(n=0, payload=False, has_off=False, has_size=False, has_out=False), "null context"),
    (dict(expect=True, status=False), "null context"),
    (dict(expect=True, n_bad=False), "null context"),
])
def test_bad_arguments_are_found_before_the_context_is_used(lib, fn, kw, text):
    rc, msg = _call(lib, fn=fn, **kw)
    assert rc == _lib.ZC_ERR_ARG
    assert msg.startswith(fn + ": ") and text in msg, msg


def test_last_stats_without_a_context(lib):
    d = ctypes.c_double(7.0)
    assert lib.zc_meta_last_stats(None, ctypes.byref(d), None, None) == _lib.ZC_ERR_ARG
    assert b"zc_meta_last_stats" in lib.zc_last_error(None) and d.value == 7.0


def _some_meta(n, W=4096, seed=9):
    rng = np.random.default_rng(seed)
    return meta_ref.records([rng.integers(0, 256, W, dtype=np.uint8).tobytes() for _ in range(n)], W)


def test_sidecar_round_trip_through_both_readers(lib, tmp_path):
    from tests.adapter import build as adapter_build
    from zbackup_amd import ZcError, read_sidecar, write_sidecar
    meta = _some_meta(7)
    d = tmp_path / "zchunk"
    path = write_sidecar(str(d), meta)
    data = open(path, "rb").read()
    assert os.path.basename(path) == hashlib.sha256(data[:-32]).hexdigest() == data[-32:].hex()
    assert data[:24] == b"ZCMETA01" + struct.pack("<IIQ", 48, 0, 7) and len(data) == 24 + 7 * 48 + 32
    assert os.listdir(d) == [os.path.basename(path)]  # no temporary file left
    back = read_sidecar(path)
    assert back.dtype == meta.dtype and back.tobytes() == meta.tobytes()
    assert write_sidecar(str(d), meta) == path  # the same records: the same file
    assert write_sidecar(str(d), meta[:0]) is None
    # the binding's reader takes the file
    exe = adapter_build.build_sidecar_reader(out=str(tmp_path / "sidecar_read"))
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "7"
    assert out[1:8] == ["%016x %d" % (int(r["rolling"]), int(r["anchor"])) for r in meta]
    # damaged, truncated or foreign files are refused
    for k, damaged in enumerate((data[:100] + bytes([data[100] ^ 1]) + data[101:], data[:-1], b"ZCMETA02" + data[8:],
                                 data[:8] + struct.pack("<I", 40) + data[12:])):
        p = tmp_path / f"bad{k}"
        p.write_bytes(damaged)
        with pytest.raises(ZcError):
            read_sidecar(str(p))


def test_bundle_layout_and_report_bookkeeping():
    from zbackup_amd import ZcError
    from zbackup_amd.adopt import build_report, bundle_layout
    W = 4096
    blob = lambda k: bytes([k] * 16) + struct.pack("<Q", 1000 + k)  # noqa: E731
    bundles = [[(blob(1), W), (blob(2), 100)], [], [(blob(3), W), (blob(4), W), (blob(5), 7)]]
    payloads = [bytes(W + 100), b"", bytes(2 * W + 7)]
    off, size, expect, first = bundle_layout(bundles, payloads)
    assert off.tolist() == [0, W, W + 100, 2 * W + 100, 3 * W + 100] and size.tolist() == [W, 100, W, W, 7]
    assert first == [0, 2, 2, 5]
    assert expect["rolling"].tolist() == [1001, 1002, 1003, 1004, 1005] and expect["size"].tolist() == size.tolist()
    assert bytes(expect["sha1"][3]) == bytes([4] * 16)
    with pytest.raises(ZcError, match="bundle 2 decoded to 8198 bytes, its chunks take 8199"):
        bundle_layout(bundles, [payloads[0], b"", bytes(2 * W + 6)])
    with pytest.raises(ZcError, match="bundle 0: a chunk id of 23 bytes"):
        bundle_layout([[(bytes(23), 5)]], [bytes(5)])
    with pytest.raises(ZcError, match="3 bundles, 2 payloads"):
        bundle_layout(bundles, payloads[:2])
    meta = _some_meta(5)
    meta["size"][1], meta["size"][4] = 100, 7
    status = np.array([0, 0, 3, 0, 4], dtype=np.uint8)
    r = build_report(first, meta, status, W)
    assert r.chunks == 5 and r.bytes == 3 * W + 107
    assert r.bad == [(2, 0, 3), (2, 2, 4)]
    assert r.meta.tobytes() == meta[[0, 3]].tobytes()  # size W and status 0 only, in bundle order
    empty = build_report([0], meta[:0], status[:0], W)
    assert empty.chunks == 0 and empty.bytes == 0 and empty.bad == [] and len(empty.meta) == 0
