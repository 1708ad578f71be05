"""CPU tests of zc_ser_core.h, the definitions the device serializer's kernels
(zc_ser.hip) and zc_serialized_size share:

* tests/ser/ser_core_check.cpp, a program of its own built with
  -fsanitize=address,undefined, runs the length function, the header and
  chunk-id writers and the run decomposition single-threaded -- the walk the
  write kernel makes, group by group and run by run -- against a plain
  serializer written from Message::serialize, at the payload lengths where the
  outer or the inner varint grows (each with one below and one above), and
  checks that every output byte is written exactly once;
* zc_serialized_size, the same length function behind the C ABI, against the
  sum of len(serialize_instruction(...)) of the Python mirror.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from zbackup_amd import RECORD_DTYPE, _build, _lib, chunk_id_blob, serialize_instruction, serialized_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the outer and inner varint steps of a bytes_to_emit message
STEPS = [0, 1, 125, 126, 127, 128, 16381, 16383, 16384, 2097148, 2097151, 2097152, (1 << 28) - 6, 1 << 28]
SIZES = sorted({s + d for s in STEPS for d in (-1, 0, 1) if s + d >= 0})


def test_core_matches_a_plain_serializer(tmp_path):
    exe = str(tmp_path / "ser_core_check")
    subprocess.run(["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ser", "ser_core_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    m = re.search(r"^ok (\d+) checks$", out.stdout, re.M)
    assert m and int(m.group(1)) > 10000, out.stdout[-2000:]


def _message_len(kind, size):
    """len(serialize_instruction(...)) without building a payload of `size` bytes."""
    if kind != _lib.ZC_BYTES:
        return len(serialize_instruction(chunk_blob=chunk_id_blob(bytes(16), 0)))
    if size <= 70000:
        return len(serialize_instruction(raw=bytes(size)))
    return _by_definition(size)  # equal to the mirror up to 2 MiB: test_by_definition_is_the_python_mirror


def _by_definition(size):
    """message.cc:16-23 for one bytes_to_emit field of `size` bytes: varint(body) + tag + varint(size) + size."""
    def varint_len(v):
        k = 1
        while v >= 0x80:
            v >>= 7
            k += 1
        return k
    body = 1 + varint_len(size) + size
    return varint_len(body) + body


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_by_definition_is_the_python_mirror():
    for size in [s for s in SIZES if s <= 2097153]:
        assert _by_definition(size) == len(serialize_instruction(raw=bytes(size))), size


def test_serialized_size_at_every_varint_step(lib):
    for size in SIZES + [0xFFFFFFFF]:
        recs = np.zeros(1, dtype=RECORD_DTYPE)
        recs["kind"], recs["size"] = _lib.ZC_BYTES, size
        assert serialized_size(recs) == _by_definition(size), size
    for kind in (0, 1, 3, 7, 0xFFFFFFFF):  # every other kind value is a chunk, whatever its size field says
        recs = np.zeros(1, dtype=RECORD_DTYPE)
        recs["kind"], recs["size"] = kind, 12345
        assert serialized_size(recs) == 27


def test_serialized_size_is_the_sum_over_the_records(lib):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 64, 65, 1000):
        recs = np.zeros(n, dtype=RECORD_DTYPE)
        recs["kind"] = rng.integers(0, 3, n)
        recs["size"] = rng.choice(np.array(SIZES[:-6] + [200, 5000, 65536]), n)
        want = sum(_message_len(int(r["kind"]), int(r["size"])) for r in recs)
        assert serialized_size(recs) == want, n
