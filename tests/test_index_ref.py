"""CPU tests of the index-file reader's two restatements:

* tests/index_ref.py (pure Python) passes its own round trip, reaches every
  status with its crafted files and mutations, and agrees with the protobuf
  runtime (libprotobuf's parser) on the messages themselves;
* zc_index_core.h -- the walkers the kernels of zc_index.hip run -- compiled for
  the host (under ASan + UBSan where that links) with a main of its own
  (tests/index/index_core_check.cpp): its own checks, and the same status and
  records as index_ref on every crafted and mutated file."""
import os
import random
import re
import struct
import subprocess

import pytest

from tests import aes_ref
from tests import index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(0x40, 0x50))
RND = bytes(range(0xA0, 0xB0))
EDGE_SIZES = [0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28, 2 ** 32 - 1]


@pytest.mark.parametrize("key", [None, KEY], ids=["plain", "keyed"])
def test_round_trip(key):
    rng = random.Random(1)
    for counts in ([], [0], [1], [4, 5], [600], [3, 0, 2, 0]):
        for size_first in (False, True):
            b = R.rand_bundles(rng, counts, EDGE_SIZES)
            f = R.write(b, key, RND, size_first=size_first)
            assert len(f) == R.file_size(len(R.body(b, size_first)), key is not None)
            assert R.read(f, key) == (R.OK, b)
    b = R.rand_bundles(rng, [3])
    assert R.read(R.seal(R.body(b), None, trailing=b"junk after the Adler-32"), None) == (R.OK, b)
    mixed = R.body(b, size_first=[True, False, True])
    assert mixed != R.body(b) and R.read(R.seal(mixed, key, RND), key) == (R.OK, b)


def test_the_crafted_files_have_the_status_they_are_made_for():
    for key in (None, KEY):
        seen = set()
        for name, data, status in R.bad_files(key, RND):
            got, bundles = R.read(data, key)
            assert got == status, (name, R.STATUS_NAMES[got], R.STATUS_NAMES[status])
            assert bundles == [] or status == R.OK
            seen.add(got)
        want = set(range(9)) - ({R.BAD_PADDING} if key is None else set())
        assert seen == want, [R.STATUS_NAMES[s] for s in want - seen]


def test_the_mutations_reach_the_parse_statuses():
    rng = random.Random(2)
    base = R.body(R.rand_bundles(rng, [2, 0, 3]))
    for key in (None, KEY):
        seen = {R.read(m, key)[0] for m in R.mutations(base, key, RND)}
        assert {R.OK, R.TRUNCATED, R.BAD_MESSAGE, R.BAD_ADLER} <= seen
        if key is not None:
            assert {R.BAD_SIZE, R.BAD_PADDING} <= seen


def _messages():
    """FileHeader, IndexBundleHeader and BundleInfo / ChunkRecord as the
    protobuf runtime sees them, from descriptors written after zbackup.proto."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="index_ref_check.proto", package="index_ref_check", syntax="proto2")
    m = fd.message_type.add(name="FileHeader")
    m.field.add(name="version", number=1, type=F.TYPE_UINT32, label=F.LABEL_REQUIRED)
    m = fd.message_type.add(name="IndexBundleHeader")
    m.field.add(name="id", number=1, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    m = fd.message_type.add(name="BundleInfo")
    c = m.nested_type.add(name="ChunkRecord")
    c.field.add(name="id", number=1, type=F.TYPE_BYTES, label=F.LABEL_REQUIRED)
    c.field.add(name="size", number=2, type=F.TYPE_UINT32, label=F.LABEL_REQUIRED)
    m.field.add(name="chunk_record", number=1, type=F.TYPE_MESSAGE, label=F.LABEL_REPEATED,
                type_name=".index_ref_check.BundleInfo.ChunkRecord")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return {n: message_factory.GetMessageClass(pool.FindMessageTypeByName("index_ref_check." + n))
            for n in ("FileHeader", "IndexBundleHeader", "BundleInfo")}


def test_the_protobuf_runtime_reads_and_writes_the_same_bytes():
    pytest.importorskip("google.protobuf")
    M = _messages()
    rng = random.Random(3)
    bundles = R.rand_bundles(rng, [0, 1, 5, 40], EDGE_SIZES)

    def framed(msg):
        return R.message(msg.SerializeToString())

    # the runtime's serialisation is index_ref's writer, message by message
    want = bytearray(framed(M["FileHeader"](version=1)))
    for bid, recs in bundles:
        info = M["BundleInfo"]()
        for cid, size in recs:
            info.chunk_record.add(id=cid, size=size)
        want += framed(M["IndexBundleHeader"](id=bid)) + framed(info)
        assert info.SerializeToString() == R.bundle_info(recs)
    want += framed(M["IndexBundleHeader"]())
    assert bytes(want) == R.body(bundles)

    # and ParseFromString reads index_ref's file to the same records
    p = R.body(bundles, size_first=True)
    pos, got = 0, []

    def take():
        nonlocal pos
        n, pos = R._varint(p, pos, len(p))
        pos += n
        return p[pos - n:pos]

    h = M["FileHeader"]()
    h.ParseFromString(take())
    assert h.version == 1
    while True:
        bh = M["IndexBundleHeader"]()
        bh.ParseFromString(take())
        if not bh.HasField("id"):
            break
        info = M["BundleInfo"]()
        info.ParseFromString(take())
        got.append((bh.id, [(r.id, r.size) for r in info.chunk_record]))
    assert pos == len(p) and got == bundles
    assert R.read(R.seal(p), None) == (R.OK, bundles)


# ---- the core's walkers on the host ----

def _sanitizers_link(tmp_path):
    """Whether g++ links a trivial program under ASan + UBSan here."""
    src = tmp_path / "trivial.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "trivial")],
                          capture_output=True).returncode == 0


def _build_check(tmp_path):
    """The check program under ASan + UBSan.  Only where not even a trivial
    program links with them is it built plain; a fault that shows under the
    sanitizers alone fails the build here."""
    exe = str(tmp_path / "index_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "index", "index_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if _sanitizers_link(tmp_path):
        out = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-4000:]
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return _build_check(tmp_path_factory.mktemp("index_core"))


def test_core_walkers_stay_in_bounds_and_end(check_exe):
    exe, sanitized = check_exe
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    # 60 valid files, every truncation of two, 6,000 mutated ones
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) >= 6000


def _fnv(bundles):
    h = 0xcbf29ce484222325
    for bid, recs in bundles:
        blob = bid + struct.pack("<I", len(recs)) + b"".join(c + struct.pack("<I", s) for c, s in recs)
        for x in blob:
            h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_core_agrees_with_index_ref(check_exe, tmp_path):
    """Every crafted file and mutation, keyed (decrypted here: the core reads
    plaintext) and not: the same status, and for a good file the same records."""
    exe, _ = check_exe
    rng = random.Random(4)
    base = R.body(R.rand_bundles(rng, [2, 0, 3], EDGE_SIZES), size_first=[False, True])
    cases = []
    for key in (None, KEY):
        files = [d for _, d, _ in R.bad_files(key, RND)] + R.mutations(base, key, RND)
        files.append(R.write(R.rand_bundles(rng, [0, 1, 4, 5, 600], EDGE_SIZES), key, RND))
        for f in files:
            keyed = key is not None
            plain = aes_ref.cbc_decrypt(key, bytes(16), f) if keyed and len(f) and len(f) % 16 == 0 else f
            cases.append((keyed, plain, R.read(f, key)))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for keyed, plain, _ in cases:
            fh.write(struct.pack("<BI", keyed, len(plain)) + plain)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    seen = set()
    for k, (line, (keyed, plain, (status, bundles))) in enumerate(zip(lines, cases)):
        st, nb, nr, h = line.split()
        assert int(st) == status, (k, keyed, R.STATUS_NAMES[int(st)], R.STATUS_NAMES[status], plain.hex())
        assert (int(nb), int(nr), int(h, 16)) == (len(bundles), sum(len(r) for _, r in bundles), _fnv(bundles)), k
        seen.add(status)
    assert seen == set(range(9))
