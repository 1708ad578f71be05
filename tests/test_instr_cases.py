"""CPU tests of the device instruction parse's inputs and of its core:

* the cases of tests/instr_cases.py are what they claim, by the host parser
  (zc_parse_instructions) alone;
* zc_instr_core.h -- hop, tile exits, chain, emit, the steps zc_instr.hip's
  kernels run -- compiled for the host (under ASan + UBSan where that links)
  with a main of its own, run tile by tile at T = 64, 256 and the default over
  every case and compared with a plain serial parser
  (tests/instr/instr_core_check.cpp), which also asserts hop[p] > p and
  exit[p] >= the tile's end everywhere."""
import collections
import os
import re
import struct
import subprocess

import pytest

from tests import instr_cases as C
from zbackup_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz()


def test_texts_are_the_host_parsers():
    src = open(os.path.join(ROOT, "zbackup_amd", "csrc", "zc_engine.cpp")).read()
    body = src[src.index("int zc_parse_instructions("):src.index("// ---- encrypted repositories")]
    assert sorted(re.findall(r'bad\("([^"]+)"', body)) == sorted(C.TEXTS) and len(C.TEXTS) == 8
    core = open(os.path.join(ROOT, "zbackup_amd", "csrc", "zc_instr_core.h")).read()
    for text in C.TEXTS:
        assert f'"{text}"' in core
    assert f"kTileDefault = {C.T_DEFAULT};" in core


def test_named_cases_are_what_they_claim(lib):
    named = C.all_named()
    assert len({name for name, _, _ in named}) == len(named)
    by_name = {name: (data, tile) for name, data, tile in named}
    kind = lambda name: C.host_parse(lib, by_name[name][0])  # noqa: E731
    assert len(kind("six_messages")[1]) == 6 * 48 and len(kind("other_order")[1]) == 2 * 48
    assert kind("empty") == ("ok", b"") and len(kind("one_message")[1]) == 48
    # the malformed streams fail where they were put
    assert len(C.MALFORMED) == 11
    for name, bad in C.MALFORMED:
        alone = kind(f"{name}: alone")
        assert alone[0] == "error"
        what, at = alone[1].rsplit(" at byte ", 1)
        for where, shift in (("straddling", 3 * C.T - 1), ("behind 1000", len(C.good(1000, seed=3)))):
            assert kind(f"{name}: {where}") == ("error", f"{what} at byte {int(at) + shift}"), (name, where)
        data = by_name[f"{name}: straddling"][0]
        assert len(data) > 3 * C.T - 1 and (3 * C.T - 1) % C.T == C.T - 1
    # geometry
    assert kind("ends_at_tile_end")[0] == "ok"
    for vlen in (2, 3, 5):
        data = by_name[f"varint_{vlen}_across_edge"][0]
        assert kind(f"varint_{vlen}_across_edge")[0] == "ok"
        lv = data[2 * C.T - 1:2 * C.T - 1 + vlen]
        assert all(b & 0x80 for b in lv[:-1]) and not lv[-1] & 0x80
    for whole in (0, 1, 40):
        data = by_name[f"bytes_over_{whole}_tiles"][0]
        st, recs = kind(f"bytes_over_{whole}_tiles")
        assert st == "ok"
        sizes = [struct.unpack_from("<QQ", recs, 48 * k + 32) for k in range(len(recs) // 48)]
        off, size = max(sizes, key=lambda x: x[1])
        first, last = -(-off // C.T), (off + size) // C.T  # the tiles that lie inside the payload
        assert last - first >= whole and (whole == 0 or first < last)
    for n in (C.T - 1, C.T, C.T + 1):
        assert len(by_name[f"stream_of_{n}"][0]) == n and kind(f"stream_of_{n}")[0] == "ok"
    assert len(kind("entries_0_1_2")[1]) // 48 == 2 * 4 + 3 * 4
    assert len(by_name["scan_two_rounds"][0]) > 256 * C.T
    for name, tile in (("zeros_T64", C.T), ("zeros_default", C.T_DEFAULT)):
        assert by_name[name][0] == bytes(2 * tile + 1) and kind(name) == ("ok", b"")
    # phantoms: the payload adds nothing; cut, the outer message fails at its start
    for name, payload in C.phantom_payloads():
        st, recs = kind(f"phantom {name}")
        plain = C.host_parse(lib, C.good(3) + C.ser(raw=b"." * len(payload)) + C.good(20, seed=2))
        assert st == "ok" and recs == plain[1]
        assert kind(f"phantom cut {name}") == ("error", "instruction length past the end of the stream at byte "
                                               f"{len(C.good(3))}")
    assert C.host_parse(lib, C.good(50, seed=11))[0] == "ok"


def test_fuzz_meets_its_condition(lib, fuzz):
    """Each of the eight failure texts occurs at least ten times among the
    mutants, and at least 200 mutants still parse."""
    streams, mutants = fuzz
    assert len(streams) == 200 and len(mutants) == 2000
    assert min(len(d) for _, d, _ in streams) == 0 and max(len(d) for _, d, _ in streams) >= 70000
    assert {t for _, _, t in streams} == {t for _, _, t in mutants} == set(C.TILES)
    assert all(C.host_parse(lib, d)[0] == "ok" for _, d, _ in streams)
    seen = collections.Counter()
    for _, d, _ in mutants:
        r = C.host_parse(lib, d)
        seen["ok" if r[0] == "ok" else r[1].rsplit(" at byte ", 1)[0]] += 1
    print(dict(seen))
    assert set(seen) == set(C.TEXTS) | {"ok"}
    assert all(seen[t] >= 10 for t in C.TEXTS) and seen["ok"] >= 200


def _build_check(tmp_path):
    """The check program, sanitized when a sanitized binary links here, else plain."""
    exe = str(tmp_path / "instr_core_check")
    base = ["g++", "-O1", "-g", "-Wall", "-Werror", "-std=c++17", "-I" + os.path.join(ROOT, "zbackup_amd", "csrc"),
            os.path.join(ROOT, "tests", "instr", "instr_core_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base[:1] + san + base[1:], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(base, check=True)
    return exe, False


def test_core_matches_a_serial_parser(tmp_path, fuzz):
    exe, sanitized = _build_check(tmp_path)
    cases = C.all_named() + fuzz[0] + fuzz[1]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for _, data, _ in cases:
            f.write(struct.pack("<Q", len(data)) + data)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    m = re.search(r"^ok (\d+) cases (\d+) checks$", out.stdout, re.M)
    assert int(m.group(1)) == len(cases) and int(m.group(2)) == 3 * len(cases)
