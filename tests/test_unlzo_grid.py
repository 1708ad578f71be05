"""CPU tests beside tests/test_unlzo.py:

* the decoder core (zc_lzo_dec.h's token walker, through the check program of
  tests/test_unlzo.py: ASan + UBSan, a sink that aborts on any op outside the
  walker's validity rule and copies matches in the replicating k % dist form)
  against liblzo2 on the hand-built match grid of tests/unlzo_grid.py -- every
  match form at distances and lengths a compressor's output only hits by
  chance (1, 2, 3, 63, 64, 65, ... 49151; extended lengths; 0-3 trailing
  literals; a second match over the bytes just written);
* RestorePlan.instruction_image, the part of the restore's scratch buffer
  that comes from the host whoever decodes the payloads."""
import re
import subprocess

import numpy as np

from tests import unlzo_grid, unlzo_inputs
from tests.test_unlzo import _build_check, needs_lzo
from zbackup_amd.chunker import serialize_instruction


@needs_lzo
def test_grid_streams_are_valid_and_cover_the_match_forms():
    """The assembler's own check: the library accepts every grid stream (the
    share left out is 0), decodes it to the planned size, and M2, M3 and M4
    all occur."""
    cases = unlzo_grid.grid_cases()
    assert len(cases) == len(unlzo_grid.DISTS) * len(unlzo_grid.LENS) * len(unlzo_grid.TRAILS) == 18 * 9 * 4
    for framed, n, what in cases:
        status, data = unlzo_inputs.library_decode(framed)
        assert status == 0 and len(data) == n, (what, status, len(data), n)
    assert {w[3] for _, _, w in cases} == {"M2", "M3", "M4"}
    # the second match really reads the bytes the first one (and its trailing literals) wrote
    framed, n, (dist, length, ntrail, _) = cases[4 * 9 * 3 + 4 * 4 + 2]  # dist 7, len 65, 2 trailing
    data = unlzo_inputs.library_decode(framed)[1]
    first = n - 67 - ntrail - length
    assert (dist, length, ntrail) == (7, 65, 2)
    assert data[first:first + length] == bytes(data[first - 7 + k % 7] for k in range(length))
    assert data[n - 67:] == bytes(data[first + k] for k in range(67))


@needs_lzo
def test_decoder_core_matches_liblzo2_on_the_grid(tmp_path):
    cases = [(f, n, 0) for f, n, _ in unlzo_grid.grid_cases()]
    cases += [(f, n - 1, -5) for f, n, _ in unlzo_grid.grid_cases()[::37]]  # the last match one byte short of room
    path = str(tmp_path / "grid.bin")
    unlzo_inputs.write_cases(path, cases)
    exe, sanitized = _build_check(tmp_path)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    print(out.stdout, "sanitized" if sanitized else "NOT sanitized")
    assert int(re.search(r"^ok (\d+)$", out.stdout, re.M).group(1)) == len(cases)


def test_instruction_image_is_the_host_part_of_the_scratch_buffer():
    from zbackup_amd import _build
    from zbackup_amd.restore import Restorer
    _build.build()  # Restorer.plan parses through the library (host-only entry point)
    a, b = bytes([1]) * 24, bytes([2]) * 24
    bundles = [[(a, 300)], [(b, 4096)]]
    stream = (serialize_instruction(raw=b"head") + serialize_instruction(chunk_blob=b) +
              serialize_instruction(chunk_blob=a) + serialize_instruction(raw=b"tail bytes"))
    p = Restorer.plan(stream, bundles)
    at, instr = p.instruction_image()
    assert at == p.instr_off == 4096 + 304 and instr.dtype == np.uint8 and instr.tobytes() == stream
    assert at + len(instr) == p.work_size
    payloads = [bytes([7]) * 4096, bytes([9]) * 300]  # in plan.used order: bundle 1 first
    assert p.used == [1, 0]
    img = p.host_image(payloads)
    only = np.zeros(p.work_size, dtype=np.uint8)
    only[at:at + len(instr)] = instr
    for k, pay in enumerate(payloads):  # host_image = the instruction image plus the payloads
        only[p.pay_off[k]:p.pay_off[k] + len(pay)] = np.frombuffer(pay, dtype=np.uint8)
    assert np.array_equal(img, only)
    # every bytes_to_emit run of the scatter list reads inside the image
    runs = [(int(s), int(n)) for s, n in zip(p.src_off, p.sizes) if s >= at]
    assert [instr[s - at:s - at + n].tobytes() for s, n in runs] == [b"head", b"tail bytes"]
