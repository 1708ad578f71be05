"""GPU tests of every compiled form of the CBC kernels and of the bundle
parser's edges, through the C ABI.

The library picks a CBC kernel per call from four environment variables
(ZC_AES_TABLE, ZC_AES_ENC, ZC_AES_CPW, ZC_AES_PREFETCH: kept for the
measurements of DESIGN 4.8); zc_aes_last_form reports the one that ran, and
every test here that sets a variable asserts it.  One fixed set of 130 chains
goes through every form and is compared byte for byte, canaries included, with
one reference pass of tests/aes_ref.py; 18 keys go through both ways the round
keys reach a kernel; bundle files with padded and canonical varints, empty
parts, more than 64 files per call, bad files between good ones and odd
addresses go through seal / unseal against the Python restatement of the
format.

Everything is compared: there is no budget skip.  The bytes put through the
reference cipher are counted (41,104 when the whole module runs, under the
64 KiB the pure-Python cipher is allowed), and the last test asserts that
every case a reference was computed for was compared with a device result."""
import itertools

import numpy as np
import pytest

from tests import aes_ref
from tests.test_gpu_aes import CANARY, KEY, _bad_files, _first_diff, _layout
from zbackup_amd import _lib

pytestmark = pytest.mark.gpu

ENV = ("ZC_AES_TABLE", "ZC_AES_ENC", "ZC_AES_CPW", "ZC_AES_PREFETCH")
DEC, PLAIN, LANE, AHEAD1 = (_lib.ZC_AES_FORM_DECRYPT, _lib.ZC_AES_FORM_PLAIN_TABLES, _lib.ZC_AES_FORM_LANE,
                            _lib.ZC_AES_FORM_AHEAD_1)
CPW_SHIFT = _lib.ZC_AES_FORM_CPW_SHIFT
assert (DEC, PLAIN, LANE, AHEAD1, CPW_SHIFT) == (1, 2, 4, 8, 8)  # the bits include/zchunk.h documents


class _Tally:
    """The cases a reference was computed for, those a device result was
    compared with, and the bytes that went through the reference cipher."""
    referenced, compared, ref_bytes = set(), set(), 0


def _referenced(cases, nbytes):
    _Tally.referenced.update(cases)
    _Tally.ref_bytes += nbytes
    assert _Tally.ref_bytes <= 64 << 10, "the reference traffic of this module must stay under aes_ref's budget"


def _compared(cases):
    _Tally.compared.update(cases)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from zbackup_amd import _build
    _build.build()
    return torch


@pytest.fixture(scope="module")
def comp(torch_cuda):
    from zbackup_amd.bundle import BundleCompressor
    with BundleCompressor() as c:
        yield c


@pytest.fixture(autouse=True)
def default_form(monkeypatch):
    """Every test starts from the default form, whatever the caller's environment holds."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _select(monkeypatch, table=None, enc=None, pf=None, cpw=None):
    for name, v in zip(ENV, (table, enc, cpw, pf)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _form(decrypt=False, table=None, enc=None, pf=None, cpw=None):
    """The bits zc_aes_last_form documents for a call under these settings."""
    f = PLAIN if table == "shared" else 0
    if decrypt:
        return f | DEC
    if enc != "lane":
        return f
    return f | LANE | (AHEAD1 if pf == "1" else 0) | (int(cpw) if cpw else 64) << CPW_SHIFT


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- B. one chain set through every form ----

N_CHAINS = 130
CYCLE = [16, 32, 48, 64, 80, 240, 272]


def _chain_images(tag, key, rng, lens):
    """Random chains packed back to back, non-zero IVs, shuffled outputs between
    canaries; one reference pass.  Returns the inputs and the expected output
    image of each direction (the decrypt input is the reference's ciphertext)."""
    n = len(lens)
    in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    plain = rng.integers(0, 256, int(sum(lens)), dtype=np.uint8)
    ivs = rng.integers(1, 256, 16 * n, dtype=np.uint8).tobytes()
    out_off, total = _layout(rng, lens, True)
    cipher = np.empty_like(plain)
    enc_img = np.full(total, CANARY, dtype=np.uint8)
    dec_img = np.full(total, CANARY, dtype=np.uint8)
    for k in range(n):
        a = int(in_off[k])
        piece = plain[a:a + lens[k]].tobytes()
        c = np.frombuffer(aes_ref.cbc_encrypt(key, ivs[16 * k:16 * k + 16], piece), dtype=np.uint8)
        cipher[a:a + lens[k]] = c
        enc_img[out_off[k]:out_off[k] + lens[k]] = c
        dec_img[out_off[k]:out_off[k] + lens[k]] = plain[a:a + lens[k]]
    cases = [(tag, k) for k in range(n)]
    _referenced(cases, int(sum(lens)))
    return dict(key=key, lens=lens, in_off=in_off, ivs=ivs, out_off=out_off, total=total, cases=cases,
                plain=_frozen(plain), cipher=_frozen(cipher), enc_img=_frozen(enc_img), dec_img=_frozen(dec_img))


@pytest.fixture(scope="module")
def chainset():
    lens = [4112] + [CYCLE[k % 7] for k in range(1, N_CHAINS)]
    assert len(lens) == 130 and sum(lens) == 17792
    assert {n // 16 % 4 for n in lens} == {0, 1, 2, 3} and min(lens) < 4 * 16 < 256 * 16 < lens[0]
    return _chain_images("chain", KEY, np.random.default_rng(2024), lens)


def _run_set(torch, comp, cs, decrypt, form):
    """The whole set in one call: every output byte and canary, then the form that ran."""
    src = cs["cipher"] if decrypt else cs["plain"]
    d_in = torch.from_numpy(src.copy()).cuda()
    d_out = torch.full((cs["total"],), CANARY, dtype=torch.uint8, device="cuda")
    fn = comp.aes_decrypt if decrypt else comp.aes_encrypt
    fn(cs["key"], d_in.data_ptr(), cs["in_off"], cs["lens"], d_out.data_ptr(), cs["out_off"], iv=cs["ivs"])
    at = _first_diff(d_out.cpu().numpy(), cs["dec_img" if decrypt else "enc_img"])
    assert at is None, f"first wrong byte at {at} of {cs['total']} ({'decrypt' if decrypt else 'encrypt'})"
    got = comp.aes_last_form()
    assert got == form, f"form {got:#x} ran, {form:#x} was asked for"
    _compared(cs["cases"])


ENC_FORMS = [(table, None, None, None) for table in (None, "shared")] + \
            [(table, "lane", pf, cpw) for table in (None, "shared") for pf in (None, "1")
             for cpw in (None, "64", "7", "1")]


def _form_id(f):
    table, enc, pf, cpw = f
    parts = [table or "replicated", enc or "enc4"] + (["ahead1"] if pf else []) + (["cpw" + cpw] if cpw else [])
    return "-".join(parts)


@pytest.mark.parametrize("form", ENC_FORMS, ids=_form_id)
def test_encrypt_forms(torch_cuda, comp, chainset, monkeypatch, form):
    """130 chains: a third workgroup of the four-lane kernel (64 chains each), a
    third wave of the lane kernel at 64 chains per wave, ragged last waves at
    7, a wave per chain at 1; chains shorter than one read-ahead group."""
    table, enc, pf, cpw = form
    _select(monkeypatch, table, enc, pf, cpw)
    _run_set(torch_cuda, comp, chainset, False, _form(False, table, enc, pf, cpw))


@pytest.mark.parametrize("table", [None, "shared"], ids=["replicated", "shared"])
def test_decrypt_forms(torch_cuda, comp, chainset, monkeypatch, table):
    """Chain 0 has 257 blocks: more than one pass of the kernel's 256 threads."""
    _select(monkeypatch, table)
    _run_set(torch_cuda, comp, chainset, True, _form(True, table))


@pytest.mark.parametrize("cpw", ["0", "65", "x"])
def test_chains_per_wave_out_of_range_is_64(torch_cuda, comp, chainset, monkeypatch, cpw):
    _select(monkeypatch, enc="lane", cpw=cpw)
    _run_set(torch_cuda, comp, chainset, False, LANE | 64 << CPW_SHIFT)


def test_unknown_values_select_the_default_form(torch_cuda, comp, chainset, monkeypatch):
    _select(monkeypatch, enc="quad")
    _run_set(torch_cuda, comp, chainset, False, 0)
    _select(monkeypatch, table="SHARED")  # the value is case sensitive
    _run_set(torch_cuda, comp, chainset, False, 0)
    _run_set(torch_cuda, comp, chainset, True, DEC)
    _select(monkeypatch, table="shared", cpw="7", pf="1")  # neither applies to the four-lane kernel
    _run_set(torch_cuda, comp, chainset, False, PLAIN)


def test_no_form_before_the_first_cbc_launch(torch_cuda):
    """A fresh context reports ZC_ERR_ARG with a message; a seal without a key launches no CBC kernel."""
    import ctypes
    from zbackup_amd.bundle import BundleCompressor
    torch = torch_cuda
    with BundleCompressor() as c:
        form = ctypes.c_uint32(0xABCD)
        assert c._L.zc_aes_last_form(c._ctx, ctypes.byref(form)) == _lib.ZC_ERR_ARG
        assert b"no CBC kernel" in c._L.zc_last_error(c._ctx) and form.value == 0xABCD
        d = torch.full((256,), CANARY, dtype=torch.uint8, device="cuda")
        c.seal(None, [b"\x00\x00"], d.data_ptr(), [0], [4], d.data_ptr() + 128, [0])
        with pytest.raises(_lib.ZcError, match="no CBC kernel"):
            c.aes_last_form()
        assert c._L.zc_aes_last_form(c._ctx, None) == _lib.ZC_ERR_ARG
        c.aes_encrypt(KEY, d.data_ptr(), [0], [16], d.data_ptr(), [64])
        assert c.aes_last_form() == 0
        assert c._L.zc_last_error(c._ctx) == b""


# ---- C. keys ----

@pytest.fixture(scope="module")
def keyset():
    """16 seeded random keys, the all-zero key and the all-0xFF key; chains of 16, 80 and 272 bytes under each."""
    rng = np.random.default_rng(77)
    keys = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(16)] + [bytes(16), b"\xff" * 16]
    sets = [_chain_images(("key", i), key, rng, [16, 80, 272]) for i, key in enumerate(keys)]
    assert sum(sum(s["lens"]) for s in sets) == 6624
    return sets


@pytest.mark.parametrize("mode", ["enc4", "lane", "decrypt"])
def test_keys(torch_cuda, comp, keyset, monkeypatch, mode):
    """The round keys reach the kernels two ways: a device buffer (the four-lane
    kernel) and a kernel argument (the lane kernel, decrypt)."""
    enc = "lane" if mode == "lane" else None
    _select(monkeypatch, enc=enc)
    for cs in keyset:
        _run_set(torch_cuda, comp, cs, mode == "decrypt", _form(mode == "decrypt", enc=enc))


# ---- D. bundle files ----

WIDTHS = (1, 2, 3, 4, 5)
TRIPLES = ((0, 0, 0), (2, 5, 1), (3, 127, 33))  # (header, info, body) bytes
LAYOUT_FIELDS = ("header_off", "header_len", "info_off", "info_len", "body_off", "body_len")


def _padded_varint(v, width):
    """v as a varint of exactly `width` bytes: the canonical bytes, then 0x80
    continuation bytes (zero payload) up to a final 0x00, which protobuf's
    reader accepts."""
    out = bytearray(aes_ref.varint(v))
    assert len(out) <= width <= 5
    if len(out) < width:
        out[-1] |= 0x80
        out += b"\x80" * (width - len(out) - 1) + b"\x00"
    return bytes(out)


def _file_set(tag, key, prefixes, bodies):
    """The reference's view of a set of files: sealed bytes, plaintext, layout."""
    keyed = key is not None
    files = [aes_ref.seal_ref(key, p, b) for p, b in zip(prefixes, bodies)]
    plains = [aes_ref.plaintext_ref(p, b, keyed) for p, b in zip(prefixes, bodies)]
    layouts = []
    for f, plain in zip(files, plains):
        st, lay, back = aes_ref.unseal_ref(key, f)
        assert st == aes_ref.OK and back == plain and sorted(lay) == sorted(LAYOUT_FIELDS)
        layouts.append(lay)
    body_len = [len(b) for b in bodies]
    body_off = np.concatenate([[0], np.cumsum(body_len)[:-1]]).astype(np.uint64)
    cases = [(tag, k) for k in range(len(files))]
    _referenced(cases, 2 * sum(len(f) for f in files) if keyed else 0)  # seal_ref and unseal_ref
    return dict(key=key, prefixes=prefixes, bodies=bodies, files=files, plains=plains, layouts=layouts, cases=cases,
                body_off=body_off, body_len=body_len, sizes=[len(f) for f in files],
                body_blob=_frozen(np.frombuffer(b"".join(bodies) + b"\0", dtype=np.uint8).copy()))


@pytest.fixture(scope="module")
def matrix():
    """Header-length varint width 1..5 x info-length varint width 1..5 x three
    (header, info, body) length triples: 75 files, keyed and plain."""
    out = {}
    for keyed in (True, False):
        rng = np.random.default_rng(31 if keyed else 32)
        prefixes, bodies, want = [], [], []
        for (h, i, b), wh, wi in itertools.product(TRIPLES, WIDTHS, WIDTHS):
            R = rng.integers(0, 256, 16, dtype=np.uint8).tobytes() if keyed else b""
            prefixes.append(R + _padded_varint(h, wh) + rng.integers(0, 256, h, dtype=np.uint8).tobytes() +
                            _padded_varint(i, wi) + rng.integers(0, 256, i, dtype=np.uint8).tobytes())
            bodies.append(rng.integers(0, 256, b, dtype=np.uint8).tobytes())
            start = 16 if keyed else 0
            want.append(dict(header_off=start + wh, header_len=h, info_off=start + wh + h + wi, info_len=i,
                             body_off=start + wh + h + wi + i + 4, body_len=b))
        m = _file_set(("matrix", keyed), KEY if keyed else None, prefixes, bodies)
        assert len(m["files"]) == 75 and m["layouts"] == want  # the reference reads the intended lengths back
        if keyed:
            assert sum(m["sizes"]) == 7200
        out[keyed] = m
    return out


def _image(total, offs, pieces):
    img = np.full(total, CANARY, dtype=np.uint8)
    for o, p in zip(offs, pieces):
        img[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return img


def _caps(sizes):
    return [max(16, (s + 15) // 16 * 16) for s in sizes]


def _seal_set(torch, comp, m, rng):
    """One seal call for the whole set: the sizes, then every byte of every file and the canaries between."""
    file_off, total = _layout(rng, _caps(m["sizes"]), True)
    d_body = torch.from_numpy(m["body_blob"].copy()).cuda()
    d_files = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    got = comp.seal(m["key"], m["prefixes"], d_body.data_ptr(), m["body_off"], m["body_len"], d_files.data_ptr(),
                    file_off)
    assert [int(s) for s in got] == m["sizes"]
    at = _first_diff(d_files.cpu().numpy(), _image(total, file_off, m["files"]))
    assert at is None, f"first wrong byte at {at} of {total}"


def _check_unsealed(m, layout, got, plain_off, total):
    for k, (lay, ref_lay) in enumerate(zip(layout, m["layouts"])):
        assert int(lay["status"]) == 0, (k, int(lay["status"]))
        for name in LAYOUT_FIELDS:
            assert int(lay[name]) == ref_lay[name], (k, name)
    at = _first_diff(got, _image(total, plain_off, m["plains"]))
    assert at is None, f"first wrong byte at {at} of {total}"


def _unseal_set(torch, comp, m, rng):
    """One unseal call over the reference's files: status, every layout field, every plaintext byte, the canaries."""
    file_off, ftotal = _layout(rng, _caps(m["sizes"]), True)
    plain_off, ptotal = _layout(rng, _caps(m["sizes"]), True)
    d_files = torch.from_numpy(_image(ftotal, file_off, m["files"])).cuda()
    d_plain = torch.full((ptotal,), CANARY, dtype=torch.uint8, device="cuda")
    layout = comp.unseal(m["key"], d_files.data_ptr(), file_off, m["sizes"], d_plain.data_ptr(), plain_off)
    _check_unsealed(m, layout, d_plain.cpu().numpy(), plain_off, ptotal)


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_varint_matrix(torch_cuda, comp, matrix, keyed):
    """All five iterations of the device's varint loop for both lengths, empty
    header / info / body and a 1-byte body, 75 files (a second workgroup of the
    one-lane-per-file parse kernel, 75 chains) per call."""
    m = matrix[keyed]
    rng = np.random.default_rng(41)
    _seal_set(torch_cuda, comp, m, rng)
    if keyed:
        assert comp.aes_last_form() == 0
    _unseal_set(torch_cuda, comp, m, rng)
    if keyed:
        assert comp.aes_last_form() == DEC
    _compared(m["cases"])


def test_sealed_files_under_the_other_forms(torch_cuda, comp, matrix, monkeypatch):
    """A keyed seal through the lane kernel with plain tables, one block of
    read-ahead and 7 chains per wave, then the unseal through the plain-table
    decrypt kernel: the reference's bytes, and the forms reported."""
    m = matrix[True]
    rng = np.random.default_rng(42)
    _select(monkeypatch, table="shared", enc="lane", pf="1", cpw="7")
    _seal_set(torch_cuda, comp, m, rng)
    assert comp.aes_last_form() == LANE | PLAIN | AHEAD1 | 7 << CPW_SHIFT
    _unseal_set(torch_cuda, comp, m, rng)
    assert comp.aes_last_form() == DEC | PLAIN
    _compared(m["cases"])


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_bad_files_between_good_ones(torch_cuda, comp, matrix, keyed):
    """One bad file after every sixth good file of the matrix, all in one unseal
    call: each bad file gets its own status, every good file stays 0 with its
    layout and plaintext, and nothing is written outside the plaintext extents."""
    torch = torch_cuda
    m = matrix[keyed]
    key = KEY if keyed else None
    bad, good, _ = _bad_files(key)
    cases = [("bad", keyed, name) for name, _, _ in bad]
    # _bad_files encrypts each wrong plaintext, the whole file it then cuts, and the good file it returns
    _referenced(cases, sum((len(f) + 15) // 16 * 16 for _, f, _ in bad) + len(good) if keyed else 0)
    files, want_status, good_at, left = [], [], [], list(bad)
    for k, f in enumerate(m["files"]):
        good_at.append(len(files))
        files.append(f)
        want_status.append(0)
        if (k + 1) % 6 == 0 and left:
            name, f_bad, st = left.pop(0)
            files.append(f_bad)
            want_status.append(st)
    assert not left and len(files) == 75 + len(bad) and len(files) > 64
    sizes = [len(f) for f in files]
    rng = np.random.default_rng(43)
    file_off, ftotal = _layout(rng, _caps(sizes), True)
    plain_off, ptotal = _layout(rng, _caps(sizes), True)
    d_files = torch.from_numpy(_image(ftotal, file_off, files)).cuda()
    d_plain = torch.full((ptotal,), CANARY, dtype=torch.uint8, device="cuda")
    layout = comp.unseal(key, d_files.data_ptr(), file_off, sizes, d_plain.data_ptr(), plain_off)
    status = [int(s) for s in layout["status"]]
    names = {at: name for at, name in zip(sorted(set(range(len(files))) - set(good_at)), (b[0] for b in bad))}
    for at, (got_st, want_st) in enumerate(zip(status, want_status)):
        assert got_st == want_st, (at, names.get(at, "good file"), got_st, want_st)
    got = d_plain.cpu().numpy()
    want = np.full(ptotal, CANARY, dtype=np.uint8)
    for at in range(len(files)):
        o, s = plain_off[at], sizes[at]
        if want_status[at] in (aes_ref.OK, aes_ref.BAD_SIZE):  # a file of a refused size is left alone
            continue
        want[o:o + s] = got[o:o + s]  # the plaintext of a bad file is not pinned
    for k, at in enumerate(good_at):
        o = plain_off[at]
        want[o:o + sizes[at]] = np.frombuffer(m["plains"][k], dtype=np.uint8)
        for name in LAYOUT_FIELDS:
            assert int(layout[at][name]) == m["layouts"][k][name], (k, name)
    at = _first_diff(got, want)
    assert at is None, f"first wrong byte at {at} of {ptotal}"
    _compared(cases)
    _compared(m["cases"])


def test_canonical_varint_edges(torch_cuda, comp):
    """Info lengths on both sides of the 1-to-2, 2-to-3 and 3-to-4 byte varint
    edges, without a key (the varint code is the same for both kinds of file)."""
    info_lens = [127, 128, 16383, 16384, 2097151, 2097152]
    rng = np.random.default_rng(44)
    prefixes = [aes_ref.message(b"\x08\x01") + aes_ref.message(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                for n in info_lens]
    m = _file_set("edge", None, prefixes, [b"body"] * len(info_lens))
    assert [lay["info_off"] - (lay["header_off"] + lay["header_len"]) for lay in m["layouts"]] == [1, 2, 2, 3, 3, 4]
    assert [lay["info_len"] for lay in m["layouts"]] == info_lens
    _seal_set(torch_cuda, comp, m, rng)
    _unseal_set(torch_cuda, comp, m, rng)
    _compared(m["cases"])


def _parity_layout(rng, sizes, parity):
    """Offsets of the given parity with 1..15 canary bytes between the extents, in a shuffled order."""
    off, pos = [0] * len(sizes), 0
    for k in rng.permutation(len(sizes)):
        gap = int(rng.integers(1, 16))
        if (pos + gap) % 2 != parity:
            gap += 1 if gap < 15 else -1
        off[k] = pos + gap
        pos = off[k] + sizes[k]
    assert all(o % 2 == parity for o in off)
    return off, pos + 16


# (files base, plaintext base, parity of every file_off, parity of every plain_off).  An odd base
# with odd offsets, the first two rows, gives even addresses; the rows after them make the
# addresses themselves odd: on one side only (an odd distance from source to destination), on
# both, and from aligned bases.
UNALIGNED = [(1, 3, 1, 1), (3, 1, 1, 1), (1, 3, 0, 1), (3, 1, 1, 0), (1, 3, 0, 0), (0, 0, 1, 1)]


@pytest.mark.parametrize("case", UNALIGNED, ids=lambda c: "files+%d,plain+%d,offsets%d%d" % c)
def test_plain_unseal_at_odd_addresses(torch_cuda, comp, matrix, case):
    """Without a key nothing needs alignment.  The copy kernel's head (the bytes
    up to the destination's 16-byte alignment) and the Adler-32 kernel's first
    slot depend on the absolute address, and the copy's unaligned loads on the
    distance from source to destination, so it is those that are made odd and
    asserted, at every odd residue mod 16."""
    torch = torch_cuda
    m = matrix[False]
    fb, pb, f_par, p_par = case
    rng = np.random.default_rng(45)
    file_off, ftotal = _parity_layout(rng, m["sizes"], f_par)
    plain_off, ptotal = _parity_layout(rng, m["sizes"], p_par)
    # the images start at the base pointers; 16 spare bytes behind each
    img = np.concatenate([np.full(fb, CANARY, np.uint8), _image(ftotal, file_off, m["files"])])
    d_files = torch.from_numpy(img).cuda()
    d_plain = torch.full((pb + ptotal,), CANARY, dtype=torch.uint8, device="cuda")
    assert d_files.data_ptr() % 16 == 0 and d_plain.data_ptr() % 16 == 0
    f_ptr, p_ptr = d_files.data_ptr() + fb, d_plain.data_ptr() + pb
    f_abs = [f_ptr + o for o in file_off]
    p_abs = [p_ptr + o for o in plain_off]
    f_odd, p_odd = (fb + f_par) % 2, (pb + p_par) % 2
    assert all(a % 2 == f_odd for a in f_abs) and all(a % 2 == p_odd for a in p_abs)
    if case not in UNALIGNED[:2]:
        assert f_odd or p_odd
    if f_odd:
        assert {a % 16 for a in f_abs} == set(range(1, 16, 2))
    if p_odd:
        assert {a % 16 for a in p_abs} == set(range(1, 16, 2))  # every odd head of the copy
    if f_odd != p_odd:
        assert {(a - b) % 16 for a, b in zip(f_abs, p_abs)} == set(range(1, 16, 2))
    layout = comp.unseal(None, f_ptr, file_off, m["sizes"], p_ptr, plain_off)
    got = d_plain.cpu().numpy()
    assert (got[:pb] == CANARY).all()
    _check_unsealed(m, layout, got[pb:], plain_off, ptotal)
    _compared(m["cases"])


def test_misaligned_offsets_are_refused(torch_cuda, comp):
    """Keyed unseal with an odd plain_off, and seal (keyed or not) with an odd
    file_off: ZC_ERR_ARG with a message, and every byte left as it was."""
    torch = torch_cuda
    d = torch.full((2048,), CANARY, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    with pytest.raises(_lib.ZcError, match="zc_bundle_unseal.*not 16-byte aligned"):
        comp.unseal(KEY, p, [0], [64], p + 1024, [17])
    assert bool((d == CANARY).all())
    for key in (KEY, None):
        with pytest.raises(_lib.ZcError, match="zc_bundle_seal.*not 16-byte aligned"):
            comp.seal(key, [b"p" * 20], p, [0], [8], p + 1024, [17])
        assert bool((d == CANARY).all())


def test_every_referenced_case_was_compared():
    """Runs last: no case a reference was computed for went uncompared, and the
    reference traffic stayed under the pure-Python cipher's budget."""
    assert _Tally.compared == _Tally.referenced
    assert len(_Tally.compared) == len(_Tally.referenced)
    assert _Tally.ref_bytes <= 64 << 10
    print(f"{len(_Tally.compared)} cases compared, {_Tally.ref_bytes} bytes through the reference cipher")
