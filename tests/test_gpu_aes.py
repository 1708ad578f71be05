"""GPU tests of the encryption path, through the C ABI: AES-128-CBC chains in
both directions against the reference helper (libcrypto when it loads, else
the pure-Python cipher on a 64 KiB budget), the refusals, and whole bundle
files sealed and unsealed against the Python restatement of the format.
Outputs lie between 0xEE canaries, which are checked."""
import hashlib

import numpy as np
import pytest

from oracle import lzo_oracle, oracle
from tests import aes_ref
from tests.lzo_inputs import payload

pytestmark = pytest.mark.gpu

CANARY = 0xEE
# blocks of 16 bytes per tile of the decrypt kernel's tile list (kAesTileBlocks in zc_aes.hip)
TILE = 4096 * 16
LENS = [16, 32, 48, 1008, 1024, 1040, 4096, 65552]
KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d7781")

_budget = [aes_ref.byte_budget()]


def _afford(n):
    """Whether the reference may take n more bytes (always, with libcrypto)."""
    if _budget[0] is None:
        return True
    if _budget[0] < n:
        return False
    _budget[0] -= n
    return True


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


def _first_diff(got, want):
    if np.array_equal(got, want):
        return None
    return int(np.nonzero(got != want)[0][0])


def _layout(rng, lens, shuffle):
    """Output offsets with 16..48 canary bytes between the extents, in a shuffled
    order when asked; returns (offsets, total)."""
    order = rng.permutation(len(lens)) if shuffle else np.arange(len(lens))
    off, pos = [0] * len(lens), 16
    for k in order:
        pos += 16 * int(rng.integers(0, 3))
        off[k] = pos
        pos += lens[k] + 16
    return off, pos + 16


def _run_chains(torch, comp, rng, lens, decrypt, ivs, shuffle=True):
    """Chains packed back to back in the input; every output byte compared."""
    n = len(lens)
    in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    src = rng.integers(0, 256, int(sum(lens)), dtype=np.uint8)
    out_off, total = _layout(rng, lens, shuffle)
    iv_list = [ivs[16 * k:16 * k + 16] if ivs is not None else bytes(16) for k in range(n)]
    want = np.full(total, CANARY, dtype=np.uint8)
    compared = []
    ref = aes_ref.cbc_decrypt if decrypt else aes_ref.cbc_encrypt
    for k in range(n):
        if not _afford(lens[k]):
            continue
        piece = src[int(in_off[k]):int(in_off[k]) + lens[k]].tobytes()
        want[out_off[k]:out_off[k] + lens[k]] = np.frombuffer(ref(KEY, iv_list[k], piece), dtype=np.uint8)
        compared.append(k)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    fn = comp.aes_decrypt if decrypt else comp.aes_encrypt
    fn(KEY, d_in.data_ptr(), in_off, lens, d_out.data_ptr(), out_off, iv=ivs)
    got = d_out.cpu().numpy()
    for k in set(range(n)) - set(compared):  # out of reference budget: not byte-compared
        want[out_off[k]:out_off[k] + lens[k]] = got[out_off[k]:out_off[k] + lens[k]]
    at = _first_diff(got, want)
    assert at is None, f"first wrong byte at {at} of {total} ({'decrypt' if decrypt else 'encrypt'}, {n} chains)"
    assert compared or _budget[0] is not None, "no chain was compared with the reference"
    return src, in_off, got, out_off


def test_vectors(torch_cuda, comp):
    """FIPS-197 C.1 (one block, zero IV = ECB) and SP 800-38A F.2.1 / F.2.2, device and host forms."""
    torch = torch_cuda
    for key, iv, plain, cipher in ((aes_ref.C1_KEY, None, aes_ref.C1_PLAIN, aes_ref.C1_CIPHER),
                                   (aes_ref.F2_KEY, aes_ref.F2_IV, aes_ref.F2_PLAIN, aes_ref.F2_CIPHER)):
        n = len(plain)
        for src, want, fn, host_fn in ((plain, cipher, comp.aes_encrypt, comp._L.zc_aes128_cbc_encrypt_host),
                                       (cipher, plain, comp.aes_decrypt, comp._L.zc_aes128_cbc_decrypt_host)):
            d_in = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
            d_out = torch.full((n + 32,), CANARY, dtype=torch.uint8, device="cuda")
            fn(key, d_in.data_ptr(), [0], [n], d_out.data_ptr(), [16], iv=iv)
            got = d_out.cpu().numpy()
            assert got[16:16 + n].tobytes() == want
            assert (got[:16] == CANARY).all() and (got[16 + n:] == CANARY).all()
            h_in = np.frombuffer(src, dtype=np.uint8).copy()
            h_out = np.full(n + 32, CANARY, dtype=np.uint8)
            off, ln, o16 = (np.array([v], dtype=np.uint64) for v in (0, n, 16))
            rc = host_fn(comp._ctx, key, h_in.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, iv, h_out.ctypes.data,
                         o16.ctypes.data)
            assert rc == 0, comp._L.zc_last_error(comp._ctx)
            assert h_out[16:16 + n].tobytes() == want
            assert (h_out[:16] == CANARY).all() and (h_out[16 + n:] == CANARY).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_chains_across_lanes_and_waves(torch_cuda, comp, n, decrypt):
    """Neighbouring chains differ in length; per-chain IVs; shuffled outputs.
    Packed back to back with non-zero IVs, a decrypt that took the block before
    a chain's first from memory instead of the chain's IV would differ here."""
    rng = np.random.default_rng(100 + n)
    lens = [int(v) for v in rng.choice(LENS, n)]
    lens[0] = 65552 if n > 1 else 1040
    ivs = rng.integers(1, 256, 16 * n, dtype=np.uint8).tobytes()
    _run_chains(torch_cuda, comp, rng, lens, decrypt, ivs)


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_null_iv_is_the_zero_iv(torch_cuda, comp, decrypt):
    rng = np.random.default_rng(7)
    _run_chains(torch_cuda, comp, rng, [16, 4096, 48, 1008, 32], decrypt, None, shuffle=False)


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_widest_divergence(torch_cuda, comp, decrypt):
    """A 16-byte chain beside a 256 KiB chain in one call."""
    rng = np.random.default_rng(8)
    ivs = rng.integers(1, 256, 32, dtype=np.uint8).tobytes()
    _run_chains(torch_cuda, comp, rng, [16, 256 << 10], decrypt, ivs)
    _run_chains(torch_cuda, comp, rng, [256 << 10, 16], decrypt, ivs)


def test_decrypt_around_the_tile_size(torch_cuda, comp):
    """Chains of TILE - 16, TILE, TILE + 16 and 2 TILE + 16 bytes back to back:
    the block before a tile's first is the previous tile's last ciphertext
    block, the block before a chain's first is that chain's IV."""
    rng = np.random.default_rng(9)
    lens = [TILE - 16, TILE, TILE + 16, 16, 2 * TILE + 16, TILE]
    ivs = rng.integers(1, 256, 16 * len(lens), dtype=np.uint8).tobytes()
    _run_chains(torch_cuda, comp, rng, lens, True, ivs)
    _run_chains(torch_cuda, comp, rng, lens, False, ivs)


def test_encrypt_in_place_and_round_trip(torch_cuda, comp):
    torch = torch_cuda
    rng = np.random.default_rng(10)
    lens = [int(v) for v in rng.choice(LENS, 70)] + [TILE + 16]
    n = len(lens)
    off, total = _layout(rng, lens, True)
    ivs = rng.integers(0, 256, 16 * n, dtype=np.uint8).tobytes()
    img = np.full(total, CANARY, dtype=np.uint8)
    plain = [rng.integers(0, 256, m, dtype=np.uint8) for m in lens]
    for o, p in zip(off, plain):
        img[o:o + len(p)] = p
    d = torch.from_numpy(img.copy()).cuda()
    comp.aes_encrypt(KEY, d.data_ptr(), off, lens, d.data_ptr(), off, iv=ivs)  # every chain over itself
    enc = d.cpu().numpy()
    want = img.copy()
    for k in range(n):
        if _afford(lens[k]):
            want[off[k]:off[k] + lens[k]] = np.frombuffer(
                aes_ref.cbc_encrypt(KEY, ivs[16 * k:16 * k + 16], plain[k].tobytes()), dtype=np.uint8)
        else:
            want[off[k]:off[k] + lens[k]] = enc[off[k]:off[k] + lens[k]]
    assert _first_diff(enc, want) is None
    d_back = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    comp.aes_decrypt(KEY, d.data_ptr(), off, lens, d_back.data_ptr(), off, iv=ivs)
    assert _first_diff(d_back.cpu().numpy(), img) is None  # the plaintext and every canary


def _raw(comp, decrypt, key, d_in, in_off, lens, d_out, out_off, iv=None):
    fn = comp._L.zc_aes128_cbc_decrypt if decrypt else comp._L.zc_aes128_cbc_encrypt
    a, b, c = (np.asarray(v, dtype=np.uint64) for v in (in_off, lens, out_off))
    rc = fn(comp._ctx, key, d_in, a.ctypes.data, b.ctypes.data, len(b), iv, d_out, c.ctypes.data)
    return rc, comp._L.zc_last_error(comp._ctx)


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_refusals(torch_cuda, comp, decrypt):
    """Every ZC_ERR_ARG case: a message, and not one byte written."""
    torch = torch_cuda
    d_in = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_out = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    i, o = d_in.data_ptr(), d_out.data_ptr()
    assert i % 16 == 0 and o % 16 == 0
    cases = {
        "zero length": (KEY, i, [0, 64], [32, 0], o, [0, 64]),
        "length not a multiple of 16": (KEY, i, [0], [40], o, [0]),
        "input offset not aligned": (KEY, i, [8], [32], o, [0]),
        "output offset not aligned": (KEY, i, [0], [32], o, [4]),
        "input base not aligned": (KEY, i + 8, [8], [32], o, [0]),
        "output base not aligned": (KEY, i, [0], [32], o + 1, [15]),
        "null key": (None, i, [0], [32], o, [0]),
        "outputs overlap": (KEY, i, [0, 64], [64, 64], o, [0, 48]),
        "outputs identical": (KEY, i, [0, 64], [64, 64], o, [128, 128]),
        "input over another chain's output": (KEY, o, [0, 512], [64, 64], o, [1024, 32]),
    }
    if decrypt:
        cases["in place"] = (KEY, o, [0], [64], o, [0])
        cases["input one block into its output"] = (KEY, o, [16], [64], o, [64])
    for name, (key, a, in_off, lens, b, out_off) in cases.items():
        rc, msg = _raw(comp, decrypt, key, a, in_off, lens, b, out_off)
        assert rc == -1, (name, rc)
        assert msg and msg != b"null context", name
        assert bool((d_out == CANARY).all()), name
    # the Python layer's own checks, then a good call clears the message
    with pytest.raises(ValueError):
        comp.aes_encrypt(KEY[:15], i, [0], [16], o, [0])
    rc, msg = _raw(comp, decrypt, KEY, i, [0], [16], o, [16])
    assert rc == 0 and msg == b""
    if not decrypt:  # encryption alone may run over its own input
        rc, msg = _raw(comp, False, KEY, o, [32], [32], o, [32])
        assert rc == 0, msg


# ---- bundle files ----

@pytest.fixture(scope="module")
def bundles(torch_cuda, comp):
    """Six bundles whose bodies are real zc_lzo_compress output, left on the
    device: (d_z, body_off, body_len, bodies as bytes, keyed prefixes)."""
    from zbackup_amd.bundle import lzo_capacity
    torch = torch_cuda
    pays = [payload("random", 1, 1), payload("random", 70000, 2), np.zeros(100001, np.uint8), payload("text", 30011, 3),
            payload("runs", 5000, 4), payload("repeats", 65536, 5)]
    pay_size = np.array([len(p) for p in pays], dtype=np.uint64)
    pay_off = np.concatenate([[0], np.cumsum(pay_size)[:-1]]).astype(np.uint64)
    z_off = np.concatenate([[0], np.cumsum([lzo_capacity(int(s)) for s in pay_size])]).astype(np.uint64)
    d_pay = torch.from_numpy(np.concatenate(pays)).cuda()
    d_z = torch.empty(int(z_off[-1]), dtype=torch.uint8, device="cuda")
    z_size = comp.compress(d_pay.data_ptr(), pay_off, pay_size, d_z.data_ptr(), z_off[:-1])
    z = d_z.cpu().numpy()
    bodies = [z[int(o):int(o) + int(s)].tobytes() for o, s in zip(z_off[:-1], z_size)]
    assert len(bodies[1]) > 70000  # incompressible
    rng = np.random.default_rng(11)
    prefixes = []
    for k, (body, residue) in enumerate(zip(bodies, [0, 1, 15, 0, 1, 15])):
        R = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        head = R + aes_ref.message(b"\x08\x01")  # BundleFileHeader{version = 1}
        # an info message of 130..145 bytes (a two-byte varint), sized for the residue wanted
        fill = 130 + (residue - (len(head) + 2 + 130 + len(body) + 8)) % 16
        prefixes.append(head + aes_ref.message(rng.integers(0, 256, fill, dtype=np.uint8).tobytes()))
        assert (len(prefixes[k]) + len(body) + 8) % 16 == residue
    return d_z, z_off[:-1], z_size, bodies, prefixes, pays


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_seal_matches_the_reference(torch_cuda, comp, bundles, keyed):
    from zbackup_amd.bundle import bundle_file_size
    torch = torch_cuda
    d_z, body_off, body_len, bodies, prefixes, _ = bundles
    key = KEY if keyed else None
    pre = prefixes if keyed else [p[16:] for p in prefixes]  # no R without a key
    want_files = [aes_ref.seal_ref(key, p, b) for p, b in zip(pre, bodies)]
    sizes = [len(f) for f in want_files]
    if keyed:
        pads = [s - (len(p) + len(b) + 8) for s, p, b in zip(sizes, pre, bodies)]
        assert pads == [16, 15, 1, 16, 15, 1]  # residue 0 takes the whole pad block
    rng = np.random.default_rng(12)
    file_off, total = _layout(rng, [(s + 15) // 16 * 16 for s in sizes], True)
    want = np.full(total, CANARY, dtype=np.uint8)
    for o, f in zip(file_off, want_files):
        want[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_files = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    got_size = comp.seal(key, pre, d_z.data_ptr(), body_off, body_len, d_files.data_ptr(), file_off)
    assert [int(s) for s in got_size] == sizes
    assert sizes == [bundle_file_size(len(p), len(b), keyed) for p, b in zip(pre, bodies)]
    at = _first_diff(d_files.cpu().numpy(), want)
    assert at is None, f"first wrong byte at {at} of {total}"
    assert comp.seal_host(key, pre, bodies) == want_files  # the host form


def _check_layout(lay, ref_lay):
    for name, v in ref_lay.items():
        assert int(lay[name]) == v, name


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_unseal_round_trip(torch_cuda, comp, bundles, keyed):
    torch = torch_cuda
    d_z, body_off, body_len, bodies, prefixes, _ = bundles
    key = KEY if keyed else None
    pre = prefixes if keyed else [p[16:] for p in prefixes]
    sizes = [aes_ref.file_size(len(p), len(b), keyed) for p, b in zip(pre, bodies)]
    rng = np.random.default_rng(13)
    caps = [(s + 15) // 16 * 16 for s in sizes]
    file_off, ftotal = _layout(rng, caps, True)
    plain_off, ptotal = _layout(rng, caps, True)
    d_files = torch.full((ftotal,), CANARY, dtype=torch.uint8, device="cuda")
    comp.seal(key, pre, d_z.data_ptr(), body_off, body_len, d_files.data_ptr(), file_off)
    d_plain = torch.full((ptotal,), CANARY, dtype=torch.uint8, device="cuda")
    layout = comp.unseal(key, d_files.data_ptr(), file_off, sizes, d_plain.data_ptr(), plain_off)
    got = d_plain.cpu().numpy()
    want = np.full(ptotal, CANARY, dtype=np.uint8)
    files = d_files.cpu().numpy()
    for k in range(len(sizes)):
        st, ref_lay, plain = aes_ref.unseal_ref(key, files[file_off[k]:file_off[k] + sizes[k]].tobytes())
        assert st == aes_ref.OK and int(layout[k]["status"]) == 0
        _check_layout(layout[k], ref_lay)
        assert plain == aes_ref.plaintext_ref(pre[k], bodies[k], keyed)
        want[plain_off[k]:plain_off[k] + sizes[k]] = np.frombuffer(plain, dtype=np.uint8)
        lay = layout[k]
        p = got[plain_off[k]:plain_off[k] + sizes[k]]
        assert p[int(lay["body_off"]):int(lay["body_off"] + lay["body_len"])].tobytes() == bodies[k]
        start = 16 if keyed else 0
        assert p[start:int(lay["info_off"] + lay["info_len"])].tobytes() == pre[k][start:]
    at = _first_diff(got, want)
    assert at is None, f"first wrong byte at {at} of {ptotal}"
    # the host form: (header, info, body) per bundle
    host_files = [files[o:o + s].tobytes() for o, s in zip(file_off, sizes)]
    for (hdr, info, body), p, b in zip(comp.unseal_host(key, host_files), pre, bodies):
        assert hdr == b"\x08\x01" and body == b and p.endswith(info) and len(info) >= 130


def _bad_files(key):
    """(name, file bytes, status) of files made from deliberately wrong plaintexts."""
    keyed = key is not None
    R = bytes(range(1, 17)) if keyed else b""
    prefix = R + aes_ref.message(b"\x08\x01") + aes_ref.message(b"info" * 9)
    body = bytes(range(200)) + b"x" * 3  # keyed: 16 + 3 + 37 + 4 + 203 + 4 = 267 -> pad 5
    good = aes_ref.plaintext_ref(prefix, body, keyed)
    a1_at = len(prefix)
    a2_at = a1_at + 4 + len(body)
    out = []

    def add(name, plain, status):
        out.append((name, aes_ref.encrypt_file(key, bytes(plain)), status))

    p = bytearray(good)
    p[a1_at + 1] ^= 0x40
    add("wrong A1", p, aes_ref.BAD_ADLER1)
    p = bytearray(good)
    p[a2_at + 3] ^= 0x01
    add("wrong A2", p, aes_ref.BAD_ADLER2)
    p = bytearray(good)
    p[a1_at + 10] ^= 0x80  # a body byte: A1 still holds
    add("wrong body byte", p, aes_ref.BAD_ADLER2)
    big = R + b"\xff\xff\xff\xff\x0f" + b"abc"  # a header length of 2^32 - 1
    add("varint length past the end", aes_ref.plaintext_ref(big, b"", keyed), aes_ref.TRUNCATED)
    add("varint of six bytes", aes_ref.plaintext_ref(R + b"\x80\x80\x80\x80\x80\x01" + b"a", b"", keyed),
        aes_ref.TRUNCATED)
    add("no room for A1 and A2", (R + b"\x00\x00\x01\x02\x03\x04" + b"\x0a" * 10) if keyed else b"\x00\x00\x01\x02\x03",
        aes_ref.TRUNCATED)
    if keyed:
        assert len(good) - a2_at - 4 == 5
        for name, last in (("pad byte 0", 0), ("pad byte 17", 17)):
            p = bytearray(good)
            p[-1] = last
            add(name, p, aes_ref.BAD_PADDING)
        p = bytearray(good)
        p[-3] = 4
        add("inconsistent pad bytes", p, aes_ref.BAD_PADDING)
        full = aes_ref.seal_ref(key, prefix, body)
        out.append(("cut to a non-multiple of 16", full[:-7], aes_ref.BAD_SIZE))
    out.append(("cut to 0 bytes", b"", aes_ref.BAD_SIZE))
    return out, aes_ref.seal_ref(key, prefix, body), (prefix, body)


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "plain"])
def test_unseal_statuses(torch_cuda, comp, keyed):
    """Each bad file gets its status; the good bundles in the same call stay OK."""
    torch = torch_cuda
    key = KEY if keyed else None
    bad, good, (prefix, body) = _bad_files(key)
    for name, f, st in bad:  # the restated format agrees on what is wrong with each
        assert aes_ref.unseal_ref(key, f)[0] == st, name
    flipped = bytearray(good)
    flipped[37] ^= 0x10  # one ciphertext byte: the test does not pin which check sees it
    files = [good] + [f for _, f, _ in bad] + [bytes(flipped), good]
    sizes = [len(f) for f in files]
    caps = [max(16, (s + 15) // 16 * 16) for s in sizes]
    rng = np.random.default_rng(14)
    file_off, ftotal = _layout(rng, caps, True)
    plain_off, ptotal = _layout(rng, caps, True)
    img = np.full(ftotal, CANARY, dtype=np.uint8)
    for o, f in zip(file_off, files):
        img[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_files = torch.from_numpy(img).cuda()
    d_plain = torch.full((ptotal,), CANARY, dtype=torch.uint8, device="cuda")
    layout = comp.unseal(key, d_files.data_ptr(), file_off, sizes, d_plain.data_ptr(), plain_off)
    status = [int(s) for s in layout["status"]]
    assert status[0] == 0 and status[-1] == 0
    for (name, _, st), got in zip(bad, status[1:]):
        assert got == st, (name, got, st)
    assert status[-2] != 0
    got = d_plain.cpu().numpy()
    plain = aes_ref.plaintext_ref(prefix, body, keyed)
    for k in (0, len(files) - 1):
        assert got[plain_off[k]:plain_off[k] + sizes[k]].tobytes() == plain
        _check_layout(layout[k], aes_ref.unseal_ref(key, good)[1])
    # nothing outside the plaintext extents was written
    mask = np.ones(ptotal, dtype=bool)
    for o, s in zip(plain_off, sizes):
        mask[o:o + s] = False
    assert (got[mask] == CANARY).all()
    # the host form raises with the status, or reports it
    with pytest.raises(Exception, match="status"):
        comp.unseal_host(key, files)
    loose = comp.unseal_host(key, files, strict=False)
    assert loose[0][2] == body and loose[-1][2] == body and [v for v in loose[1:-1] if not isinstance(v, int)] == []


def test_unseal_refusals(torch_cuda, comp):
    torch = torch_cuda
    d = torch.full((1024,), CANARY, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for file_off, plain_off in (([8], [512]), ([0], [520]), ([0], [16])):  # misaligned, misaligned, overlapping
        with pytest.raises(Exception, match="zc_bundle_unseal"):
            comp.unseal(KEY, p, file_off, [64], p, plain_off)
        assert bool((d == CANARY).all())
    with pytest.raises(Exception, match="zc_bundle_seal"):
        comp.seal(KEY, [b"p" * 20, b"q" * 20], p, [0, 0], [8, 8], p + 512, [0, 32])  # 48-byte files 32 apart
    with pytest.raises(Exception, match="zc_bundle_seal"):
        comp.seal(KEY, [b"p" * 20], p, [0], [8], p + 512, [8])
    assert bool((d == CANARY).all())


def test_sealed_backup_end_to_end(torch_cuda, comp):
    """stream -> chunks -> bundles -> lzo1x_1 -> sealed files (all on the GPU);
    then the files unsealed in shuffled order, the bodies decoded by liblzo2
    and the stream replayed by the Restorer."""
    from zbackup_amd import ZC_CHUNK_NEW, BackupCreator, Restorer
    from zbackup_amd.bundle import bundle_file_size, lzo_capacity, plan_bundles
    torch = torch_cuda
    if lzo_oracle.lzo_lib() is None:
        pytest.skip("liblzo2 not in this image")
    oracle.build()
    W = 4096
    a = payload("text", 700 << 10, 21)
    data = np.concatenate([a, payload("random", 600 << 10, 22), a[5:300 << 10], np.zeros(200 << 10, np.uint8),
                           payload("runs", (2 << 20) - (700 << 10) - (600 << 10) - (300 << 10) + 5 - (200 << 10), 23)])
    assert len(data) == 2 << 20
    d = torch.from_numpy(data).cuda()
    with BackupCreator(chunk_max_size=W, sha1=True) as bc:
        bc.chunk_device(d.data_ptr(), len(data))
        recs = bc.records()
        backup_data = bc.get_backup_data()
    seen, offs, sizes, ids = set(), [], [], []
    for r in recs[recs["kind"] == ZC_CHUNK_NEW]:
        cid = bytes(r["sha1"]) + int(r["rolling"]).to_bytes(8, "little")
        if cid not in seen:
            seen.add(cid)
            offs.append(int(r["offset"]))
            sizes.append(int(r["size"]))
            ids.append(cid)
    bundle_of, nb = plan_bundles(sizes, max_payload=256 << 10)
    assert nb >= 4
    d_payload = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    comp.gather(d.data_ptr(), offs, sizes, d_payload.data_ptr())
    pay_size = np.bincount(bundle_of, weights=sizes, minlength=nb).astype(np.uint64)
    pay_off = np.concatenate([[0], np.cumsum(pay_size)[:-1]]).astype(np.uint64)
    z_off = np.concatenate([[0], np.cumsum([lzo_capacity(int(s)) for s in pay_size])]).astype(np.uint64)
    d_z = torch.empty(int(z_off[-1]), dtype=torch.uint8, device="cuda")
    z_size = comp.compress(d_payload.data_ptr(), pay_off, pay_size, d_z.data_ptr(), z_off[:-1])
    # seal: R + BundleFileHeader + a stand-in BundleInfo (the ids and sizes; protobufs stay with the caller)
    rng = np.random.default_rng(24)
    infos = [[(ids[i], sizes[i]) for i in np.nonzero(bundle_of == k)[0]] for k in range(nb)]
    prefixes = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() + aes_ref.message(b"\x08\x01") +
                aes_ref.message(b"".join(cid + n.to_bytes(4, "little") for cid, n in info)) for info in infos]
    fsize = [bundle_file_size(len(p), int(z), True) for p, z in zip(prefixes, z_size)]
    f_off = np.concatenate([[0], np.cumsum(fsize)[:-1]]).astype(np.uint64)
    d_files = torch.empty(int(sum(fsize)), dtype=torch.uint8, device="cuda")
    assert [int(s) for s in comp.seal(KEY, prefixes, d_z.data_ptr(), z_off[:-1], z_size, d_files.data_ptr(), f_off)] == fsize
    files = d_files.cpu().numpy()
    assert files[int(f_off[1]):int(f_off[1]) + fsize[1]].tobytes() == aes_ref.seal_ref(
        KEY, prefixes[1], d_z[int(z_off[1]):int(z_off[1]) + int(z_size[1])].cpu().numpy().tobytes())
    # the restore: files in shuffled order
    order = [int(k) for k in rng.permutation(nb)]
    unsealed = comp.unseal_host(KEY, [files[int(f_off[k]):int(f_off[k]) + fsize[k]].tobytes() for k in order])
    read_infos = []
    for (hdr, info, _), k in zip(unsealed, order):
        assert hdr == b"\x08\x01"
        read_infos.append([(info[i:i + 24], int.from_bytes(info[i + 24:i + 28], "little")) for i in range(0, len(info), 28)])
        assert read_infos[-1] == infos[k]
    plan = Restorer.plan(backup_data, read_infos)
    assert plan.length == len(data)
    payloads = [lzo_oracle.unframe(unsealed[b_][2]) for b_ in plan.used]
    d_work = torch.from_numpy(plan.host_image(payloads)).cuda()
    d_out = torch.full((len(data) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    with Restorer(ctx=comp._ctx) as rs:
        n = rs.replay(plan, d_work.data_ptr(), d_out.data_ptr() + 16, len(data))
    assert n == len(data)
    out = d_out.cpu().numpy()
    assert (out[:16] == CANARY).all() and (out[16 + n:] == CANARY).all()
    assert np.array_equal(out[16:16 + n], data)
    assert hashlib.sha256(out[16:16 + n].tobytes()).digest() == hashlib.sha256(data.tobytes()).digest()
