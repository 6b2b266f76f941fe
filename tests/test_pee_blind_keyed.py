"""Keyed blind MED-PEE on the GPU (include/codec_tcc_blind_keyed.h), bit-exact against the
specification tests/pee_blind_keyed_spec.py: stego, info and payload bits of embed_blind_keyed /
decode_blind_keyed on the table of DESIGN §3m at B = 3 and B = 9 with mixed lengths; T chosen per
slice; a batch decoded from two embeds' slices; the per-slice-nonce AEAD entries against aead_spec and
against their namesakes; tampering; the DICOM round trip; the top-level calls."""
import numpy as np
import pytest

import aead_spec as AS
import pee_blind_cases as CS
import pee_blind_keyed_cases as KC
import pee_blind_keyed_spec as KSP
import pee_blind_spec as BS

pytestmark = pytest.mark.gpu

_spec = {}


def _want(name, n, g, seed, nonce=KC.NONCE):
    """(bits, spec stego, info, tag) of the case's cover with n payload bits at index g; built once."""
    k = (name, n, g, seed, nonce)
    if k not in _spec:
        img = KC.cover(name)
        bits = KC.payload(n, seed)
        stego, info, _p, tag = KSP.embed(img, bits, KC.CASE[name][2], KC.KEY, nonce, g, CS.top(img.dtype))
        _spec[k] = (bits, stego, info, tag)
    return _spec[k]


def _codec(B, img, T, tmax=16):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, img.shape[0], img.shape[1], dtype=str(img.dtype), T=T, tmax=tmax, maxval=CS.top(img.dtype))


def _frame_tags(stego_slices):
    """The 16 tag bytes the stego carries, read by the unkeyed spec decoder from a copy with side bit 41 clear."""
    out = []
    for st in stego_slices:
        plain = st.copy()
        plain.ravel()[plain.size - 1 - 41] &= ~np.asarray(1, plain.dtype)
        user = BS.decode(plain, verify=False)[0]
        out.append(KSP.unframe(user)[2])
    return out


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("name", [c[0] for c in KC.CASES])
def test_gpu_blind_keyed_parity(name, B):
    """Stego and info bit for bit the spec's, ts the codec's T; a refused slice is its cover; the
    embedded ones decode, on a codec built with another T, to the payloads and the covers."""
    torch = pytest.importorskip("torch")
    _n, _src, T, _E, lengths, cap = KC.CASE[name]
    img = KC.cover(name)
    index0 = KC.index(name, B)
    ns = [lengths[(b + (1 if B == 9 else 0)) % len(lengths)] for b in range(B)]   # B = 9 reaches the table's last lengths
    want = [_want(name, ns[b], index0 + b, b) for b in range(B)]
    covers = np.stack([img] * B)
    cov = torch.from_numpy(covers).cuda()
    codec = _codec(B, img, T)
    stego, info, ts = codec.embed_blind_keyed(cov, [w[0] for w in want], key=KC.KEY, nonce=KC.NONCE, index0=index0,
                                              check=False)
    got_st, got_info = stego.cpu().numpy(), info.cpu().numpy()
    assert got_info.shape == (B, 6) and ts.cpu().tolist() == [T] * B
    print(name, B, "n_ct", ns, "status", got_info[:, 0].tolist())
    for b, (_bits, st, winfo, _tag) in enumerate(want):
        assert tuple(int(v) for v in got_info[b]) == tuple(winfo), (name, b, got_info[b], winfo)
        assert (winfo[0] == 0) == (ns[b] <= cap) and winfo[1] == 224 + ns[b]
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"{name}: stego of slice {b} (n_ct = {ns[b]})")
        if winfo[0]:
            np.testing.assert_array_equal(got_st[b], img)
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)   # the embed left the covers alone
    keep = [b for b in range(B) if want[b][2][0] == 0]
    if not keep:
        with pytest.raises(ValueError, match="header"):
            codec.decode_blind_keyed(stego, KC.KEY)
        return
    other = _codec(len(keep), img, 13)   # decode takes T and maxval from the headers
    out, back = other.decode_blind_keyed(torch.from_numpy(got_st[keep]).cuda(), KC.KEY)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
    for k, b in enumerate(keep):
        np.testing.assert_array_equal(out[k], want[b][0], err_msg=f"{name}: bits of slice {b}")


def test_gpu_blind_keyed_tag_is_the_per_slice_routes():
    """The tag a keyed blind slice carries is enc.tag of PeeCodec.embed(key=) for the same (cover,
    payload, key, nonce, index), and the spec's."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import aead
    img = KC.cover("smooth")
    ns, index0 = (64, 33, 160), 77
    want = [_want("smooth", n, index0 + b, 20 + b) for b, n in enumerate(ns)]
    cov = torch.from_numpy(np.stack([img] * 3)).cuda()
    codec = _codec(3, img, 4)
    bits = [w[0] for w in want]
    stego, _info, _ts = codec.embed_blind_keyed(cov, bits, key=KC.KEY, nonce=KC.NONCE, index0=index0)
    enc = codec.embed(cov, bits, key=KC.KEY, nonce=KC.NONCE, index0=index0)
    assert aead.tag_bytes(enc.tag) == [w[3] for w in want] == _frame_tags(stego.cpu().numpy())


def test_gpu_blind_keyed_chosen_t():
    """tmax = 8: ts and the stegos are the spec's at the smallest T that takes frame and ciphertext."""
    torch = pytest.importorskip("torch")
    for name, table in KC.AUTO:
        img = KC.cover(name)
        B = len(table)
        bits = [KC.payload(n, 30 + q) for q, (n, _t) in enumerate(table)]
        cov = torch.from_numpy(np.stack([img] * B)).cuda()
        codec = _codec(B, img, 2)
        stego, info, ts = codec.embed_blind_keyed(cov, bits, key=KC.KEY, nonce=KC.NONCE, index0=5, tmax=KC.TMAX, check=False)
        assert ts.cpu().tolist() == [t for _n, t in table]
        got, ginfo = stego.cpu().numpy(), info.cpu().tolist()
        for b in range(B):
            st, winfo, T, _tag = KSP.embed_auto(img, bits[b], KC.TMAX, KC.KEY, KC.NONCE, 5 + b, 4095)
            assert T == table[b][1] and tuple(ginfo[b]) == tuple(winfo)
            np.testing.assert_array_equal(got[b], st)
        out, back = codec.decode_blind_keyed(stego, KC.KEY)
        for b in range(B):
            np.testing.assert_array_equal(out[b], bits[b])
        np.testing.assert_array_equal(back.cpu().numpy(), cov.cpu().numpy())
    # a slice no T <= tmax serves: refused, T 0, the cover; check=True names it
    img = KC.cover("smooth")
    cov = torch.from_numpy(np.stack([img] * 2)).cuda()
    codec = _codec(2, img, 2)
    bits = [KC.payload(100, 1), KC.payload(2000, 2)]
    stego, info, ts = codec.embed_blind_keyed(cov, bits, key=KC.KEY, tmax=KC.TMAX, check=False)
    assert ts.cpu().tolist() == [4, 0] and info[:, 0].cpu().tolist() == [0, 1]
    np.testing.assert_array_equal(stego.cpu().numpy()[1], img)
    with pytest.raises(ValueError, match=r"embed_blind_keyed: .*capacity in slices \[1\]"):
        codec.embed_blind_keyed(cov, bits, key=KC.KEY, tmax=KC.TMAX)


def test_gpu_blind_keyed_mixed_batch():
    """Two embeds under one key with different nonces, index0 = 0 and 2^31 - 3; their stegos
    concatenated out of order decode in one B = 6 call: every slice brings its own nonce and index."""
    torch = pytest.importorskip("torch")
    img = KC.cover("smooth")
    codec = _codec(3, img, 4)
    cov = torch.from_numpy(np.stack([img] * 3)).cuda()
    n1, n2 = bytes(range(8)), bytes(range(100, 108))
    b1 = [KC.payload(n, 40 + q) for q, n in enumerate((0, 65, 160))]
    b2 = [KC.payload(n, 50 + q) for q, n in enumerate((33, 1, 64))]
    s1, _i1, _t1 = codec.embed_blind_keyed(cov, b1, key=KC.KEY, nonce=n1, index0=0)
    s2, _i2, _t2 = codec.embed_blind_keyed(cov, b2, key=KC.KEY, nonce=n2, index0=(1 << 31) - 3)
    np.testing.assert_array_equal(s2.cpu().numpy()[2], KSP.embed(img, b2[2], 4, KC.KEY, n2, (1 << 31) - 1, 4095)[0])
    order = [(1, 2), (0, 1), (1, 0), (0, 2), (0, 0), (1, 1)]
    hosts = (s1.cpu().numpy(), s2.cpu().numpy())
    mixed = torch.from_numpy(np.stack([hosts[w][b] for w, b in order])).cuda()
    out, back = _codec(6, img, 2).decode_blind_keyed(mixed, KC.KEY)
    for k, (w, b) in enumerate(order):
        np.testing.assert_array_equal(out[k], (b1, b2)[w][b], err_msg=f"slice {k}")
    np.testing.assert_array_equal(back.cpu().numpy(), np.stack([img] * 6))


ROW_BITS = (0, 1, 63, 64, 65, 511, 512, 513, 20000)


def _rows_case(torch):
    """Nine rows of ROW_BITS bits with nine distinct (g, nonce) triples, on the host and the device."""
    from codec_tcc_amd import aead
    B, rw = len(ROW_BITS), (max(ROW_BITS) + 63) // 64
    rng = np.random.default_rng(77)
    rows = rng.integers(-(1 << 63), (1 << 63) - 1, (B, rw), dtype=np.int64, endpoint=True)   # set bits past every length
    gs = [0, 1, (1 << 31) - 1, 12345, 7, 1 << 30, 2, 99, 65536]
    nonces = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(B)]
    n12 = np.array([[g] + [int.from_bytes(nc[4 * i:4 * i + 4], "little") for i in range(2)] for g, nc in zip(gs, nonces)],
                   dtype=np.uint32)
    dev = (torch.from_numpy(rows).cuda(), torch.tensor(ROW_BITS, dtype=torch.int32).cuda(),
           torch.from_numpy(n12.view(np.int32)).cuda(), aead.upload_ctx(KC.KEY, bytes(8)))
    words = [[int(v) & 0xFFFFFFFFFFFFFFFF for v in r] for r in rows]
    return words, gs, nonces, dev


def _u64(t):
    return [[int(v) & 0xFFFFFFFFFFFFFFFF for v in r] for r in t.cpu().numpy()]


def test_gpu_chacha20_rows_n_and_release_n():
    """chacha20_rows_n against aead_spec under nine distinct nonce12 rows on the row lengths 0 .. 513
    and 20000 bits; release_n: a flipped bit in one tag word zeroes that slice's row alone."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import aead
    words, gs, nonces, (rows, lens, n12, ctx) = _rows_case(torch)
    B = len(ROW_BITS)
    want = [AS.crypt_row(KC.KEY, nonces[b], gs[b], words[b], ROW_BITS[b]) for b in range(B)]
    ct = aead.chacha20_rows_n(ctx, n12, rows, lens)
    assert _u64(ct) == want
    assert _u64(aead.chacha20_rows_n(ctx, n12, ct, lens)) == \
        [AS.bytes_row(AS.row_bytes(words[b], ROW_BITS[b]), len(words[b])) for b in range(B)]
    tags = aead.poly1305_tags_n(ctx, n12, None, ct, lens)
    assert aead.tag_bytes(tags) == [AS.tag(KC.KEY, nonces[b], gs[b], b"", want[b], ROW_BITS[b]) for b in range(B)]
    forged = tags.clone()
    hit = {1: 0, 3: 1, 4: 2, 8: 3}   # slice -> the tag word with a flipped bit
    for b, w in hit.items():
        forged[b, w] ^= 1 << (5 + 7 * w)
    pt, ok = aead.release_n(ctx, n12, tags, forged, ct, lens)
    assert ok.cpu().tolist() == [0 if b in hit else 1 for b in range(B)]
    plain = [AS.bytes_row(AS.row_bytes(words[b], ROW_BITS[b]), len(words[b])) for b in range(B)]
    assert _u64(pt) == [[0] * len(words[b]) if b in hit else plain[b] for b in range(B)]
    pt2, ok2 = aead.release_n(ctx, n12, tags, tags.clone(), ct, lens)
    assert ok2.cpu().tolist() == [1] * B and _u64(pt2) == plain


@pytest.mark.parametrize("nbytes", [0, 15, 16, 17, 64 * 96 * 2])
def test_gpu_poly1305_tags_n_aad(nbytes):
    """poly1305_tags_n against aead_spec with AAD of 0, 15, 16, 17 bytes and one slice's worth."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import aead
    words, gs, nonces, (rows, lens, n12, ctx) = _rows_case(torch)
    B = len(ROW_BITS)
    data = np.random.default_rng(5 + nbytes).integers(0, 256, (B, max(nbytes, 1)), dtype=np.uint8)
    aad = torch.from_numpy(data).cuda() if nbytes else None
    tags = aead.poly1305_tags_n(ctx, n12, aad, rows, lens)
    assert aead.tag_bytes(tags) == [AS.tag(KC.KEY, nonces[b], gs[b], data[b].tobytes() if nbytes else b"", words[b], ROW_BITS[b])
                                    for b in range(B)]
    if nbytes:   # no rows: an empty ciphertext
        assert aead.tag_bytes(aead.poly1305_tags_n(ctx, n12, aad)) == \
            [AS.tag(KC.KEY, nonces[b], gs[b], data[b].tobytes(), [0], 0) for b in range(B)]


@pytest.mark.parametrize("index0", [0, (1 << 31) - 9])
def test_gpu_n_entries_equal_their_namesakes(index0):
    """For nonce12[b] = (index0 + b, the ctx's nonce) the three entries give what the existing ones give."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import aead
    _words, _gs, _nonces, (rows, lens, _n12, _ctx) = _rows_case(torch)
    B = len(ROW_BITS)
    ctx = aead.upload_ctx(KC.KEY, KC.NONCE)
    n12 = aead.nonce12_rows(KC.NONCE, index0, B)
    assert n12.cpu().numpy().view(np.uint32)[:, 0].tolist() == [index0 + b for b in range(B)]
    aad = torch.from_numpy(np.random.default_rng(3).integers(0, 4096, (B, 64, 96)).astype(np.uint16)).cuda()
    ct = aead.chacha20_rows(ctx, rows, lens, index0)
    assert torch.equal(aead.chacha20_rows_n(ctx, n12, rows, lens), ct)
    tags = aead.poly1305_tags(ctx, aad, ct, lens, index0)
    assert torch.equal(aead.poly1305_tags_n(ctx, n12, aad, ct, lens), tags)
    forged = tags.clone()
    forged[2, 3] ^= -(1 << 31)   # the top bit of an int32 word
    pt, ok = aead.release(ctx, tags, forged, ct, lens, index0)
    pt_n, ok_n = aead.release_n(ctx, n12, tags, forged, ct, lens)
    assert torch.equal(pt_n, pt) and torch.equal(ok_n, ok) and ok.cpu().tolist() == [1, 1, 0] + [1] * (B - 3)


def test_gpu_blind_keyed_tampering():
    """A changed pixel, a wrong key, verify=False, and a cleared flag bit on a B = 3 stego."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import IntegrityError
    img = KC.cover("planted1")
    H, W = img.shape
    ns = (33, 121, 0)
    bits = [KC.payload(n, 60 + q) for q, n in enumerate(ns)]
    cov = torch.from_numpy(np.stack([img] * 3)).cuda()
    codec = _codec(3, img, 4)
    stego, info, _ts = codec.embed_blind_keyed(cov, bits, key=KC.KEY, nonce=KC.NONCE, index0=9)
    region_row = int(info[1, 5])
    host = stego.cpu().numpy()
    bent = host.copy()
    assert 20 < region_row
    bent[1, 20, 30] ^= 1   # outside the reserved rows
    with pytest.raises(IntegrityError) as e:
        codec.decode_blind_keyed(torch.from_numpy(bent).cuda(), KC.KEY)
    assert e.value.keyed and e.value.slices == [1] and not e.value.rows[1].any()
    out, _back = codec.decode_blind_keyed(torch.from_numpy(bent).cuda(), KC.KEY, verify=False)
    np.testing.assert_array_equal(out[0], bits[0])
    np.testing.assert_array_equal(out[2], bits[2])
    np.testing.assert_array_equal(np.unpackbits(e.value.rows[0].view(np.uint8), bitorder="little")[:ns[0]], bits[0])
    with pytest.raises(IntegrityError) as e:
        codec.decode_blind_keyed(stego, bytes(32))
    assert e.value.keyed and e.value.slices == [0, 1, 2] and not e.value.rows.any()
    out, back = codec.decode_blind_keyed(stego, KC.KEY, verify=False)
    for b in range(3):
        np.testing.assert_array_equal(out[b], bits[b])
    np.testing.assert_array_equal(back.cpu().numpy(), cov.cpu().numpy())
    out, _back = codec.decode_blind_keyed(stego, KC.KEY, verify="require")   # the tag satisfies it
    np.testing.assert_array_equal(out[1], bits[1])
    with pytest.raises(ValueError, match=r"flags = 0x2"):   # the unkeyed decoder keeps refusing flag bit 1
        codec.decode_blind(stego)
    clear = host.copy()
    clear.reshape(3, -1)[:, H * W - 1 - 41] &= 0xFFFE
    with pytest.raises(ValueError, match=r"slices \[0, 1, 2\].*decode_blind"):
        codec.decode_blind_keyed(torch.from_numpy(clear).cuda(), KC.KEY)
    framed, back = codec.decode_blind(torch.from_numpy(clear).cuda())
    for b in range(3):
        np.testing.assert_array_equal(framed[b], KSP.seal(img, bits[b], KC.KEY, KC.NONCE, 9 + b)[0])
        assert framed[b].size == 224 + ns[b]
    np.testing.assert_array_equal(back.cpu().numpy(), cov.cpu().numpy())


def test_gpu_blind_keyed_dicom_round_trip(tmp_path):
    """encode_dicom_pee_keyed writes a plain DICOM whose pixels are the spec's keyed stego;
    decode_dicom_pee_keyed reads it with the key alone; decode_dicom_pee refuses it."""
    import golden_io
    from codec_tcc_amd import IntegrityError, dicom, framing, pipeline
    img = golden_io.images()["pe"]   # 512 x 512 uint16
    path = str(tmp_path / "keyed.dcm")
    res = pipeline.encode_dicom_pee_keyed(img, "a keyed blind payload", path, KC.KEY, T=3, nonce=KC.NONCE, maxval=4095)
    bits = framing.to_bits("a keyed blind payload")
    st, info, _p, _tag = KSP.embed(img, bits, 3, KC.KEY, KC.NONCE, 0, 4095)
    assert (res["T"], res["nonce"], res["L"], res["status"], res["n_user"]) == (3, KC.NONCE, bits.size, 0, 224 + bits.size)
    assert info[0] == 0
    pixels, _attrs = dicom.read_dicom(path)
    np.testing.assert_array_equal(pixels, st)
    got, cover = pipeline.decode_dicom_pee_keyed(path, KC.KEY)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(cover, img)
    with pytest.raises(ValueError, match="flags"):
        pipeline.decode_dicom_pee(path)
    with pytest.raises(IntegrityError):
        pipeline.decode_dicom_pee_keyed(path, bytes(32))
    auto = pipeline.encode_dicom_pee_keyed(img, "a keyed blind payload", str(tmp_path / "auto.dcm"), KC.KEY, tmax=8, maxval=4095)
    assert auto["T"] == KSP.choose(img, bits.size, 8, 4095) >= 1 and len(auto["nonce"]) == 8
    np.testing.assert_array_equal(pipeline.decode_dicom_pee_keyed(str(tmp_path / "auto.dcm"), KC.KEY)[0], bits)


def test_gpu_blind_keyed_top_level():
    """encode_blind_keyed / decode_blind_keyed: numpy in, the spec's stego out; each decoder refuses
    the other's stegos with a ValueError."""
    import codec_tcc_amd as pkg
    cover = KC.cover("planted3").copy()   # writable: the call wraps it in a tensor
    bits = KC.payload(55, 9)
    stego, info, ts = pkg.encode_blind_keyed(cover, [bits], KC.KEY, T=4, nonce=KC.NONCE, index0=12, maxval=4095)
    st, want, _p, _tag = KSP.embed(cover, bits, 4, KC.KEY, KC.NONCE, 12, 4095)
    assert ts.cpu().tolist() == [4] and tuple(info.cpu().tolist()[0]) == tuple(want)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
    out, back = pkg.decode_blind_keyed(stego.cpu().numpy(), KC.KEY)
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], cover)
    with pytest.raises(ValueError, match="flags"):
        pkg.decode_blind(stego)
    plain, _i = pkg.encode_blind(cover, [bits], T=4, maxval=4095)
    with pytest.raises(ValueError, match="decode_blind"):
        pkg.decode_blind_keyed(plain, KC.KEY)
    with pytest.raises(ValueError, match=r"capacity in slices \[0\]"):
        pkg.encode_blind_keyed(cover, [KC.payload(56, 1)], KC.KEY, T=4, maxval=4095)
    s2, _i2, t2 = pkg.encode_blind_keyed(cover, [KC.payload(100, 1)], KC.KEY, tmax=8, maxval=4095)
    assert t2.cpu().tolist() == [5]
    np.testing.assert_array_equal(pkg.decode_blind_keyed(s2, KC.KEY, restore=False)[0][0], KC.payload(100, 1))
