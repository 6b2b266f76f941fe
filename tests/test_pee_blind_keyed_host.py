"""Keyed blind MED-PEE without a GPU: the spec tests/pee_blind_keyed_spec.py against the scalar
restatement tests/pee_blind_keyed_scalar.py against the known answers
tests/golden/pee_blind_keyed_kat.json on every case of tests/pee_blind_keyed_cases.py; the frame's
bit order and the flag bit written out by hand; the tag against aead_spec; the argument and header
refusals of codec_tcc_amd; the loader's entry list."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import aead_spec as AS
import pee_blind_cases as CS
import pee_blind_keyed_cases as KC
import pee_blind_keyed_scalar as KS
import pee_blind_keyed_spec as KSP
import pee_blind_spec as BS
from codec_tcc_amd import _lib, blind, build

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [c[0] for c in KC.CASES]


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "pee_blind_keyed_kat.json")) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


@pytest.mark.parametrize("name", NAMES)
def test_spec_scalar_and_known_answers_agree(name, kat):
    """Stego, info and tag of the two statements and of the known answers agree on the table of
    DESIGN §3m; E and the keyed capacity are the table's; a refused slice is its cover; an embedded
    one decodes, by both statements, to the payload and the cover."""
    _n, _src, T, E, lengths, cap = KC.CASE[name]
    img = KC.cover(name)
    mv, nbytes = CS.top(img.dtype), img.dtype.itemsize
    k = next(c for c in kat["cases"] if c["case"] == name)
    assert (bytes.fromhex(kat["key"]), bytes.fromhex(kat["nonce"])) == (KC.KEY, KC.NONCE)
    assert (k["T"], k["maxval"], k["cover_sha256"]) == (T, mv, _sha(img))
    assert KSP.capacity(img, T, mv) == cap == k.get("capacity", cap)
    assert len(k["runs"]) == len(lengths)
    small = img.size <= 64 * 96
    rows = img.astype(np.int64).tolist()
    for q, (n, run) in enumerate(zip(lengths, k["runs"])):
        bits, g = KC.payload(n, q), KC.index(name, q)
        stego, info, _p, tag = KSP.embed(img, bits, T, KC.KEY, KC.NONCE, g, mv)
        assert (run["n_ct"], run["g"]) == (n, g)
        assert tuple(info) == tuple(run["info"]) and tag.hex() == run["tag"] and _sha(stego) == run["stego_sha256"], (name, n)
        assert info[1] == 224 + n and (info[0] == 0) == (n <= cap)
        if small or q == 0:   # the scalar statement again (the known answers are its output)
            s2, i2, t2 = KS.embed(rows, bits.tolist(), T, mv, nbytes, KC.KEY, KC.NONCE, g)
            assert tuple(i2) == tuple(info) and t2 == tag and s2 == stego.astype(np.int64).tolist()
        if info[0]:
            assert info[0] == 1
            np.testing.assert_array_equal(stego, img)
            continue
        assert info[2] == (E[q] if isinstance(E, tuple) else E)
        assert [int(v) for v in BS.read_words(stego, 0, 6 + info[2])] == run["words"]
        got, back, h = KSP.decode(stego, KC.KEY)
        np.testing.assert_array_equal(got, bits)
        np.testing.assert_array_equal(back, img)
        assert (h["flags"], h["g"], h["nonce"], h["tag"], h["n_user"]) == (2, g, KC.NONCE, tag, 224 + n)
        if small:
            g2, b2, f2 = KS.decode(stego.astype(np.int64).tolist(), nbytes, KC.KEY)
            assert g2 == bits.tolist() and b2 == rows and f2 == (g, KC.NONCE, tag)


def test_auto_table(kat):
    """The T chosen at tmax = 8 by the spec, the scalar statement and the known answers: the table's."""
    for (name, table), k in zip(KC.AUTO, kat["auto"]):
        img = KC.cover(name)
        mv = CS.top(img.dtype)
        assert k["case"] == name and k["tmax"] == KC.TMAX
        assert [tuple(v) for v in k["chosen"]] == list(table)
        for n, T in table:
            assert KSP.choose(img, n, KC.TMAX, mv) == T
            st, info, T2, _tag = KSP.embed_auto(img, KC.payload(n, 1), KC.TMAX, KC.KEY, KC.NONCE, 3, mv)
            assert T2 == T and info[0] == 0
            assert int(BS.read_words(st, 1, 1)[0]) & 0xFF == T
    assert KSP.choose(KC.cover("smooth"), 2000, KC.TMAX, 4095) == 0
    st, info, T, _tag = KSP.embed_auto(KC.cover("smooth"), KC.payload(2000, 1), KC.TMAX, KC.KEY, KC.NONCE, 3, 4095)
    assert T == 0 and info[0] == 1
    np.testing.assert_array_equal(st, KC.cover("smooth"))


def test_frame_bit_order_and_flag_by_hand():
    """One case spelled out: the user stream's 64-bit words are g | nonce_lo << 32, nonce_hi | tag0 <<
    32, tag1 | tag2 << 32, tag3 | CT[0:32] << 32, the ciphertext following 32 bits off a word; side
    bit 41 (bit 0 of pixel H W - 1 - 41) is the one difference from the unkeyed stego of those bits."""
    img = KC.cover("planted1")
    H, W = img.shape
    n, g = 33, 0x01020304
    bits = KC.payload(n, 5)
    stego, info, _p, tag = KSP.embed(img, bits, 4, KC.KEY, KC.NONCE, g, 4095)
    assert info[:4] == (0, 224 + n, 1, 224)
    words = [int(v) for v in BS.read_words(stego, 0, 6)]
    assert words[0] == 0x4D504231 and words[1] == 4 | (2 << 8) | (4095 << 16) and words[2] == 257 and words[5] == 0
    assert (int(stego.ravel()[H * W - 1 - 41]) & 1) == 1
    plain = stego.copy()
    plain.ravel()[H * W - 1 - 41] &= 0xFFFE
    user, cover, h = BS.decode(plain)   # the unkeyed decoder reads the framed bits once the flag is clear
    np.testing.assert_array_equal(cover, img)
    assert h["flags"] == 0 and user.size == 257
    with pytest.raises(ValueError, match="flags"):
        BS.decode(stego)
    unkeyed, _i, _p2 = BS.embed(img, user, 4, 4095)
    assert np.flatnonzero(unkeyed != stego).tolist() == [H * W - 1 - 41]
    padded = np.concatenate([user, np.zeros(320 - user.size, np.uint8)])
    w64 = [int(v) for v in np.packbits(padded, bitorder="little").view("<u8")]
    nlo, nhi = int.from_bytes(KC.NONCE[:4], "little"), int.from_bytes(KC.NONCE[4:], "little")
    t = AS.tag_words(tag)
    ct = AS.crypt_row(KC.KEY, KC.NONCE, g, [int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")], n)
    assert w64[0] == g | (nlo << 32)
    assert w64[1] == nhi | (t[0] << 32)
    assert w64[2] == t[1] | (t[2] << 32)
    assert w64[3] == t[3] | ((ct[0] & 0xFFFFFFFF) << 32)
    assert w64[4] == ct[0] >> 32 and ct[0] >> 33 == 0
    # byte k of the frame in user bits 8k .. 8k+7, LSB first
    frame = g.to_bytes(4, "little") + KC.NONCE + tag
    for kbyte in (0, 3, 4, 11, 12, 27):
        assert sum(int(user[8 * kbyte + j]) << j for j in range(8)) == frame[kbyte]


@pytest.mark.parametrize("name", ["smooth", "u8"])
def test_tag_is_the_per_slice_routes(name):
    """The frame's tag is aead_spec.tag of (cover bytes as they lie, the payload's ciphertext), i.e.
    what PeeCodec.embed(key=) computes for the same (cover, payload, key, nonce, g)."""
    img = KC.cover(name)
    n, g = 64, 11
    bits = KC.payload(n, 2)
    row = [int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")]
    ct = AS.crypt_row(KC.KEY, KC.NONCE, g, row, n)
    want = AS.tag(KC.KEY, KC.NONCE, g, img.astype(img.dtype.newbyteorder("<")).tobytes(), ct, n)
    _st, _info, _p, tag = KSP.embed(img, bits, KC.CASE[name][2], KC.KEY, KC.NONCE, g, CS.top(img.dtype))
    assert tag == want
    assert KS.user_bits(img.astype(np.int64).tolist(), bits.tolist(), img.dtype.itemsize, KC.KEY, KC.NONCE, g)[1] == want


def test_spec_decode_refusals():
    img = KC.cover("smooth")
    bits = KC.payload(40, 1)
    stego, _info, _p, _tag = KSP.embed(img, bits, 4, KC.KEY, KC.NONCE, 5, 4095)
    with pytest.raises(KSP.TagMismatch):
        KSP.decode(stego, bytes(32))
    np.testing.assert_array_equal(KSP.decode(stego, KC.KEY, verify=False)[0], bits)
    bent = stego.copy()
    bent[3, 3] ^= 1
    with pytest.raises(KSP.TagMismatch):
        KSP.decode(bent, KC.KEY)
    with pytest.raises(ValueError, match="tag mismatch"):
        KS.decode(bent.astype(np.int64).tolist(), 2, KC.KEY)
    unkeyed = BS.embed(img, bits, 4, 4095)[0]
    with pytest.raises(ValueError, match="flags"):
        KSP.decode(unkeyed, KC.KEY)
    with pytest.raises(ValueError, match="keyed"):
        KS.decode(unkeyed.astype(np.int64).tolist(), 2, KC.KEY)


def _hdr(flags, n_user, E=0, end=1000, T=4, maxval=4095):
    return [blind.MAGIC, T | (flags << 8) | (maxval << 16), n_user, E, end, 0]


def test_parse_header_keyword():
    """keyed=True admits exactly flags 2 with n_user >= 224; the default keeps today's behaviour."""
    H, W = 64, 96
    h = blind.parse_header(_hdr(2, 300), H, W, 65535, keyed=True)
    assert (h["flags"], h["n_user"], h["L"]) == (2, 300, 492)
    assert blind.parse_header(_hdr(2, 224, end=415), H, W, 65535, keyed=True)["n_user"] == 224
    for flags in (0, 1, 3, 4, 0x82):
        with pytest.raises(ValueError, match="flags"):
            blind.parse_header(_hdr(flags, 300), H, W, 65535, keyed=True)
    for flags in (0, 1):
        with pytest.raises(ValueError, match="decode_blind"):
            blind.parse_header(_hdr(flags, 300), H, W, 65535, keyed=True)
    with pytest.raises(ValueError, match="n_user = 223"):
        blind.parse_header(_hdr(2, 223), H, W, 65535, keyed=True)
    # without the keyword: flags 0 and 1 parse, bit 1 is refused
    assert blind.parse_header(_hdr(0, 300), H, W, 65535)["flags"] == 0
    assert blind.parse_header(_hdr(1, 300), H, W, 65535)["flags"] == 1
    for flags in (2, 3):
        with pytest.raises(ValueError, match=r"flags = 0x[23] \(bit 0 alone is defined\)"):
            blind.parse_header(_hdr(flags, 300), H, W, 65535)
        with pytest.raises(ValueError, match="flags"):
            blind.parse_header(_hdr(flags, 300), H, W, 65535, keyed=False)
    # all slices at once, naming the bad ones
    hdrs = np.array([_hdr(2, 300) + [0, 0], _hdr(0, 300) + [0, 0], _hdr(2, 223) + [0, 0], _hdr(2, 224) + [0, 0]], dtype=np.uint32)
    with pytest.raises(ValueError, match=r"keyed blind MED-PEE header in slices \[1, 2\].*decode_blind.*n_user = 223"):
        blind.parse_headers(hdrs, H, W, 2, keyed=True)
    good = blind.parse_headers(hdrs[[0, 3]], H, W, 2, keyed=True)
    assert good["n_user"].tolist() == [300, 224] and good["flags"].tolist() == [2, 2]
    with pytest.raises(ValueError, match=r"slices \[0, 2, 3\]"):
        blind.parse_headers(hdrs, H, W, 2)
    assert blind.KEYED_FRAME_BITS == KSP.FRAME_BITS == 224 and blind.FLAG_KEYED == KSP.FLAG_KEYED == 2


def test_argument_refusals():
    """Key, nonce, index and every blind argument rule as ValueError before any GPU work (this runs
    without a GPU); the unkeyed calls keep refusing key=."""
    import codec_tcc_amd as pkg
    from codec_tcc_amd import pipeline
    cover = CS.smooth(64, 96)
    key = KC.KEY
    for bad in (None, b"short", "k" * 32, bytes(33), 7):
        with pytest.raises(ValueError, match="key"):
            pkg.encode_blind_keyed(cover, [b"x"], bad)
    for bad in (b"1234567", bytes(12), "12345678", 5):
        with pytest.raises(ValueError, match="nonce"):
            pkg.encode_blind_keyed(cover, [b"x"], key, nonce=bad)
    for bad in (-1, 1.5, True, (1 << 31) + 1, 1 << 32):   # (0x80000000 alone is aead's stream index, as in embed(key=))
        with pytest.raises(ValueError, match="ind"):
            pkg.encode_blind_keyed(cover, [b"x"], key, index0=bad)
    with pytest.raises(ValueError, match="ind"):   # the batch's last index
        pkg.encode_blind_keyed(np.stack([cover] * 3), [b"x"] * 3, key, index0=(1 << 31) - 2)
    for kw, text in ((dict(T="auto"), "fixed T"), (dict(T=0), "T in 1..64"), (dict(T=65), "T in 1..64"), (dict(tmax=0), "tmax"),
                     (dict(tmax=17), "tmax"), (dict(tmax=True), "tmax"), (dict(maxval=0), "maxval"),
                     (dict(maxval=65536), "maxval"), (dict(max_entries=-1), "max_entries"),
                     (dict(max_entries=65537), "max_entries"), (dict(max_entries=2.5), "max_entries")):
        with pytest.raises(ValueError, match=text):
            pkg.encode_blind_keyed(cover, [b"x"], key, **kw)
    with pytest.raises(ValueError, match="header bits"):
        pkg.encode_blind_keyed(np.zeros((8, 16), np.uint16), [b"x"], key)
    with pytest.raises(ValueError, match="65535"):
        pkg.encode_blind_keyed(np.zeros((2, 65536), np.uint8), [b"x"], key)
    with pytest.raises(ValueError, match="shape"):
        pkg.encode_blind_keyed(np.zeros(16, np.uint16), [b"x"], key)
    for bad in (None, b"short", "k" * 32):
        with pytest.raises(ValueError, match="key"):
            pkg.decode_blind_keyed(cover, bad)
        with pytest.raises(ValueError, match="key"):
            pipeline.decode_dicom_pee_keyed(b"not read", bad)
        with pytest.raises(ValueError, match="key"):
            pipeline.encode_dicom_pee_keyed(cover, b"x", "unused.dcm", bad)
    with pytest.raises(ValueError, match="nonce"):
        pipeline.encode_dicom_pee_keyed(cover, b"x", "unused.dcm", key, nonce=b"123")
    # the unkeyed calls: as before
    ok = dict(scheme=1, T=2, gate=None, H=64, W=96, maxval=4095)
    with pytest.raises(ValueError, match="takes no key="):
        blind.check_args(**ok, key=key)
    with pytest.raises(ValueError, match="takes no key="):
        blind.check_args_auto(scheme=1, tmax=8, gate=None, H=64, W=96, maxval=4095, key=key)
    with pytest.raises(ValueError, match="takes no key="):
        pkg.encode_blind(cover, [b"x"], key=key)
    assert {"encode_blind_keyed", "decode_blind_keyed"} <= set(pkg.__all__)


def test_loader_lists_the_keyed_entries():
    path = os.path.join(build.INC, "codec_tcc_blind_keyed.h")
    hdr = open(path).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_BLIND_KEYED) == {
        "codec_chacha20_rows_n", "codec_poly1305_tags_n", "codec_aead_release_n", "codec_pee_blind_frames",
        "codec_pee_blind_embed_keyed", "codec_pee_blind_unframe"}
    assert path in build._common_deps()
    # in the digest: it is the digest of exactly SRCS + _common_deps()
    assert build.source_digest() == build._digest(build.SRCS + build._common_deps(), build.FLAGS)
    assert f"#define CODEC_PEE_BLIND_FLAG_KEYED {_lib.BLIND_FLAG_KEYED}" in hdr
    assert f"#define CODEC_PEE_BLIND_FRAME_BITS {_lib.BLIND_FRAME_BITS}" in hdr
    assert f"#define CODEC_PEE_BLIND_FRAME_WORDS {_lib.BLIND_FRAME_WORDS}" in hdr and 32 * _lib.BLIND_FRAME_WORDS == 224
    for name in _lib.EXPORTS_BLIND_KEYED:   # the loader binds them: argument counts as declared
        m = re.search(rf"{name}\s*\(([^)]*)\)", hdr, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib._SIGS_BLIND_KEYED[name][1]), name
    # the headers beside it keep their entry sets
    for other, exports in (("codec_tcc_blind.h", _lib.EXPORTS_BLIND), ("codec_tcc_blind_auto.h", _lib.EXPORTS_BLIND_AUTO),
                           ("codec_tcc_aead.h", _lib.EXPORTS_AEAD)):
        text = open(os.path.join(build.INC, other)).read()
        assert set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", text, re.M)) == set(exports), other
