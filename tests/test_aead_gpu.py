"""The keyed-MED-PEE kernels (include/codec_tcc_aead.h, codec_tcc_amd/aead.py) on the GPU, bit for
bit against tests/aead_spec.py and the openssl-made tests/golden/aead_kat.json."""
import json
import os

import numpy as np
import pytest

import aead_spec as S
from codec_tcc_amd import aead

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
P = S.P1305
KAT_LENGTHS = [0, 1, 7, 8, 63, 64, 65, 511, 512, 513]


def _torch():
    import torch
    return torch


def _kat():
    with open(os.path.join(HERE, "golden", "aead_kat.json")) as f:
        return json.load(f)["cases"]


def _rows(rows):
    """list of rows of 64-bit ints -> int64 [B, row_words] on the GPU"""
    return _torch().from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).cuda()


def _words(t):
    return [[int(v) for v in r] for r in t.cpu().numpy().view(np.uint64)]


def _lens(ls):
    return _torch().tensor(ls, dtype=_torch().int32, device="cuda")


def _bytes_t(data: bytes, offset: int = 0):
    """uint8 GPU tensor of `data` whose first byte lies `offset` bytes past an allocation's start"""
    torch = _torch()
    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[offset:offset + len(data)]


def _otk_t(otks):
    return _torch().from_numpy(np.frombuffer(b"".join(otks), dtype="<i4").reshape(len(otks), 8).copy()).cuda()


def _rand_bytes(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _rand_rows(rng, B, rw):
    return [[int(v) for v in rng.integers(0, 1 << 64, size=rw, dtype=np.uint64)] for _ in range(B)]


# ------------------------------------------------------------------ known answers
def test_rfc8439_2_8_2_through_the_entries():
    key, nonce, aad = bytes(range(0x80, 0xA0)), bytes(range(0x40, 0x48)), bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    text = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
            b"sunscreen would be it.")
    ctx = aead.upload_ctx(key, nonce)
    L = _lens([8 * len(text)])
    ct = aead.chacha20_rows(ctx, _rows([S.bytes_row(text, 15)]), L, index0=7)
    assert S.row_bytes(_words(ct)[0], 8 * len(text))[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    tags = aead.poly1305_tags(ctx, _bytes_t(aad).reshape(1, 12), ct, L, index0=7)
    assert aead.tag_bytes(tags) == [bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")]
    pt, ok = aead.release(ctx, tags, tags.clone(), ct, L, index0=7)
    assert ok.tolist() == [1] and S.row_bytes(_words(pt)[0], 8 * len(text)) == text


def test_openssl_kat_through_the_entries():
    bad = []
    for c in _kat():
        key, nonce, aad = bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"]), bytes.fromhex(c["aad"])
        ctx = aead.upload_ctx(key, nonce)
        rw, L = c["row_words"], _lens([c["L"]])
        ct = aead.chacha20_rows(ctx, _rows([S.bytes_row(bytes.fromhex(c["pt_row"]), rw)]), L, index0=c["index"])
        got_ct = b"".join(w.to_bytes(8, "little") for w in _words(ct)[0]).hex()
        aad_t = _bytes_t(aad, 3).reshape(1, -1) if aad else None
        tag = aead.tag_bytes(aead.poly1305_tags(ctx, aad_t, ct, L, index0=c["index"]))[0].hex()
        if got_ct != c["ct_row"] or tag != c["tag"]:
            bad.append((c["name"], got_ct == c["ct_row"], tag, c["tag"]))
    assert not bad, bad


# ------------------------------------------------------------------ Poly1305 with chosen keys
def _check_otk(otks, aads, rows=None, lengths=None, offset=0):
    """tags of B slices under given one-time keys against the specification"""
    B, n = len(otks), len(aads[0])
    aad_t = _bytes_t(b"".join(aads), offset).reshape(B, n) if n else None
    rt = _rows(rows) if rows is not None else None
    lt = _lens(lengths) if rows is not None else None
    got = aead.tag_bytes(aead.poly1305_tags_otk(_otk_t(otks), aad_t, rt, lt))
    want = [S.tag_otk(otks[b], aads[b], rows[b] if rows is not None else [], lengths[b] if rows is not None else 0)
            for b in range(B)]
    assert [g.hex() for g in got] == [w.hex() for w in want]
    return want


def test_extreme_one_time_keys():
    rng = np.random.default_rng(5)
    n = 16 * 300 + 5                                # more blocks than lanes, and a partial one
    ff = b"\xFF" * n
    keys = [b"\xFF" * 16 + _rand_bytes(rng, 16),    # r at its clamped maximum, all-0xFF data: largest limbs and carries
            bytes(16) + _rand_bytes(rng, 16),       # r = 0: the tag is s
            _rand_bytes(rng, 16) + b"\xFF" * 16,    # s = 2^128 - 1
            b"\xFF" * 32]
    want = _check_otk(keys, [ff] * 4, [[(1 << 64) - 1] * 9] * 4, [64 * 9, 64 * 9, 513, 1])
    assert want[1] == keys[1][16:]


def test_accumulator_between_p_and_2_130():
    """r = 1: the sum is the plain integer sum of the blocks.  Two AAD blocks and the lengths
    block (value 32) give 3 * 2^128 + m0 + m1 + 32; m0 is chosen so that this is p + k, k = 0 .. 4,
    i.e. in [p, 2^130) when the final reduction starts; also p - 1 and 2^130 (= p + 5)."""
    r1 = (1).to_bytes(16, "little")
    otks, aads = [], []
    for k in (-1, 0, 1, 2, 3, 4, 5):
        m0 = (1 << 128) - 5 + k - 32
        m1 = 0
        if m0 >= 1 << 128:
            m0, m1 = (1 << 128) - 1, m0 - ((1 << 128) - 1)
        for s in (bytes(16), b"\xFF" * 16):
            otks.append(r1 + s)
            aads.append(m0.to_bytes(16, "little") + m1.to_bytes(16, "little"))
            want_h = (3 * (1 << 128) + m0 + m1 + 32) % P
            assert S.poly1305_pre_final(otks[-1], S.mac_data(aads[-1], b"")) == want_h == (k if k >= 0 else P - 1)
    _check_otk(otks, aads)


# ------------------------------------------------------------------ Poly1305 sizes and alignments
def _sizes():
    C = aead.chunk_bytes()
    return [0, 1, 15, 16, 17, C - 16, C, C + 1, 3 * C + 17]


@pytest.mark.parametrize("k", range(9))
def test_aad_sizes_aligned_and_not(k):
    n = _sizes()[k]
    rng = np.random.default_rng(100 + k)
    rw = 9
    for offset in (0, 1) if n else (0,):
        otks = [_rand_bytes(rng, 32) for _ in range(2)]
        aads = [_rand_bytes(rng, n) for _ in range(2)]
        L = [KAT_LENGTHS[(k + offset) % 10], KAT_LENGTHS[(k + 5 + offset) % 10]]
        _check_otk(otks, aads, _rand_rows(rng, 2, rw), L, offset)


def test_odd_slices_of_37_by_53_bytes_and_ct_lengths():
    rng = np.random.default_rng(7)
    torch = _torch()
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    ctx = aead.upload_ctx(key, nonce)
    img = rng.integers(0, 256, size=(3, 37, 53), dtype=np.uint8)
    cover = torch.from_numpy(img).cuda()
    rw = 9
    for lens in ([0, 1, 7], [8, 63, 64], [65, 511, 512], [513, 64 * rw, 64 * rw - 1]):
        rows = _rand_rows(rng, 3, rw)
        got = aead.tag_bytes(aead.poly1305_tags(ctx, cover, _rows(rows), _lens(lens), index0=11))
        want = [S.tag(key, nonce, 11 + b, img[b].tobytes(), rows[b], lens[b]) for b in range(3)]
        assert got == want, lens
    # covers alone (an empty CT), and rows alone (an empty AAD)
    assert aead.tag_bytes(aead.poly1305_tags(ctx, cover, index0=2)) == \
        [S.tag(key, nonce, 2 + b, img[b].tobytes(), [], 0) for b in range(3)]
    rows = _rand_rows(rng, 3, rw)
    assert aead.tag_bytes(aead.poly1305_tags(ctx, None, _rows(rows), _lens([100, 0, 576]))) == \
        [S.tag(key, nonce, b, b"", rows[b], L) for b, L in enumerate([100, 0, 576])]


def test_a_long_ct_row_is_absorbed_in_parallel():
    """128 KB of CT: 8192 blocks over the finishing workgroup's lanes, then the lengths block"""
    rng = np.random.default_rng(8)
    rw = 16384 + 1
    rows = _rand_rows(rng, 2, rw)
    otks = [_rand_bytes(rng, 32) for _ in range(2)]
    _check_otk(otks, [_rand_bytes(rng, 40)] * 2, rows, [64 * rw, 64 * rw - 77])


# ------------------------------------------------------------------ ChaCha20
def _check_chacha(key, nonce, index0, rows, lens, in_place=False):
    ctx = aead.upload_ctx(key, nonce)
    t, lt = _rows(rows), _lens(lens)
    out = aead.chacha20_rows(ctx, t, lt, index0=index0, out=t if in_place else None)
    want = [S.crypt_row(key, nonce, index0 + b, rows[b], lens[b]) for b in range(len(rows))]
    assert _words(out) == want
    if not in_place:
        assert _words(t) == rows                          # the input is not modified
    back = aead.chacha20_rows(ctx, out, lt, index0=index0)   # an involution on the first L bits
    assert _words(back) == [S.bytes_row(S.row_bytes(rows[b], lens[b]), len(rows[b])) for b in range(len(rows))]
    return out


@pytest.mark.parametrize("in_place", [False, True])
def test_chacha_lengths_around_block_and_word_edges(in_place):
    rng = np.random.default_rng(20)
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    lens = [0, 1, 63, 64, 65, 127, 128, 511, 512, 513, 575, 576, 577, 1023, 1024, 3 * 512 + 1, 25 * 64, 25 * 64 - 1]
    rw = 25                                               # 3 blocks and a word: rows at odd 8-byte bases
    _check_chacha(key, nonce, 40, _rand_rows(rng, len(lens), rw), lens, in_place)


def test_chacha_lengths_out_of_range_count_as_the_bounds():
    rng = np.random.default_rng(21)
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    rows = _rand_rows(rng, 2, 3)
    ctx = aead.upload_ctx(key, nonce)
    out = aead.chacha20_rows(ctx, _rows(rows), _lens([-5, 1000]))
    assert _words(out) == [S.crypt_row(key, nonce, 0, rows[0], 0), S.crypt_row(key, nonce, 1, rows[1], 192)]


def test_chacha_one_long_row_and_the_stream_index():
    rng = np.random.default_rng(22)
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    L = (1 << 20) + 3
    rw = (L + 63) // 64 + 2
    _check_chacha(key, nonce, S.STREAM_INDEX, _rand_rows(rng, 1, rw), [L])


def test_chacha_many_short_rows():
    rng = np.random.default_rng(23)
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    B, rw = 300, 5
    _check_chacha(key, nonce, (1 << 31) - B, _rand_rows(rng, B, rw), [int(v) for v in rng.integers(0, 64 * rw + 1, size=B)])


# ------------------------------------------------------------------ release
def test_release_zeroes_exactly_the_slices_whose_tags_differ():
    rng = np.random.default_rng(30)
    torch = _torch()
    key, nonce = _rand_bytes(rng, 32), _rand_bytes(rng, 8)
    ctx = aead.upload_ctx(key, nonce)
    B, rw = 5, 9
    rows, lens = _rand_rows(rng, B, rw), [513, 64, 0, 576, 100]
    ct = _rows(rows)
    got = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(B, 4), dtype=np.int64).astype(np.int32)).cuda()
    want = got.clone()
    want[1, 3] ^= -2 ** 31          # the tag's last bit
    want[3, 0] ^= 1                 # its first
    pt, ok = aead.release(ctx, got, want, ct, _lens(lens), index0=9)
    assert ok.tolist() == [1, 0, 1, 0, 1]
    exp = [S.crypt_row(key, nonce, 9 + b, rows[b], lens[b]) if b not in (1, 3) else [0] * rw for b in range(B)]
    assert _words(pt) == exp
    pt2, ok2 = aead.release(ctx, got, want, ct, _lens(lens), index0=9, out=ct)   # in place
    assert pt2.data_ptr() == ct.data_ptr() and _words(ct) == exp and ok2.tolist() == [1, 0, 1, 0, 1]


def test_bad_arguments_raise_before_anything_is_queued():
    torch = _torch()
    ctx = aead.upload_ctx(bytes(32), bytes(8))
    rows, lens = _rows([[1, 2]]), _lens([3])
    with pytest.raises(ValueError):
        aead.chacha20_rows(ctx, rows, lens, index0=1 << 31 | 1)
    with pytest.raises(ValueError):
        aead.chacha20_rows(ctx, rows, lens, index0=-1)
    with pytest.raises(ValueError):
        aead.chacha20_rows(ctx, _rows([[1], [2]]), _lens([1, 1]), index0=S.STREAM_INDEX)   # the stream is one row
    with pytest.raises(ValueError):
        aead.chacha20_rows(ctx, rows.to(torch.int32), lens)
    with pytest.raises(ValueError):
        aead.chacha20_rows(ctx[:40], rows, lens)
    with pytest.raises(ValueError):
        aead.poly1305_tags(ctx, None)
    with pytest.raises(ValueError):
        aead.upload_ctx(bytes(31), bytes(8))
    with pytest.raises(ValueError):
        aead.upload_ctx(bytes(32), "12345678")
