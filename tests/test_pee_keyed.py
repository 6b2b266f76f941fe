"""Keyed MED-PEE on the GPU (PeeCodec.embed(key=) / decode(key=)): the keyed embed is
the plain embed of the specification's ciphertext rows (tests/aead_spec.py) on every route, the
tag is the specification's, decode returns payload and cover exactly, and a wrong key, a wrong
nonce, a changed stego pixel or a changed tag bit raise IntegrityError for the slices concerned
with no plaintext of theirs on the host."""
import numpy as np
import pytest

import aead_spec as S
import pee_gate_spec as G
from codec_tcc_amd import IntegrityError, aead, framing, synth

pytestmark = pytest.mark.gpu

B, H, W, MAXVAL = 3, 64, 64, 4095
KEY = bytes(range(1, 33))
NONCE = bytes(range(0xA0, 0xA8))
INDEX0 = 5


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def covers():
    return np.stack([synth.ct12(H, W, 700 + i) for i in range(B)])


def _bits(n=(40, 24, 48)):   # a 64 x 64 slice holds about 70 bits at T = 2
    return [np.asarray(G.payload_bits(k, 31 + i), dtype=np.uint8) for i, k in enumerate(n)]


def _spec_rows(bits, key=KEY, nonce=NONCE, index0=INDEX0):
    """(plaintext rows, ciphertext rows by the specification, lengths) as lists of 64-bit ints"""
    rows, lengths = framing.pack_bits(bits)
    pt = [[int(v) for v in r] for r in rows.view(np.uint64)]
    return pt, [S.crypt_row(key, nonce, index0 + b, pt[b], lengths[b]) for b in range(len(bits))], lengths


def _packed(ct, lengths):
    torch = _torch()
    return (torch.from_numpy(np.array(ct, dtype=np.uint64).view(np.int64)).cuda(), list(lengths),
            torch.tensor(list(lengths), dtype=torch.int32, device="cuda"))


def _codec(route):
    from codec_tcc_amd.pee import PeeCodec
    kw = dict(dtype="uint16", maxval=MAXVAL)
    if route == "auto":
        return PeeCodec(B, H, W, T="auto", tmax=8, **kw)
    if route == "gate":
        return PeeCodec(B, H, W, T=3, gate="auto", **kw)
    if route == "scheme2":
        return PeeCodec(B, H, W, T=2, scheme=2, **kw)
    return PeeCodec(B, H, W, T=2, **kw)


@pytest.mark.parametrize("route", ["fixed", "auto", "gate", "roi", "scheme2", "inplace"])
def test_keyed_embed_is_the_plain_embed_of_the_spec_ciphertext(covers, route):
    torch = _torch()
    codec = _codec(route)
    bits = _bits((40, 100, 200)) if route in ("auto", "scheme2") else _bits()
    pt, ct, lengths = _spec_rows(bits)
    kw = {"roi": (9, 11, 31, 41)} if route == "roi" else {}
    cov = torch.from_numpy(covers).cuda()
    if route == "inplace":
        a, b = cov.clone(), cov.clone()
        keyed = codec.embed(a, bits, stego=a, key=KEY, nonce=NONCE, index0=INDEX0)
        plain = codec.embed(b, None, stego=b, packed=_packed(ct, lengths))
    else:
        keyed = codec.embed(cov, bits, key=KEY, nonce=NONCE, index0=INDEX0, **kw)
        plain = codec.embed(cov, None, packed=_packed(ct, lengths), **kw)
    assert torch.equal(keyed.stego, plain.stego) and not torch.equal(keyed.stego, cov)
    assert torch.equal(keyed.meta, plain.meta)
    assert keyed.lengths == plain.lengths == lengths and keyed.payload_crc is None
    assert (keyed.nonce, keyed.index0) == (NONCE, INDEX0) and plain.tag is None
    # the tag is of the COVER (also in place) and the ciphertext
    want = [S.tag(KEY, NONCE, INDEX0 + b, covers[b].tobytes(), ct[b], lengths[b]) for b in range(B)]
    assert aead.tag_bytes(keyed.tag) == want
    got_bits, restored = codec.decode(keyed, key=KEY)
    assert torch.equal(restored, cov)
    for b in range(B):
        np.testing.assert_array_equal(got_bits[b], bits[b])
    # verify=False decrypts without the tag pass
    got2, _ = codec.decode(keyed, verify=False, key=KEY)
    for b in range(B):
        np.testing.assert_array_equal(got2[b], bits[b])


def test_packed_rows_of_the_caller_are_not_modified_and_checksums_compose(covers):
    torch = _torch()
    codec = _codec("fixed")
    bits = _bits()
    pt, ct, lengths = _spec_rows(bits)
    packed = _packed(pt, lengths)
    before = packed[0].clone()
    cov = torch.from_numpy(covers).cuda()
    enc = codec.embed(cov, None, packed=packed, key=KEY, nonce=NONCE, index0=INDEX0, checksum="tiles", tile=16)
    assert torch.equal(packed[0], before)
    assert enc.cover_crc is not None and enc.cover_tile_crc is not None and enc.payload_crc is None
    got, restored = codec.decode(enc, verify="require", key=KEY)
    assert torch.equal(restored, cov)
    np.testing.assert_array_equal(got[2], bits[2])
    # a changed pixel: the keyed failure names the slice and, with a tile table, the tile
    enc.stego.view(torch.int16)[1, 40, 40] ^= 1
    with pytest.raises(IntegrityError) as e:
        codec.decode(enc, key=KEY)
    assert e.value.keyed and e.value.slices == [1] and set(e.value.tiles) == {1} and e.value.tiles[1][2, 2]


def _fails(codec, enc, key, slices):
    with pytest.raises(IntegrityError) as e:
        codec.decode(enc, key=key)
    assert e.value.keyed is True and e.value.slices == slices
    rows = e.value.rows                              # what the one read-back brought
    for b in range(B):
        assert (not rows[b].any()) == (b in slices), b


def test_decode_refuses_what_was_not_embedded(covers):
    import copy
    torch = _torch()
    codec = _codec("fixed")
    bits = _bits((40, 33, 48))
    cov = torch.from_numpy(covers).cuda()
    enc = codec.embed(cov, bits, key=KEY, nonce=NONCE, index0=INDEX0)
    _fails(codec, enc, bytes(32), [0, 1, 2])                                  # a wrong key
    other = copy.copy(enc)
    other.nonce = bytes(8)
    _fails(codec, other, KEY, [0, 1, 2])                                      # a wrong nonce
    other = copy.copy(enc)
    other.index0 = INDEX0 + 1
    _fails(codec, other, KEY, [0, 1, 2])                                      # another slice's nonce
    other = copy.copy(enc)
    other.stego = enc.stego.clone()
    other.stego.view(torch.int16)[1, 17, 23] ^= 1                                               # one stego pixel
    _fails(codec, other, KEY, [1])
    other = copy.copy(enc)
    other.tag = enc.tag.clone()
    other.tag[2, 1] ^= 1 << 9                                                 # one tag bit
    _fails(codec, other, KEY, [2])
    got, restored = codec.decode(enc, key=KEY)                                # the original still decodes
    assert torch.equal(restored, cov) and all(np.array_equal(got[b], bits[b]) for b in range(B))
    # the release itself: the failing slice's row is zero on the device
    words, cover = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    lens = torch.tensor(enc.lengths, dtype=torch.int32, device="cuda")
    ctx = aead.upload_ctx(KEY, NONCE)
    tags = aead.poly1305_tags(ctx, cover, words, lens, INDEX0)
    assert torch.equal(tags, enc.tag)
    bad = enc.tag.clone()
    bad[0, 3] ^= 1
    pt, ok = aead.release(ctx, tags, bad, words, lens, INDEX0)
    assert ok.tolist() == [0, 1, 1] and not pt[0].any().item() and pt[1].any().item()


def test_key_arguments_are_judged_before_any_launch(covers):
    torch = _torch()
    codec = _codec("fixed")
    cov = torch.from_numpy(covers).cuda()
    bits = _bits()
    for kw in (dict(key=b"short"), dict(key=KEY, nonce=b"1234567"), dict(key=KEY, index0=-1),
               dict(key=KEY, index0=(1 << 31) - 2), dict(nonce=NONCE), dict(index0=3), dict(key="k" * 32)):
        with pytest.raises(ValueError):
            codec.embed(cov, bits, **kw)
    enc = codec.embed(cov, bits, key=KEY)             # a fresh nonce
    assert len(enc.nonce) == 8 and enc.index0 == 0
    assert codec.embed(cov, bits, key=KEY).nonce != enc.nonce
    with pytest.raises(ValueError):
        codec.decode(enc)                              # keyed, no key
    plain = codec.embed(cov, bits)
    assert plain.tag is None and plain.nonce is None
    with pytest.raises(ValueError):
        codec.decode(plain, key=KEY)                   # a key for an unkeyed embedding


def test_package_level_encode_and_decode_take_the_key(covers):
    import codec_tcc_amd as ct
    torch = _torch()
    cov = torch.from_numpy(covers).cuda()
    enc = ct.encode(cov, ["pat 1", "p2", "the third"], method="pee", T="auto", maxval=MAXVAL, key=KEY)
    bits, restored = ct.decode(enc, key=KEY)
    assert torch.equal(restored, cov)
    np.testing.assert_array_equal(bits[2], framing.to_bits("the third"))
    with pytest.raises(IntegrityError):
        ct.decode(enc, key=bytes(32))
    with pytest.raises(ValueError):
        ct.encode(cov, ["a", "b", "c"], key=KEY)      # the LSB path has no key


def test_graph_replay_under_a_rewritten_context(covers):
    """The keyed embed's launches (encrypt, tag, embed) captured once; the context block is
    rewritten between the replays, so each runs under its own nonce."""
    from codec_tcc_amd.pee import PeeEncoded
    torch = _torch()
    codec = _codec("fixed")
    bits = _bits()
    pt, _ct, lengths = _spec_rows(bits)
    words, lengths, lens_t = _packed(pt, lengths)
    cov = torch.from_numpy(covers).cuda()
    nonces = [bytes([i] * 8) for i in (1, 2)]
    ctx = aead.upload_ctx(KEY, bytes(8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture
        ct_rows = aead.chacha20_rows(ctx, words, lens_t, INDEX0)
        tag = aead.poly1305_tags(ctx, cov, ct_rows, lens_t, INDEX0)
        enc = codec.embed(cov, None, packed=(ct_rows, lengths, lens_t), check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ct_rows = aead.chacha20_rows(ctx, words, lens_t, INDEX0)
        tag = aead.poly1305_tags(ctx, cov, ct_rows, lens_t, INDEX0)
        enc = codec.embed(cov, None, packed=(ct_rows, lengths, lens_t), check=False)
    stegos = []
    for n in nonces:
        aead.write_ctx(ctx, KEY, n)
        g.replay()
        torch.cuda.synchronize()
        stegos.append(enc.stego.clone())
        want = [S.tag(KEY, n, INDEX0 + b, covers[b].tobytes(), S.crypt_row(KEY, n, INDEX0 + b, pt[b], lengths[b]),
                      lengths[b]) for b in range(B)]
        assert aead.tag_bytes(tag) == want
        snap = PeeEncoded(stego=enc.stego.clone(), lm=enc.lm.clone(), meta=enc.meta.clone(), lengths=list(lengths),
                          payload_words=enc.payload_words, config=enc.config, tag=tag.clone(), nonce=n, index0=INDEX0)
        got, restored = codec.decode(snap, key=KEY)
        assert torch.equal(restored, cov) and all(np.array_equal(got[b], bits[b]) for b in range(B))
    assert not torch.equal(stegos[0], stegos[1])
