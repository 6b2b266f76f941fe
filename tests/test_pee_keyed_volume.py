"""Keyed volume payloads and keyed files on the GPU (PeeCodec.embed_volume(key=) /
decode_volume(key=), pipeline.encode_file_pee(key=) / decode_bin_pee(key=)), against
tests/aead_spec.py: the stream is one row at the reserved index with an empty AAD, tagged over the
embedded total; every cover has a tag with an empty ciphertext; a file's header carries nonce and
tag."""
import struct

import numpy as np
import pytest

import aead_spec as S
import pee_gate_spec as G
from codec_tcc_amd import IntegrityError, aead, framing, pipeline, synth

pytestmark = pytest.mark.gpu

B, H, W, MAXVAL, TMAX = 4, 64, 64, 4095, 8
KEY = bytes(range(2, 34))
NONCE = bytes(range(0xB0, 0xB8))
INDEX0 = 9


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def covers():
    return np.stack([synth.ct12(H, W, 800 + i) for i in range(B)])


def _codec():
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, H, W, T="auto", tmax=TMAX, maxval=MAXVAL)


def _stream(n, seed=3):
    bits = np.asarray(G.payload_bits(n, seed), dtype=np.uint8)
    words = [int(v) for v in framing.pack_bits([bits])[0].reshape(-1).view(np.uint64)]
    return bits, words, S.crypt_row(KEY, NONCE, S.STREAM_INDEX, words, n)


def _check_volume(codec, covers, n, policy):
    torch = _torch()
    cov = torch.from_numpy(covers).cuda()
    bits, words, ct = _stream(n)
    vol = codec.embed_volume(cov, bits, policy=policy, key=KEY, nonce=NONCE, index0=INDEX0)
    total = vol.embedded_bits
    # the stego is the plain volume embed of the specification's ciphertext stream
    packed = (torch.from_numpy(np.array(ct, dtype=np.uint64).view(np.int64)).cuda(), n)
    plain = codec.embed_volume(cov, None, policy=policy, packed=packed)
    assert torch.equal(vol.enc.stego, plain.enc.stego) and torch.equal(vol.enc.meta, plain.enc.meta)
    assert plain.tag is None and plain.enc.tag is None and vol.payload_crc is None
    assert aead.tag_bytes(vol.tag) == [S.tag(KEY, NONCE, S.STREAM_INDEX, b"", ct, total)]
    assert aead.tag_bytes(vol.enc.tag) == [S.tag(KEY, NONCE, INDEX0 + b, covers[b].tobytes(), [], 0) for b in range(B)]
    assert (vol.enc.nonce, vol.enc.index0) == (NONCE, INDEX0)
    got, restored = codec.decode_volume(vol, key=KEY)
    assert torch.equal(restored, cov)
    np.testing.assert_array_equal(got, bits[:total])
    got2, _ = codec.decode_volume(vol, verify=False, key=KEY)
    np.testing.assert_array_equal(got2, bits[:total])
    return vol, cov, bits


@pytest.mark.parametrize("policy", ["even", "fill"])
def test_keyed_volume_round_trip(covers, policy):
    vol, _cov, bits = _check_volume(_codec(), covers, 600, policy)
    assert vol.embedded_bits == 600


def test_a_truncated_keyed_volume_authenticates_its_prefix(covers):
    vol, _cov, _bits = _check_volume(_codec(), covers, 5000, "even")
    assert 0 < vol.embedded_bits < 5000 and vol.plan_host()["status"] == 1


def test_keyed_volume_refuses_what_was_not_embedded(covers):
    import copy
    import dataclasses
    torch = _torch()
    codec = _codec()
    vol, cov, bits = _check_volume(codec, covers, 600, "even")
    with pytest.raises(IntegrityError) as e:
        codec.decode_volume(vol, key=bytes(32))                                # a wrong key
    assert e.value.keyed and e.value.stream and e.value.slices == [0, 1, 2, 3] and not e.value.rows.any()
    other = dataclasses.replace(vol, tag=vol.tag.clone())
    other.tag[0, 2] ^= 1 << 30                                                 # one bit of the stream's tag
    with pytest.raises(IntegrityError) as e:
        codec.decode_volume(other, key=KEY)
    assert e.value.keyed and e.value.stream and e.value.slices == [] and not e.value.rows.any()
    enc = copy.copy(vol.enc)
    enc.stego = vol.enc.stego.clone()
    enc.stego.view(torch.int16)[2, 40, 40] ^= 1                                # one pixel of slice 2 (a context pixel)
    with pytest.raises(IntegrityError) as e:
        codec.decode_volume(dataclasses.replace(vol, enc=enc), key=KEY)
    assert e.value.keyed and e.value.slices == [2]
    enc = copy.copy(vol.enc)
    enc.tag = vol.enc.tag.clone()
    enc.tag[1, 0] ^= 2                                                         # one bit of a cover's tag
    with pytest.raises(IntegrityError) as e:
        codec.decode_volume(dataclasses.replace(vol, enc=enc), key=KEY)
    assert e.value.keyed and e.value.slices == [1] and not e.value.stream
    with pytest.raises(ValueError):
        codec.decode_volume(vol)                                               # keyed, no key
    plain = codec.embed_volume(cov, bits)
    with pytest.raises(ValueError):
        codec.decode_volume(plain, key=KEY)                                    # a key for an unkeyed volume
    for kw in (dict(key=b"short"), dict(key=KEY, nonce=b"123"), dict(key=KEY, index0=(1 << 31) - 3), dict(nonce=NONCE)):
        with pytest.raises(ValueError):
            codec.embed_volume(cov, bits, **kw)


def test_package_level_volume_calls_take_the_key(covers):
    import codec_tcc_amd as ct
    torch = _torch()
    cov = torch.from_numpy(covers).cuda()
    vol = ct.encode_volume(cov, b"one record for the whole study", tmax=TMAX, maxval=MAXVAL, key=KEY)
    bits, restored = ct.decode_volume(vol, key=KEY)
    assert torch.equal(restored, cov)
    np.testing.assert_array_equal(bits, framing.to_bits(b"one record for the whole study"))
    with pytest.raises(IntegrityError):
        ct.decode_volume(vol, key=bytes(32))


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("kw", [dict(T="auto"), dict(T="auto", checksum="tiles", tile=16), dict(T=2, scheme=2)])
def test_a_keyed_file_decodes_and_a_changed_body_byte_raises(tmp_path, kw):
    img = synth.ct12(H, W, 900)
    payload = b"patient 0007"
    path = str(tmp_path / "keyed.bin")
    info = pipeline.encode_file_pee(img, payload, path, maxval=MAXVAL, key=KEY, nonce=NONCE, **kw)
    assert info["status"] == 0 and info["nonce"] == NONCE
    raw = open(path, "rb").read()
    md = pipeline.read_pee_bytes(raw).md
    bits = framing.to_bits(payload)
    row = [int(v) for v in framing.pack_bits([bits])[0].view(np.uint64)[0]]
    ct_row = S.crypt_row(KEY, NONCE, 0, row, bits.size)
    assert md["aead_nonce"] == NONCE and md["aead_tag"] == info["tag"] == S.tag(KEY, NONCE, 0, img.tobytes(), ct_row, bits.size)
    assert ("cover_crc32" in md) == ("checksum" in kw)
    got, cover = pipeline.decode_bin_pee(path, key=KEY)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(cover, img)
    got2, _ = pipeline.decode_bin_pee(path, verify=False, key=KEY)
    np.testing.assert_array_equal(got2, bits)
    with pytest.raises(ValueError, match="key"):
        pipeline.decode_bin_pee(path)
    with pytest.raises(IntegrityError) as e:
        pipeline.decode_bin_pee(path, key=bytes(32))
    assert e.value.keyed and e.value.slices == [0]
    (hlen,) = struct.unpack(">I", raw[4:8])
    bad = bytearray(raw)
    bad[-1] ^= 1                                                               # the last body byte: the raw stego's last pixel
    bad_path = str(tmp_path / "bad.bin")
    open(bad_path, "wb").write(bytes(bad))
    with pytest.raises(IntegrityError) as e:
        pipeline.decode_bin_pee(bad_path, key=KEY)
    assert e.value.keyed
    # the same call without key= writes the file it always wrote, and that file takes no key
    plain_path = str(tmp_path / "plain.bin")
    pipeline.encode_file_pee(img, payload, plain_path, maxval=MAXVAL, **kw)
    plain = open(plain_path, "rb").read()
    assert struct.unpack(">I", plain[4:8])[0] == hlen - 26 and b"A1" + NONCE not in plain[:8 + hlen]
    assert "aead_tag" not in pipeline.read_pee_bytes(plain).md
    with pytest.raises(ValueError, match="key"):
        pipeline.decode_bin_pee(plain_path, key=KEY)
