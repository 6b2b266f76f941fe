"""Host side of keyed MED-PEE (codec_tcc_amd/aead.py): key / nonce / index judgement,
the context block, and what the public types gained.  No GPU."""
import inspect
import os

import pytest

import aead_spec as S
from codec_tcc_amd import IntegrityError, _lib, aead, build
from codec_tcc_amd.pee import PeeCodec, PeeEncoded

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_and_nonce_are_bytes_of_32_and_8():
    key, nonce = bytes(range(32)), bytes(range(8))
    assert aead.check_key(key) == key and aead.check_key(bytearray(key)) == key
    assert aead.check_nonce(nonce) == nonce
    for bad in (None, "k" * 32, key[:31], key + b"\0", 7, list(key)):
        with pytest.raises(ValueError):
            aead.check_key(bad)
    for bad in (None, "n" * 8, nonce[:7], nonce + b"\0", 0):
        with pytest.raises(ValueError):
            aead.check_nonce(bad)
    assert len(aead.fresh_nonce()) == 8 and aead.fresh_nonce() != aead.fresh_nonce()


def test_slice_indices_stay_below_2_31_and_the_stream_index_is_one_row():
    assert aead.check_index(0, 256) == 0
    assert aead.check_index((1 << 31) - 256, 256) == (1 << 31) - 256
    assert aead.check_index(aead.STREAM_INDEX, 1) == S.STREAM_INDEX == _lib.AEAD_STREAM_INDEX == 0x80000000
    for index0, B in ((-1, 1), ((1 << 31) - 255, 256), (1 << 31, 2), ((1 << 31) + 1, 1), (1 << 32, 1), (0.5, 1), (True, 1)):
        with pytest.raises(ValueError):
            aead.check_index(index0, B)


def test_the_context_block_is_48_bytes_key_nonce_zero():
    key, nonce = bytes(range(100, 132)), bytes(range(8))
    raw = aead.ctx_bytes(key, nonce)
    assert len(raw) == 48 == _lib.AEAD_CTX_BYTES and raw == key + nonce + bytes(8)
    ctx = _lib.AeadCtx.from_buffer_copy(raw)
    assert list(ctx.key) == [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]
    assert list(ctx.nonce) == [0x03020100, 0x07060504] and list(ctx.reserved) == [0, 0]
    with pytest.raises(ValueError):
        aead.ctx_bytes(key, nonce[:4])


def test_the_unit_is_in_the_build_and_the_registry():
    assert os.path.join(build.HERE, "csrc", "codec_aead.hip") in build.SRCS
    assert os.path.join(build.INC, "codec_tcc_aead.h") in build._common_deps()
    assert {47: "k_chacha20_rows", 48: "k_poly1305_prep", 49: "k_poly1305", 50: "k_poly1305_finish",
            51: "k_aead_release"}.items() <= _lib.KERNEL_TAGS.items()
    assert set(_lib.EXPORTS_AEAD) == {"codec_poly1305_chunk_bytes", "codec_aead_workspace_bytes", "codec_chacha20_rows",
                                      "codec_poly1305_tags", "codec_poly1305_tags_otk", "codec_aead_release"}
    hdr = open(os.path.join(REPO, "include", "codec_tcc_aead.h")).read()
    assert "reuses the nonce" in hdr and "tests/aead_spec.py" in hdr


def test_public_types_and_signatures():
    e = IntegrityError("x", slices=[2, 0], keyed=True)
    assert e.keyed is True and e.slices == [2, 0] and e.bad_cover == [] and isinstance(e, ValueError)
    plain = IntegrityError("y", bad_cover=[1])
    assert plain.keyed is False and plain.slices == []
    enc = PeeEncoded(stego=None, lm=None, meta=None, lengths=[1], payload_words=1)
    assert enc.tag is None and enc.nonce is None and enc.index0 == 0
    sig = inspect.signature(PeeCodec.embed).parameters
    assert sig["key"].default is None and sig["nonce"].default is None and sig["index0"].default == 0
    assert inspect.signature(PeeCodec.decode).parameters["key"].default is None
    import codec_tcc_amd as ct
    assert inspect.signature(ct.encode).parameters["key"].default is None
    assert inspect.signature(ct.decode).parameters["key"].default is None
    with pytest.raises(ValueError):
        ct.encode(None, ["a"], key=bytes(32))            # the LSB path has no key: refused before the GPU
    with pytest.raises(ValueError):
        ct.encode(None, ["a"], method="pee", key=b"short")
