"""The keyed header extension of MED-PEE files (container.pee_aead_extension) on the
host: b"A1" + nonce + tag after whichever of C1 / T1 are present or directly after the fixed
fields, cut headers, and files without it unchanged.  No GPU."""
import inspect
import struct

import numpy as np
import pytest

from codec_tcc_amd import container, pipeline
from codec_tcc_amd.pee import PeeCodec, PeeVolume

NONCE, TAG = bytes(range(1, 9)), bytes(range(0x30, 0x40))


def _file(hdr: bytes, body: bytes) -> bytes:
    return container.MAGIC + struct.pack(">I", len(hdr)) + hdr + body


def _hdr1(blob=b"lmblob"):
    return container.create_pee_header("raw", 2, 6, 4, 2, 5, 3, 4095, 0, len(blob)), blob + bytes(48)


def _hdr2():
    passes = [(3, 4, 1, 2), (2, 1, 0, 0), (0, -1, 0, 1), (0, -1, 0, 0)]
    return container.create_pee2_header("raw", 2, 6, 4, 2, 4095, 5, 0, passes), b"aab" + bytes(48)


def _tiles():
    return container.pee_tile_extension(4, 4, np.arange(2, dtype=np.uint32).reshape(1, 2) + 7)   # 4 x 6 pixels at tile 4


def test_the_extension_is_26_bytes():
    ext = container.pee_aead_extension(NONCE, TAG)
    assert ext == b"A1" + NONCE + TAG and len(ext) == 26
    for nonce, tag in ((NONCE[:7], TAG), (NONCE, TAG[:15]), ("12345678", TAG), (NONCE, None)):
        with pytest.raises(ValueError):
            container.pee_aead_extension(nonce, tag)


@pytest.mark.parametrize("before", ["none", "c1", "c1t1"])
@pytest.mark.parametrize("scheme", [1, 2])
def test_round_trip_after_whichever_extensions_are_present(scheme, before):
    hdr, body = _hdr1() if scheme == 1 else _hdr2()
    parse = container.parse_pee_bytes if scheme == 1 else container.parse_pee2_bytes
    pre = {"none": b"", "c1": container.pee_crc_extension(5, 0),
           "c1t1": container.pee_crc_extension(5, 0) + _tiles()}[before]
    md0, side0, data0 = parse(_file(hdr + pre, body))
    assert "aead_tag" not in md0 and "aead_nonce" not in md0
    md, side, data = parse(_file(hdr + pre + container.pee_aead_extension(NONCE, TAG), body))
    assert md["aead_nonce"] == NONCE and md["aead_tag"] == TAG and (side, data) == (side0, data0)
    assert ("cover_crc32" in md) == (before != "none") and ("tile_crc32" in md) == (before == "c1t1")
    rest = {k: v for k, v in md.items() if not k.startswith("aead_")}
    assert rest.keys() == md0.keys() and all(np.array_equal(rest[k], md0[k]) for k in rest)


@pytest.mark.parametrize("before", ["none", "c1", "c1t1"])
@pytest.mark.parametrize("cut", [1, 2, 9, 10, 25])
def test_a_header_cut_inside_the_extension_is_refused_by_read_pee_bytes(before, cut):
    hdr, body = _hdr1()
    pre = {"none": b"", "c1": container.pee_crc_extension(5, 0),
           "c1t1": container.pee_crc_extension(5, 0) + _tiles()}[before]
    raw = _file(hdr + pre + container.pee_aead_extension(NONCE, TAG)[:cut], body)
    with pytest.raises(ValueError, match="truncated"):
        pipeline.read_pee_bytes(raw)
    with pytest.raises(ValueError, match="truncated"):
        container.parse_pee_bytes(raw)


def test_files_without_the_extension_are_what_they_were():
    hdr, body = _hdr1()
    assert len(hdr) == 36 and hdr == struct.pack(">BBBBIIiiiiiI", 16, 0, 2, 0, 6, 4, 2, 5, 3, 4095, 0, 6)
    md, _b, _d = container.parse_pee_bytes(_file(hdr, body))
    assert not any(k.startswith("aead_") for k in md)
    md, _b, _d = container.parse_pee_bytes(_file(hdr + container.pee_crc_extension(1, 2), body))
    assert md["payload_crc32"] == 2 and not any(k.startswith("aead_") for k in md)


def test_key_arguments_of_the_file_and_volume_calls():
    for fn in (pipeline.encode_file_pee, PeeCodec.embed_volume):
        sig = inspect.signature(fn).parameters
        assert sig["key"].default is None and sig["nonce"].default is None
    assert inspect.signature(pipeline.decode_bin_pee).parameters["key"].default is None
    assert inspect.signature(PeeCodec.decode_volume).parameters["key"].default is None
    assert "tag" in PeeVolume.__dataclass_fields__
    img = np.zeros((8, 8), dtype=np.uint16)
    with pytest.raises(ValueError):
        pipeline.encode_file_pee(img, b"x", "unused.bin", key=b"short")       # before the GPU is touched
    with pytest.raises(ValueError):
        pipeline.encode_file_pee(img, b"x", "unused.bin", key=bytes(32), nonce=b"123")
    with pytest.raises(ValueError):
        pipeline.encode_file_pee(img, b"x", "unused.bin", nonce=bytes(8))


def test_a_keyed_file_read_without_a_key_is_refused_before_the_gpu(tmp_path):
    blob = container.lm_blob(np.zeros(4, dtype=bool))                     # end = 3: four map bits
    hdr = container.create_pee_header("raw", 2, 6, 4, 2, 3, 3, 4095, 0, len(blob))
    for ext, key in ((container.pee_aead_extension(NONCE, TAG), None), (b"", bytes(32))):
        path = tmp_path / "f.bin"
        path.write_bytes(_file(hdr + ext, blob + bytes(48)))
        assert ("aead_tag" in pipeline.read_pee_bytes(path.read_bytes()).md) == (key is None)
        with pytest.raises(ValueError, match="key"):
            pipeline.decode_bin_pee(str(path), key=key)
