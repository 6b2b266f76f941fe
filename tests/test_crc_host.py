"""Host side of the checksummed MED-PEE: the library's GF(2) combine against zlib, the payload
checksum, and the 10-byte header extension of the version-16 container (no GPU)."""
import struct
import zlib

import numpy as np
import pytest

from codec_tcc_amd import _lib, checksum, container


def test_crc_entries_are_bound_apart_from_the_fixed_lists():
    assert set(_lib.EXPORTS_CRC) == {"codec_crc32_chunk_bytes", "codec_crc32_workspace_bytes", "codec_crc32_slices",
                                     "codec_crc32_combine"}
    assert not set(_lib.EXPORTS_CRC) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_EXT))
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.EXPORTS_CRC)


def test_build_lists_cover_the_new_source_and_header():
    import os
    from codec_tcc_amd import build
    assert os.path.join(build.HERE, "csrc", "codec_crc.hip") in build.SRCS
    assert os.path.join(build.INC, "codec_tcc_crc.h") in build._common_deps()


def test_combine_known_answers():
    a, b = zlib.crc32(b"1234"), zlib.crc32(b"56789")
    assert (a, b) == (0x9BE3E0A3, 0x131DA070)
    assert checksum.crc32_combine(a, b, 5) == 0xCBF43926 == zlib.crc32(b"123456789")


@pytest.mark.parametrize("split", [0, 1, 2, 7, 4096, 99999, 100000])
def test_combine_matches_zlib_on_split_buffers(split):
    """Lengths 0 and 1 on either side included (split = 0, 1, n - 1, n)."""
    data = np.random.default_rng(7).integers(0, 256, 100000, dtype=np.uint8).tobytes()
    a, b = data[:split], data[split:]
    assert checksum.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)


def test_combine_with_len_b_past_2_to_32():
    """B = 256 copies of a 16 MiB piece and 3 more bytes: len_b = 2^32 + 3.  crc_b comes from
    combining shorter pieces (doubling), zlib streams the same bytes as the oracle."""
    piece = np.random.default_rng(8).integers(0, 256, 1 << 24, dtype=np.uint8).tobytes()
    tail, head = b"xyz", b"head bytes"
    c, n = zlib.crc32(piece), len(piece)
    for _ in range(8):   # crc of piece * 2^k
        c, n = checksum.crc32_combine(c, c, n), 2 * n
    crc_b = checksum.crc32_combine(c, zlib.crc32(tail), len(tail))
    len_b = n + len(tail)
    assert len_b == (1 << 32) + 3
    want = zlib.crc32(head)
    for _ in range(256):
        want = zlib.crc32(piece, want)
    want = zlib.crc32(tail, want)
    assert checksum.crc32_combine(zlib.crc32(head), crc_b, len_b) == want
    # x has order 2^32 - 1 modulo the polynomial: the same shift as 4 bytes
    assert checksum.crc32_combine(0x12345678, 0, len_b) == checksum.crc32_combine(0x12345678, 0, 4)


@pytest.mark.parametrize("L", [0, 1, 7, 8, 9, 13, 64, 101])
def test_payload_crc32(L):
    bits = np.random.default_rng(L).integers(0, 2, L, dtype=np.uint8)
    by = bytearray((L + 7) // 8)
    for i, v in enumerate(bits):   # LSB-first, pad bits zero
        by[i // 8] |= int(v) << (i % 8)
    assert checksum.payload_crc32(bits) == zlib.crc32(bytes(by))
    if L % 8:   # the pad bits are zero: appending a 0 bit inside the last byte changes nothing
        assert checksum.payload_crc32(bits) == checksum.payload_crc32(np.append(bits, 0))


@pytest.mark.parametrize("L", [0, 1, 7, 8, 9, 63, 64, 65, 101])
def test_payload_crc32_of_a_packed_row(L):
    """The packed-row form (what embed and decode use) equals the bit-vector form, whatever the
    bits past L in the last byte hold."""
    from codec_tcc_amd import framing
    bits = np.random.default_rng(100 + L).integers(0, 2, L, dtype=np.uint8)
    rows, _lengths = framing.pack_bits([bits])
    raw = rows.copy().view(np.uint8)
    if L % 8:
        raw[0, (L + 7) // 8 - 1] |= (0xFF << (L % 8)) & 0xFF
    assert checksum.payload_crc32_packed(raw[0], L) == checksum.payload_crc32(bits)
    with pytest.raises(ValueError):
        checksum.payload_crc32_packed(raw[0, :1], 9)


def test_integrity_error_is_a_value_error():
    assert issubclass(checksum.IntegrityError, ValueError)
    with pytest.raises(ValueError):
        checksum.verify_mode("maybe")


def test_crc32_slices_has_no_cpu_fallback():
    """A host tensor is never checksummed on the host: without a GPU the package's "no GPU"
    RuntimeError, with one a ValueError for the tensor's device."""
    import torch
    want = (ValueError, "on the GPU") if torch.cuda.is_available() else (RuntimeError, "no GPU")
    with pytest.raises(want[0], match=want[1]):
        checksum.crc32_slices(torch.zeros((1, 4, 4), dtype=torch.uint8))


# ------------------------------------------------------------------ header extension
def _file(hdr: bytes, body: bytes) -> bytes:
    return container.MAGIC + struct.pack(">I", len(hdr)) + hdr + body


def _hdr1(blob=b"lmblob"):
    return container.create_pee_header("raw", 2, 6, 4, 2, 5, 3, 4095, 0, len(blob)), blob + bytes(48)


def _hdr2():
    blobs = [b"aa", b"", b"b", b""]
    passes = [(3, 4, 1, 2), (2, 1, 0, 0), (0, -1, 0, 1), (0, -1, 0, 0)]
    return container.create_pee2_header("raw", 2, 6, 4, 2, 4095, 5, 0, passes), b"".join(blobs) + bytes(48)


def test_extension_round_trips_scheme_1():
    hdr, body = _hdr1()
    ext = container.pee_crc_extension(0xDEADBEEF, 0x01020304)
    assert ext == b"C1" + struct.pack(">II", 0xDEADBEEF, 0x01020304) and len(ext) == 10
    md0, blob0, data0 = container.parse_pee_bytes(_file(hdr, body))
    assert "cover_crc32" not in md0 and "payload_crc32" not in md0
    md, blob, data = container.parse_pee_bytes(_file(hdr + ext, body))
    assert md["cover_crc32"] == 0xDEADBEEF and md["payload_crc32"] == 0x01020304
    assert (blob, data) == (blob0, data0)
    assert {k: v for k, v in md.items() if not k.endswith("crc32")} == md0


def test_extension_round_trips_scheme_2():
    hdr, body = _hdr2()
    ext = container.pee_crc_extension(7, 0xFFFFFFFF)
    md0, blobs0, data0 = container.parse_pee2_bytes(_file(hdr, body))
    assert "cover_crc32" not in md0
    md, blobs, data = container.parse_pee2_bytes(_file(hdr + ext, body))
    assert md["cover_crc32"] == 7 and md["payload_crc32"] == 0xFFFFFFFF
    assert (blobs, data) == (blobs0, data0)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("cut", [1, 2, 5, 9])
def test_header_cut_inside_the_extension_raises(scheme, cut):
    hdr, body = _hdr1() if scheme == 1 else _hdr2()
    ext = container.pee_crc_extension(1, 2)[:cut]
    parse = container.parse_pee_bytes if scheme == 1 else container.parse_pee2_bytes
    with pytest.raises(ValueError, match="truncated"):
        parse(_file(hdr + ext, body))


def test_default_header_layout_is_unchanged():
    """Without checksum the header encode_file_pee writes is create_pee_header's bytes alone:
    the fixed fields' calcsize, nothing after them."""
    hdr, _body = _hdr1()
    assert len(hdr) == struct.calcsize(">BBBBIIiiiiiI") == 36
    assert hdr == struct.pack(">BBBBIIiiiiiI", 16, 0, 2, 0, 6, 4, 2, 5, 3, 4095, 0, 6)
    hdr2, _ = _hdr2()
    assert len(hdr2) == struct.calcsize(">BBBBIIiiii") + 4 * struct.calcsize(">iiiI") == 92
