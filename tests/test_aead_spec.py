"""tests/aead_spec.py against RFC 8439's published answers and against tests/golden/aead_kat.json,
which the openssl binary made (tests/golden/make_aead_kat.py).  Reads only the JSON: no openssl,
no GPU, no library."""
import json
import os

import pytest

import aead_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = os.path.join(HERE, "golden", "aead_kat.json")
TEXT = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
        b"sunscreen would be it.")


def load_kat():
    with open(KAT) as f:
        return json.load(f)["cases"]


def test_rfc8439_2_3_2_block():
    key = bytes(range(32))
    nonce = bytes.fromhex("000000090000004a00000000")
    block = S.chacha20_block(key, 1, nonce)
    assert block[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert block[-16:].hex() == "b5129cd1de164eb9cbd083e8a2503c4e" and len(block) == 64


def test_rfc8439_2_5_2_tag():
    otk = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert S.poly1305(otk, b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"


def test_rfc8439_2_8_2_aead_under_the_layout():
    key, nonce, aad = bytes(range(0x80, 0xA0)), bytes(range(0x40, 0x48)), bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    assert S.nonce12(7, nonce).hex() == "07000000" + "4041424344454647"
    assert len(TEXT) == 114
    row = S.bytes_row(TEXT, 15)
    ct = S.crypt_row(key, nonce, 7, row, 8 * len(TEXT))
    ct_bytes = S.row_bytes(ct, 8 * len(TEXT))
    assert ct_bytes[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert S.tag(key, nonce, 7, aad, ct, 8 * len(TEXT)).hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert S.crypt_row(key, nonce, 7, ct, 8 * len(TEXT)) == row                      # an involution
    assert S.one_time_key(key, 7, nonce).hex().startswith("7bac2b252db447af09b67a55a4e95584")   # RFC §2.8.2's r


def test_kat_covers_what_it_must():
    cases = load_kat()
    assert 25 <= len(cases) <= 40
    assert {0, 1, 7, 8, 63, 64, 65, 511, 512, 513} <= {c["L"] for c in cases}
    assert any(len(c["aad"]) // 2 % 16 for c in cases) and any(c["index"] == S.STREAM_INDEX for c in cases)
    assert any(c["L"] == 64 * c["row_words"] for c in cases)
    assert cases[0]["tag"] == "1ae10b594f09e26a7e902ecbd0600691"


@pytest.mark.parametrize("i", range(30))
def test_spec_against_openssl_kat(i):
    cases = load_kat()
    assert len(cases) == 30
    c = cases[i]
    key, nonce, aad = bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"]), bytes.fromhex(c["aad"])
    g, L, rw = c["index"], c["L"], c["row_words"]
    assert S.one_time_key(key, g, nonce).hex() == c["otk"]
    assert S.keystream(key, S.nonce12(g, nonce), 1, (L + 7) // 8).hex() == c["keystream"]
    pt = S.bytes_row(bytes.fromhex(c["pt_row"]), rw)
    ct = S.crypt_row(key, nonce, g, pt, L)
    assert b"".join(w.to_bytes(8, "little") for w in ct).hex() == c["ct_row"]
    assert S.tag(key, nonce, g, aad, ct, L).hex() == c["tag"]
    ok, back = S.release(key, nonce, g, bytes.fromhex(c["tag"]), S.tag(key, nonce, g, aad, ct, L), ct, L)
    assert ok == 1 and back == S.bytes_row(S.row_bytes(pt, L), rw)


def test_layout_edges():
    key, nonce = bytes(32), bytes(8)
    with pytest.raises(ValueError):
        S.nonce12(1 << 31 | 1, nonce)
    with pytest.raises(ValueError):
        S.nonce12(-1, nonce)
    with pytest.raises(ValueError):
        S.nonce12(0, bytes(7))
    with pytest.raises(ValueError):
        S.crypt_row(key, nonce, 0, [0], 65)
    with pytest.raises(ValueError):
        S.keystream(key, bytes(12), 0xFFFFFFFF, 128)           # the counter never wraps
    assert S.crypt_row(key, nonce, 0, [0xFFFFFFFFFFFFFFFF, 5], 0) == [0, 0]   # zero past L
    ok, row = S.release(key, nonce, 0, bytes(16), bytes(15) + b"\x80", [1, 2], 70)
    assert ok == 0 and row == [0, 0]
    assert S.mac_data(b"a", b"") == b"a" + bytes(15) + (1).to_bytes(8, "little") + bytes(8)
    assert S.tag_words(bytes(range(16))) == [0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C]
