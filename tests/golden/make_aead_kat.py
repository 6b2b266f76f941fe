"""Writes tests/golden/aead_kat.json: known answers for keyed MED-PEE (tests/aead_spec.py,
include/codec_tcc_aead.h) made with the local `openssl` binary, never with the specification:

  keystream  openssl enc -chacha20 -K <key> -iv <LE32(counter) || nonce12>   on zeros
  tag        openssl mac -macopt hexkey:<otk> -in FILE POLY1305

The layout (nonce12 = LE32(index) || nonce, otk = the first 32 keystream bytes at counter 0, the
row's first L bits xor the keystream from counter 1, mac_data = pad16(AAD) || pad16(CT) ||
LE64(len AAD) || LE64(ceil(L / 8))) is restated here on bytes.  Deterministic: the inputs come
from a fixed seed.  Run from the repository root:  python tests/golden/make_aead_kat.py
"""
import json
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "aead_kat.json")
LENGTHS = [0, 1, 7, 8, 63, 64, 65, 511, 512, 513]
STREAM_INDEX = 0x80000000


def openssl_keystream(key: bytes, counter: int, nonce12: bytes, n: int) -> bytes:
    if n == 0:
        return b""
    iv = counter.to_bytes(4, "little") + nonce12
    r = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()], input=bytes(n),
                       capture_output=True, check=True)
    assert len(r.stdout) == n
    return r.stdout


def openssl_poly1305(otk: bytes, msg: bytes) -> bytes:
    with tempfile.NamedTemporaryFile() as f:
        f.write(msg)
        f.flush()
        r = subprocess.run(["openssl", "mac", "-macopt", "hexkey:" + otk.hex(), "-in", f.name, "POLY1305"],
                           capture_output=True, check=True, text=True)
    return bytes.fromhex(r.stdout.strip())


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def make_case(rng, name, g, aad_len, L, row_words=None, key=None, nonce=None, aad=None, pt=None):
    key = key if key is not None else bytes(rng.randrange(256) for _ in range(32))
    nonce = nonce if nonce is not None else bytes(rng.randrange(256) for _ in range(8))
    aad = aad if aad is not None else bytes(rng.randrange(256) for _ in range(aad_len))
    nb = (L + 7) // 8
    row_words = row_words if row_words is not None else max(1, (L + 63) // 64 + rng.randrange(2))
    # the plaintext row: random in every bit, also past L (the kernels must ignore those)
    row = bytearray(pt + bytes(8 * row_words - len(pt))) if pt is not None else \
        bytearray(rng.randrange(256) for _ in range(8 * row_words))
    nonce12 = g.to_bytes(4, "little") + nonce
    otk = openssl_keystream(key, 0, nonce12, 64)[:32]
    ks = openssl_keystream(key, 1, nonce12, nb)
    ct = bytearray(a ^ b for a, b in zip(row[:nb], ks))
    if L % 8:
        ct[-1] &= (1 << (L % 8)) - 1
    ct = bytes(ct)
    mac_data = pad16(aad) + pad16(ct) + len(aad).to_bytes(8, "little") + nb.to_bytes(8, "little")
    tag = openssl_poly1305(otk, mac_data)
    return {"name": name, "key": key.hex(), "nonce": nonce.hex(), "index": g, "aad": aad.hex(), "L": L,
            "row_words": row_words, "pt_row": bytes(row).hex(), "otk": otk.hex(), "keystream": ks.hex(),
            "ct_row": (ct + bytes(8 * row_words - nb)).hex(), "tag": tag.hex()}


def main():
    rng = random.Random(0xAEAD)
    cases = []
    # RFC 8439 §2.8.2 under the layout: index0 = 7, nonce = 40..47
    text = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
            b"sunscreen would be it.")
    cases.append(make_case(rng, "rfc8439-2.8.2", 7, 12, 8 * len(text), row_words=15, key=bytes(range(0x80, 0xA0)),
                           nonce=bytes(range(0x40, 0x48)), aad=bytes.fromhex("50515253c0c1c2c3c4c5c6c7"), pt=text))
    aads = [0, 1, 15, 16, 17, 31, 33, 100, 255, 257]
    for i, L in enumerate(LENGTHS):
        cases.append(make_case(rng, f"L{L}", rng.randrange(1 << 31), aads[i], L))
    for i, L in enumerate(LENGTHS):   # the same lengths with other AAD sizes, small indices
        cases.append(make_case(rng, f"L{L}-b", i, aads[(i + 3) % len(aads)], L))
    cases.append(make_case(rng, "index-max", (1 << 31) - 1, 40, 200))
    for L in (0, 513, 4099):          # the volume stream: reserved index, empty AAD
        cases.append(make_case(rng, f"stream-L{L}", STREAM_INDEX, 0, L))
    for n in (1, 47, 4096 + 5):       # cover tags: an empty CT
        cases.append(make_case(rng, f"cover-aad{n}", rng.randrange(1 << 31), n, 0, row_words=1))
    cases.append(make_case(rng, "full-row", 3, 1961, 64 * 40, row_words=40))
    cases.append(make_case(rng, "three-blocks-and-a-bit", 5, 21, 3 * 512 + 1))
    with open(OUT, "w") as f:
        json.dump({"made_with": subprocess.run(["openssl", "version"], capture_output=True, text=True).stdout.strip(),
                   "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main()
