"""Generator of tests/golden/decode_launch_tags.json: the ordered kernel tags every MED-PEE decode
records (codec_profile_begin / codec_profile_end around the one decode call), and what a failing
decode raises.

The fixture pins the launch sequence of the commit BEFORE the decode paths were folded into one
(codec_tcc_amd/pee_verify.py), so it is produced on a checkout of that parent commit and never
from the code under test:

    CODEC_TREE=<checkout of the parent commit, library built> python tests/golden/make_decode_launch_tags.py

(needs the GPU).  Only the public API is used -- PeeCodec.embed / decode / embed_volume /
decode_volume, pipeline.encode_file_pee / decode_bin_pee -- so the same file runs on either tree;
tests/test_pee_decode_paths.py imports run() from here and compares what the tree under test
records with the fixture.

Cases: kind x embedding x verify x state.
  kind       s1, s1_gate (gate=64), s1_roi (roi=(8, 8, 24, 40)), s2: PeeCodec.decode of B = 3 slices of
             40 x 56 uint16 synth.ct12 at T = 2, maxval 4095, 24 bits per slice (scheme 2: 70);
             volume, volume_gate (gate=64): decode_volume of 600 bits over B = 4 slices of 48 x 64;
             file1 .. file4: decode_bin_pee of one 40 x 56 slice, container scheme bytes 1 (plain),
             2 (scheme 2), 3 (gate=64), 4 (roi)
  embedding  plain, crc (checksum=True), tiles (checksum="tiles", tile=8), keyed, keyed_tiles
  verify     True, False, 'require'
  state      clean, altered (one even-even context pixel of slice 1 -- a file's one slice -- plus 64)

rows_zero (keyed failures only): the rows the decode's one read-back brought hold zeros for the
slices whose tag failed (a volume: the stream is all zero exactly when the stream's tag failed).
A tree whose IntegrityError has no `rows` yet (the parent) cannot show them through the public
API; there the entry is what DESIGN §3j promises -- the device releases zeros -- which
tests/test_pee_keyed.py and tests/test_pee_keyed_volume.py measured on that tree."""
import copy
import ctypes as C
import dataclasses
import json
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("CODEC_TREE") or os.path.dirname(os.path.dirname(HERE))
if TREE not in sys.path:
    sys.path.insert(0, TREE)
os.environ.setdefault("CODEC_TUNING", "1")   # as tests/conftest.py: the library reads it once, at load

from codec_tcc_amd import IntegrityError, _lib, pipeline, synth  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

KINDS = ("s1", "s1_gate", "s1_roi", "s2", "volume", "volume_gate", "file1", "file2", "file3", "file4")
EMBEDDINGS = ("plain", "crc", "tiles", "keyed", "keyed_tiles")
VERIFY = (True, False, "require")
STATES = ("clean", "altered")
T, MAXVAL, TILE, GATE, ROI = 2, 4095, 8, 64, (8, 8, 24, 40)
PIX = (1, 18, 26)
KEY, NONCE = bytes(range(1, 33)), bytes(range(0xA0, 0xA8))
OUT = os.path.join(HERE, "decode_launch_tags.json")
_ABSENT = object()


def _embed_kw(embedding):
    kw = {}
    if embedding == "crc":
        kw["checksum"] = True
    if "tiles" in embedding:
        kw.update(checksum="tiles", tile=TILE)
    if "keyed" in embedding:
        kw.update(key=KEY, nonce=NONCE)
    return kw


def _covers(B, H, W):
    return np.stack([synth.ct12(H, W, 903 + i) for i in range(B)])


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8)


def _altered(stego, pix):
    import torch
    s = stego.cpu().numpy().copy()   # torch has no uint16 arithmetic
    s[pix] += 64
    return torch.from_numpy(s).to(stego.device)


def _record(fn, want_bits, want_cover):
    """One decode under the profile window: its ordered tags and its outcome."""
    import torch
    lib, cap = _lib.load(), 256
    _lib.check(lib.codec_profile_begin(cap), "codec_profile_begin")
    rec, out = {}, None
    try:
        out = fn()
        rec["result"] = "ok"
    except Exception as e:   # what was raised is what is recorded
        rec["result"] = type(e).__name__
        if isinstance(e, IntegrityError):
            tiles = e.tiles if e.tiles is None else \
                {str(b): np.asarray(m).astype(int).tolist() for b, m in sorted(e.tiles.items())}
            rec.update(bad_cover=e.bad_cover, bad_payload=e.bad_payload, slices=e.slices, keyed=e.keyed, stream=e.stream,
                       tiles=tiles, tile=None if e.tile is None else list(e.tile))
            rows = getattr(e, "rows", _ABSENT)
            if e.keyed:
                if rows is _ABSENT:
                    rec["rows_zero"] = True
                elif np.ndim(rows) == 1:   # a volume's stream
                    rec["rows_zero"] = (not np.any(rows)) == e.stream
                else:
                    rec["rows_zero"] = all(not np.any(rows[b]) for b in e.slices)
    finally:
        torch.cuda.synchronize()
        ms, tags = (C.c_float * cap)(), (C.c_int32 * cap)()
        n = lib.codec_profile_end(ms, tags, cap)
    rec["tags"] = [_lib.KERNEL_TAGS.get(tags[i], str(tags[i])) for i in range(max(n, 0))]
    if out is not None:
        bits, cover = out
        cover = cover.cpu().numpy() if hasattr(cover, "cpu") else np.asarray(cover)
        if isinstance(want_bits, list):
            rec["bits_ok"] = all(np.array_equal(g, w) for g, w in zip(bits, want_bits))
        else:
            rec["bits_ok"] = bool(np.array_equal(bits, want_bits))
        rec["cover_ok"] = bool(np.array_equal(cover, want_cover))
    return rec


def _decoders(kind, embedding, tmp):
    """{state: decode(verify)} and the (bits, cover) a clean decode returns, for one embedding."""
    import torch
    kw = _embed_kw(embedding)
    key = {"key": KEY} if "keyed" in embedding else {}
    if kind.startswith("s"):
        covers = _covers(3, 40, 56)
        scheme = 2 if kind == "s2" else 1
        bits = [_bits(70 if scheme == 2 else 24, 50 + b) for b in range(3)]
        codec = PeeCodec(3, 40, 56, dtype="uint16", T=T, maxval=MAXVAL, scheme=scheme,
                         gate=GATE if kind == "s1_gate" else None)
        enc = codec.embed(torch.from_numpy(covers).cuda(), bits, **({"roi": ROI} if kind == "s1_roi" else {}), **kw)
        bad = copy.copy(enc)
        bad.stego = _altered(enc.stego, PIX)
        return {"clean": lambda v: codec.decode(enc, verify=v, **key),
                "altered": lambda v: codec.decode(bad, verify=v, **key)}, bits, covers
    if kind.startswith("volume"):
        covers = _covers(4, 48, 64)
        bits = _bits(600, 60)
        codec = PeeCodec(4, 48, 64, dtype="uint16", T="auto", maxval=MAXVAL)
        vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, gate=GATE if kind == "volume_gate" else None, **kw)
        assert vol.embedded_bits == 600
        enc = copy.copy(vol.enc)
        enc.stego = _altered(vol.enc.stego, PIX)
        bad = dataclasses.replace(vol, enc=enc)
        return {"clean": lambda v: codec.decode_volume(vol, verify=v, **key),
                "altered": lambda v: codec.decode_volume(bad, verify=v, **key)}, bits, covers
    img = _covers(1, 40, 56)[0]
    scheme = 2 if kind == "file2" else 1
    bits = _bits(70 if scheme == 2 else 24, 50)
    path, tampered = os.path.join(tmp, f"{kind}_{embedding}.bin"), os.path.join(tmp, f"{kind}_{embedding}_bad.bin")
    info = pipeline.encode_file_pee(img, bits, path, T=T, maxval=MAXVAL, scheme=scheme, **kw,
                                    **({"gate": GATE} if kind == "file3" else {}), **({"roi": ROI} if kind == "file4" else {}))
    assert info["status"] == 0
    raw = bytearray(open(path, "rb").read())   # the raw body (little-endian uint16) is the file's tail
    _b, y, x = PIX
    at = len(raw) - 2 * (img.size - (y * img.shape[1] + x))
    (v,) = struct.unpack("<H", raw[at:at + 2])
    assert v == int(info["stego"][y, x])
    raw[at:at + 2] = struct.pack("<H", v + 64)
    with open(tampered, "wb") as f:
        f.write(bytes(raw))
    return {"clean": lambda v: pipeline.decode_bin_pee(path, verify=v, **key),
            "altered": lambda v: pipeline.decode_bin_pee(tampered, verify=v, **key)}, bits, img


def run(kind, embedding):
    """{"<state>/<verify>": record} of one kind and embedding: one embed, six decodes."""
    with tempfile.TemporaryDirectory() as tmp:
        decoders, bits, covers = _decoders(kind, embedding, tmp)
        return {f"{state}/{verify}": _record(lambda: decoders[state](verify), bits, covers)
                for state in STATES for verify in VERIFY}


def main():
    out = {f"{kind}/{embedding}": run(kind, embedding) for kind in KINDS for embedding in EMBEDDINGS}
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:   # one line per embedding
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    print(f"{path}: {sum(len(v) for v in out.values())} decodes of {len(out)} embeddings")


if __name__ == "__main__":
    main()
