"""Host side of the tile checksums (include/codec_tcc_tile.h): the entry list, the
pure-host grid and route entries, the argument rules, the b"T1" header extension of the
version-16 container, IntegrityError's attributes, and the known answers that pin the spec
(tests/tile_crc_spec.py, zlib) -- no GPU."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest

import tile_crc_spec as S
from codec_tcc_amd import _lib, build, checksum, container

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGNED = 1 << 20   # a stand-in address: the route entry looks at its alignment only


def _grid(H, W, th, tw):
    a, b = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.load().codec_crc32_tiles_grid(H, W, th, tw, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def _route(B, H, W, nbytes, th, tw, addr=ALIGNED):
    return int(_lib.load().codec_crc32_tiles_route(B, H, W, nbytes, th, tw, addr))


# ------------------------------------------------------------------ entries and build inputs
def test_header_declarations_equal_the_loaders_list():
    hdr = open(os.path.join(REPO, "include", "codec_tcc_tile.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_TILE) == {"codec_crc32_tiles_grid", "codec_crc32_tiles_route",
                                                  "codec_crc32_tiles", "codec_crc32_tiles_compare"}
    others = (_lib.EXPORTS, _lib.EXPORTS_EXT, _lib.EXPORTS_CRC, _lib.EXPORTS_VOL, _lib.EXPORTS_GATE, _lib.EXPORTS_GVOL)
    for lst in others:
        assert not declared & set(lst)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.EXPORTS_TILE)
    assert {43: "k_tile_crc", 44: "k_tile_crc_bytes", 45: "k_tile_compare"}.items() <= _lib.KERNEL_TAGS.items()
    for name, tag in (("TILE_CRC", 43), ("TILE_CRC_BYTES", 44), ("TILE_COMPARE", 45)):
        assert f"#define CODEC_K_{name} {tag}" in hdr
    assert f"#define CODEC_TILE_MIN {_lib.TILE_MIN}" in hdr and f"#define CODEC_TILE_MAX {_lib.TILE_MAX}" in hdr
    assert (_lib.TILE_MIN, _lib.TILE_MAX) == (S.TILE_MIN, S.TILE_MAX) == (4, 1024)


def test_build_digest_covers_the_new_unit_and_headers():
    deps = build.SRCS + build._common_deps()
    assert os.path.join(build.HERE, "csrc", "codec_tile.hip") in build.SRCS
    assert os.path.join(build.INC, "codec_tcc_tile.h") in build._common_deps()
    assert os.path.join(build.HERE, "csrc", "codec_crc_gf2.h") in build._common_deps()
    assert all(os.path.exists(p) for p in deps)
    # the shared GF(2) routines live in the private header alone: one routine behind every constant
    for unit in ("codec_crc.hip", "codec_tile.hip"):
        text = open(os.path.join(build.HERE, "csrc", unit)).read()
        assert '#include "codec_crc_gf2.h"' in text
        assert not re.search(r"constexpr\s+uint32_t\s+crc_(mulmod|xpow)\s*\(", text), unit
        assert not re.search(r"uint\w+\s+crc_(mul_tab|fold4|gather_bytes)\s*\(const", text), unit


# ------------------------------------------------------------------ grid
@pytest.mark.parametrize("H,W,th,tw", [(64, 128, 64, 64), (37, 53, 8, 8), (37, 53, 64, 64), (5, 130, 64, 8),
                                       (130, 192, 64, 64), (1, 1, 4, 4), (2048, 2048, 4, 4), (2048, 2048, 1024, 1024),
                                       (1025, 1023, 1024, 1024), (40, 56, 16, 8), (1, 2 ** 31 - 1, 4, 1024),
                                       (32768, 65536, 1024, 4)])
def test_grid_entry_equals_the_spec(H, W, th, tw):
    rc, nty, ntx = _grid(H, W, th, tw)
    assert rc == 0 and (nty, ntx) == S.grid(H, W, (th, tw)) == checksum.tile_grid(H, W, (th, tw))


@pytest.mark.parametrize("H,W,th,tw", [(64, 64, 3, 64), (64, 64, 64, 3), (64, 64, 0, 8), (64, 64, 8, -8),
                                       (64, 64, 1025, 8), (64, 64, 8, 1025), (64, 64, 2 ** 31 - 1, 8),
                                       (0, 64, 8, 8), (64, 0, 8, 8), (-1, 64, 8, 8), (65536, 65536, 8, 8)])
def test_grid_entry_refuses(H, W, th, tw):
    rc, nty, ntx = _grid(H, W, th, tw)
    assert rc < 0 and _lib.load().codec_last_error()
    assert (nty, ntx) == (-7, -7)   # nothing written
    assert _lib.load().codec_crc32_tiles_grid(64, 64, 8, 8, None, None) < 0


# ------------------------------------------------------------------ routes
def test_route_masks():
    assert _route(3, 64, 128, 2, 64, 64) == 2                  # aligned rows of 128 B: the vector route
    assert _route(3, 64, 128, 2, 16, 8) == 2                   # a tile row is one 16-B vector
    assert _route(3, 64, 128, 2, 8, 4) == 1                    # 8-B tile rows
    assert _route(2, 37, 53, 2, 8, 8) == 1                     # odd W
    assert _route(2, 64, 128, 1, 64, 64) == 2 and _route(2, 33, 47, 1, 16, 16) == 1
    assert _route(3, 64, 128, 2, 64, 64, ALIGNED + 2) == 1     # an unaligned base
    assert _route(3, 64, 128, 2, 64, 64, ALIGNED + 16) == 2


def test_route_of_a_ragged_right_edge_is_documented():
    """Aligned interior tiles with a ragged last column.  The header's rule: a call takes ONE
    route; the vector route's conditions (tw * bytes, W * bytes and the base multiples of 16)
    make the last column's rows whole vectors too, so [2, 64, 136] uint16 at tile 64 -- 8-px =
    16-B edge rows -- is all vector; W = 132 (264-B rows, odd rows unaligned) is all bytes."""
    assert _route(2, 64, 136, 2, 64, 64) == 2
    assert _route(2, 64, 132, 2, 64, 64) == 1
    hdr = open(os.path.join(REPO, "include", "codec_tcc_tile.h")).read()
    assert "ONE route" in hdr and "A mixed call does not exist" in hdr


@pytest.mark.parametrize("args", [(0, 64, 64, 2, 8, 8), (-1, 64, 64, 2, 8, 8), (1, 0, 64, 2, 8, 8), (1, 64, 64, 3, 8, 8),
                                  (1, 64, 64, 0, 8, 8), (1, 64, 64, 2, 3, 8), (1, 64, 64, 2, 8, 1025),
                                  (1, 65536, 65536, 1, 8, 8), (2 ** 31 - 1, 64, 64, 2, 4, 4)])
def test_route_entry_refuses(args):
    assert _route(*args) < 0 and _lib.load().codec_last_error()


def test_route_entry_refuses_null():
    assert _route(1, 64, 64, 2, 8, 8, None) < 0


# ------------------------------------------------------------------ Python argument rules
@pytest.mark.parametrize("tile", [3, 0, -4, 1025, (8, 3), (1025, 8), (8,), (8, 8, 8), 8.0, (8, 8.5), "64", None, True,
                                  (True, 8)])
def test_check_tile_args_rejects(tile):
    with pytest.raises(ValueError):
        checksum.check_tile_args(tile)


def test_check_tile_args_accepts():
    assert checksum.check_tile_args(64) == (64, 64)
    assert checksum.check_tile_args((16, 8)) == (16, 8) == checksum.check_tile_args([16, 8])
    assert checksum.check_tile_args(np.int64(4)) == (4, 4) and checksum.check_tile_args(1024) == (1024, 1024)
    assert checksum.tile_grid(37, 53, 8) == (5, 7)
    assert checksum.checksum_mode(False) == (False, False) and checksum.checksum_mode(True) == (True, False)
    assert checksum.checksum_mode("tiles") == (True, True)
    assert checksum.checksum_mode(1) == (True, False) and checksum.checksum_mode(None) == (False, False)
    for bad in ("tile", "True", ""):
        with pytest.raises(ValueError):
            checksum.checksum_mode(bad)


def test_bad_tile_raises_before_the_gpu_is_touched():
    """ValueError for the tile, never the package's "no GPU" RuntimeError nor a device error."""
    import torch
    from codec_tcc_amd import pee, pipeline
    img = np.zeros((16, 16), dtype=np.uint16)
    with pytest.raises(ValueError, match="tile"):
        checksum.crc32_tiles(torch.zeros((1, 16, 16), dtype=torch.uint8), tile=3)
    with pytest.raises(ValueError, match="tile"):
        pee.encode(img, [b"a"], checksum="tiles", tile=2000)
    with pytest.raises(ValueError, match="tile"):
        pee.encode_volume(img[None], b"a", checksum="tiles", tile=(8, 2))
    with pytest.raises(ValueError, match="checksum"):
        pee.encode(img, [b"a"], checksum="tile")
    with pytest.raises(ValueError, match="tile"):
        pipeline.encode_file_pee(img, b"a", "/nonexistent/x.bin", checksum="tiles", tile=0)


def test_crc32_tiles_has_no_cpu_fallback():
    import torch
    want = (ValueError, "on the GPU") if torch.cuda.is_available() else (RuntimeError, "no GPU")
    with pytest.raises(want[0], match=want[1]):
        checksum.crc32_tiles(torch.zeros((1, 8, 8), dtype=torch.uint8))


# ------------------------------------------------------------------ known answers
def _kat():
    with open(os.path.join(REPO, "tests", "golden", "tile_crc_kat.json")) as f:
        return json.load(f)["cases"]


def test_kat_pins_the_spec_and_tiles_host():
    cases = _kat()
    assert len(cases) >= 6 * 4
    seen = set()
    for c in cases:
        img = np.random.default_rng(c["seed"]).integers(0, c["top"], c["shape"]).astype(c["dtype"])
        tile = tuple(c["tile"]) if isinstance(c["tile"], list) else c["tile"]
        want = np.array(c["table"], dtype=np.uint32)
        assert tuple(c["grid"]) == want.shape == S.grid(*c["shape"], tile)
        assert np.array_equal(S.tile_table(img, tile), want)
        assert np.array_equal(checksum.tiles_host(img, tile), want)
        seen.add((c["dtype"], c["shape"][1] % 2, str(tile)))
    assert {d for d, _o, _t in seen} == {"uint8", "uint16"} and {o for _d, o, _t in seen} == {0, 1}
    assert {t for _d, _o, t in seen} == {"4", "8", "(16, 8)", "64"}


def test_spec_mismatch_map_and_bitmap_words():
    a = np.random.default_rng(3).integers(0, 4096, (37, 53)).astype(np.uint16)
    b = a.copy()
    b[9, 17] ^= 1
    b[36, 52] ^= 1
    m = S.mismatch_map(a, b, 8)
    assert m.shape == (5, 7) and sorted(map(tuple, np.argwhere(m))) == [(1, 2), (4, 6)]
    assert np.array_equal(m, S.tile_table(a, 8) != S.tile_table(b, 8))
    w = S.bitmap_words(m)
    assert w.shape == (1,) and int(w[0]) == (1 << 9) | (1 << 34)
    assert np.array_equal(checksum.bitmap_mask(w, 5, 7), m)
    big = np.zeros((9, 9), dtype=bool)
    big[8, 8] = big[7, 0] = True
    w = S.bitmap_words(big)
    assert w.shape == (2,) and int(w[0]) == 1 << 63 and int(w[1]) == 1 << 16
    assert np.array_equal(checksum.bitmap_mask(w, 9, 9), big)


# ------------------------------------------------------------------ container: the b"T1" extension
def _file(hdr: bytes, body: bytes) -> bytes:
    return container.MAGIC + struct.pack(">I", len(hdr)) + hdr + body


def _hdr1(w=53, h=37, blob=b"lmblob"):
    return container.create_pee_header("raw", 2, w, h, 2, 5, 3, 4095, 0, len(blob)), blob + bytes(48)


def _hdr2(w=53, h=37):
    blobs = [b"aa", b"", b"b", b""]
    passes = [(3, 4, 1, 2), (2, 1, 0, 0), (0, -1, 0, 1), (0, -1, 0, 0)]
    return container.create_pee2_header("raw", 2, w, h, 2, 4095, 5, 0, passes), b"".join(blobs) + bytes(48)


def _hdr3(w=53, h=37, blob=b"lmblob"):
    return container.create_pee_gate_header("raw", 2, w, h, 2, 5, 3, 4095, 0, len(blob), 12), blob + bytes(48)


PARSERS = {1: (_hdr1, container.parse_pee_bytes), 2: (_hdr2, container.parse_pee2_bytes),
           3: (_hdr3, container.parse_pee_gate_bytes)}


def _table(h=37, w=53, tile=(16, 8)):
    img = np.random.default_rng(5).integers(0, 4096, (h, w)).astype(np.uint16)
    return S.tile_table(img, tile)


def test_tile_extension_bytes():
    t = _table()
    ext = container.pee_tile_extension(16, 8, t)
    assert ext[:2] == b"T1" and struct.unpack(">HHHH", ext[2:10]) == (16, 8, 3, 7)
    assert len(ext) == 10 + 4 * 21
    assert list(struct.unpack(">21I", ext[10:])) == [int(v) for v in t.reshape(-1)]
    # an int32 view of the same bits (what the device table reads back as) gives the same bytes
    assert container.pee_tile_extension(16, 8, t.view(np.int32)) == ext
    for bad in ((3, 8), (16, 1025)):
        with pytest.raises(ValueError):
            container.pee_tile_extension(*bad, t)
    with pytest.raises(ValueError):
        container.pee_tile_extension(16, 8, np.zeros((0, 3), dtype=np.uint32))
    with pytest.raises(ValueError):
        container.pee_tile_extension(4, 4, np.zeros((65536, 1), dtype=np.uint32))


@pytest.mark.parametrize("scheme", [1, 2, 3])
def test_tile_extension_round_trips(scheme):
    make, parse = PARSERS[scheme]
    hdr, body = make()
    c1 = container.pee_crc_extension(0xDEADBEEF, 0x01020304)
    t = _table()
    md0, blob0, data0 = parse(_file(hdr + c1, body))
    assert "tile" not in md0 and "tile_crc32" not in md0
    md, blob, data = parse(_file(hdr + c1 + container.pee_tile_extension(16, 8, t), body))
    assert md["tile"] == (16, 8) and md["tile_crc32"].dtype == np.uint32 and np.array_equal(md["tile_crc32"], t)
    assert (blob, data) == (blob0, data0)
    assert {k: v for k, v in md.items() if not k.startswith("tile")} == md0
    assert md["cover_crc32"] == 0xDEADBEEF and md["payload_crc32"] == 0x01020304


@pytest.mark.parametrize("scheme", [1, 2, 3])
@pytest.mark.parametrize("cut", [1, 2, 5, 9, 10, 11, 50, 93])
def test_header_cut_inside_the_tile_extension_raises(scheme, cut):
    make, parse = PARSERS[scheme]
    hdr, body = make()
    ext = container.pee_crc_extension(1, 2) + container.pee_tile_extension(16, 8, _table())[:cut]
    with pytest.raises(ValueError, match="truncated"):
        parse(_file(hdr + ext, body))


@pytest.mark.parametrize("scheme", [1, 2, 3])
def test_grid_contradicting_the_header_raises(scheme):
    make, parse = PARSERS[scheme]
    c1 = container.pee_crc_extension(1, 2)
    ext = container.pee_tile_extension(16, 8, _table())          # a 3 x 7 grid: 37 x 53 pixels
    hdr, body = make(w=57, h=37)                                   # 8 tile columns needed
    with pytest.raises(ValueError, match="contradicts"):
        parse(_file(hdr + c1 + ext, body))
    hdr, body = make(w=53, h=49)                                   # 4 tile rows needed
    with pytest.raises(ValueError, match="contradicts"):
        parse(_file(hdr + c1 + ext, body))
    hdr, body = make()
    bad = ext[:2] + struct.pack(">HHHH", 2, 8, 19, 7) + ext[10:]  # a tile size out of range
    with pytest.raises(ValueError, match="tile size"):
        parse(_file(hdr + c1 + bad, body))


def test_the_c1_extension_and_its_parse_are_unchanged():
    assert container.pee_crc_extension(0xDEADBEEF, 0x01020304) == b"C1" + struct.pack(">II", 0xDEADBEEF, 0x01020304)
    hdr, body = _hdr1()
    md0, _b, _d = container.parse_pee_bytes(_file(hdr, body))
    assert md0 == {"version": 16, "codec": "raw", "bytes": 2, "width": 53, "height": 37, "T": 2, "L": 5, "end": 3,
                   "maxval": 4095, "status": 0}
    md, _b, _d = container.parse_pee_bytes(_file(hdr + container.pee_crc_extension(7, 9), body))
    assert md == dict(md0, cover_crc32=7, payload_crc32=9)
    # bytes after C1 that are no tile extension are ignored, as they always were
    md2, _b, _d = container.parse_pee_bytes(_file(hdr + container.pee_crc_extension(7, 9) + b"ZZ" + bytes(9), body))
    assert md2 == md
    # T1 without C1 before it is not an extension position: ignored like any other tail
    md3, _b, _d = container.parse_pee_bytes(_file(hdr + container.pee_tile_extension(16, 8, _table()), body))
    assert md3 == md0


# ------------------------------------------------------------------ IntegrityError
def test_integrity_error_attributes_and_message():
    e = checksum.IntegrityError("x")
    assert isinstance(e, ValueError) and (e.bad_cover, e.bad_payload, e.tiles, e.tile) == ([], [], None, None)
    # the existing cases: message format unchanged, attributes filled
    with pytest.raises(checksum.IntegrityError) as ei:
        checksum.raise_mismatch([0, 2], [1])
    assert str(ei.value) == ("MED-PEE decode: cover checksum mismatch in slices [0, 2]; payload checksum mismatch in "
                             "slices [1] (CRC-32: this is not what was embedded)")
    assert (ei.value.bad_cover, ei.value.bad_payload, ei.value.tiles, ei.value.tile) == ([0, 2], [1], None, None)
    with pytest.raises(checksum.IntegrityError) as ei:
        checksum.raise_mismatch([], [3], "MED-PEE file")
    assert str(ei.value) == "MED-PEE file: payload checksum mismatch in slices [3] (CRC-32: this is not what was embedded)"
    assert checksum.raise_mismatch([], []) is None
    # with tile maps: the first few differing tiles as (row, column) with their pixel boxes
    m = np.zeros((5, 7), dtype=bool)
    for ij in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 6)):
        m[ij] = True
    with pytest.raises(checksum.IntegrityError) as ei:
        checksum.raise_mismatch([1], [], tiles={1: m}, tile=(8, 8), shape=(37, 53))
    e, msg = ei.value, str(ei.value)
    assert e.bad_cover == [1] and e.bad_payload == [] and e.tile == (8, 8) and np.array_equal(e.tiles[1], m)
    assert msg.startswith("MED-PEE decode: cover checksum mismatch in slices [1] (CRC-32: this is not what was embedded)")
    assert "slice 1: 5 of 35 tiles differ" in msg and "(0, 1) = rows 0..7, columns 8..15" in msg
    assert "(3, 4) = rows 24..31, columns 32..39" in msg and "(4, 6)" not in msg and "1 more" in msg
    # a payload-only failure of an encoding with a table: no differing tile, the old message
    with pytest.raises(checksum.IntegrityError) as ei:
        checksum.raise_mismatch([], [0], tiles={}, tile=(8, 8), shape=(37, 53))
    assert ei.value.tiles == {} and ei.value.tile == (8, 8)
    assert str(ei.value) == "MED-PEE decode: payload checksum mismatch in slices [0] (CRC-32: this is not what was embedded)"
    assert checksum.tile_box(4, 6, (8, 8), (37, 53)) == (32, 37, 48, 53)
