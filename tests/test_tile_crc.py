"""Tile checksums on the GPU (include/codec_tcc_tile.h): both kernels of
codec_crc32_tiles against zlib on every tile, the compare kernel, and the localisation that
MED-PEE decode reports through IntegrityError.tiles / PeeCodec.verify_tiles -- against the spec's
mismatch map (tests/tile_crc_spec.py) between the cover and what the CPU oracle restores from the
same altered stego."""
import ctypes as C
import struct

import numpy as np
import pytest

import pee_gate_spec as G
import tile_crc_spec as S
from codec_tcc_amd import IntegrityError, _lib, checksum, container, pee, pipeline, synth
from oracle import pee_cpu
from test_crc_gpu import _expanded_candidate

pytestmark = pytest.mark.gpu

T = 2
MAXVAL = 4095


def _torch():
    import torch
    return torch


def _rand(shape, dtype, seed):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=dtype)


def _styled(shape, dtype, seed):
    """Seeded random pixels; of a batch of three the second slice is constant, the third all ones."""
    a = _rand(shape, dtype, seed)
    if shape[0] >= 3:
        a[1] = 0x1234 & np.iinfo(dtype).max
        a[2] = np.iinfo(dtype).max
    return a


# ------------------------------------------------------------------ the kernels against zlib
# name -> (shape, dtype, tile, the route the case must take)
CASES = {
    "u16 tile 64, 128-B rows": ((3, 64, 128), np.uint16, 64, 2),
    "u16 tile (16, 8), one vector per tile row": ((3, 64, 128), np.uint16, (16, 8), 2),
    "u16 tile (8, 4), 8-B rows": ((3, 64, 128), np.uint16, (8, 4), 1),
    "u16 odd W tile 8": ((2, 37, 53), np.uint16, 8, 1),
    "u16 odd W, a tile larger than the image": ((2, 37, 53), np.uint16, 64, 1),
    "u16 2-row bottom edge (nv < 64)": ((1, 130, 192), np.uint16, 64, 2),
    "u16 ragged right edge on an aligned layout": ((2, 64, 136), np.uint16, 64, 2),
    "u16 rows of 3 vectors, 5 tile columns": ((2, 70, 120), np.uint16, (32, 24), 2),
    "u16 tall tile: lanes take more than 4 vectors": ((1, 300, 64), np.uint16, (256, 64), 2),
    "u8 tile 64, 64-B rows": ((2, 64, 128), np.uint8, 64, 2),
    "u8 odd W tile 16": ((2, 33, 47), np.uint8, 16, 1),
    "u8 byte route, tiles of more than 64 rows": ((1, 150, 21), np.uint8, (128, 8), 1),
}

@pytest.mark.parametrize("name", list(CASES))
def test_tiles_equal_zlib(name):
    torch = _torch()
    shape, dtype, tile, route = CASES[name]
    a = _styled(shape, dtype, len(name))
    x = torch.from_numpy(a).cuda()
    assert x.data_ptr() % 16 == 0
    assert checksum.tiles_route(x, tile) == route
    got = checksum.crc32_tiles(x, tile)
    want = S.tile_table(a, tile)
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape == (shape[0],) + S.grid(shape[1], shape[2], tile)
    got = got.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
    assert np.array_equal(checksum.tiles_host(a[0], tile), want[0])


def test_the_cases_cover_both_routes():
    """From the library's own route entry, on the cases' shapes at a 16-byte-aligned base."""
    lib = _lib.load()
    masks = set()
    for shape, dtype, tile, route in CASES.values():
        th, tw = S.tile_pair(tile)
        m = int(lib.codec_crc32_tiles_route(*shape, np.dtype(dtype).itemsize, th, tw, 1 << 20))
        assert m == route
        masks.add(m)
    assert masks == {_lib.TILE_ROUTE_BYTES, _lib.TILE_ROUTE_VECTOR}


@pytest.mark.parametrize("dtype,off", [(np.uint16, 1), (np.uint16, 8), (np.uint8, 1), (np.uint8, 16)])
def test_view_at_an_element_offset(dtype, off):
    """A contiguous view at an odd element offset of a larger buffer takes the byte route and is
    exact; an offset that keeps the base 16-byte aligned stays on the vector route."""
    torch = _torch()
    shape = (2, 64, 128)
    n = int(np.prod(shape))
    buf = torch.from_numpy(_rand((n + off,), dtype, 21 + off)).cuda()
    view = buf[off:].view(shape)
    assert view.is_contiguous() and view.storage_offset() == off
    aligned = (off * np.dtype(dtype).itemsize) % 16 == 0
    assert checksum.tiles_route(view, 64) == (2 if aligned else 1)
    got = checksum.crc32_tiles(view, 64).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, S.tile_table(view.cpu().numpy(), 64))


def test_single_slice_2d_input_and_out_argument():
    torch = _torch()
    a = _rand((64, 128), np.uint16, 31)
    x = torch.from_numpy(a).cuda()
    want = S.tile_table(a, (16, 32))[None]
    got = checksum.crc32_tiles(x, (16, 32))                        # [H, W]: B = 1
    assert tuple(got.shape) == (1, 4, 4) and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    out = torch.full((1, 4, 4), 0x55555555, dtype=torch.int32, device="cuda")
    assert checksum.crc32_tiles(x[None], (16, 32), out=out) is out
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    for bad in (torch.zeros((1, 4, 5), dtype=torch.int32, device="cuda"), torch.zeros((1, 4, 4), dtype=torch.int64, device="cuda"),
                torch.zeros((1, 4, 8), dtype=torch.int32, device="cuda")[:, :, ::2], torch.zeros((1, 4, 4), dtype=torch.int32)):
        with pytest.raises(ValueError):
            checksum.crc32_tiles(x, (16, 32), out=bad)
    with pytest.raises(ValueError):
        checksum.crc32_tiles(x[:, ::2], 16)
    with pytest.raises(ValueError):
        checksum.crc32_tiles(torch.zeros((64, 128), dtype=torch.float32, device="cuda"), 16)


# ------------------------------------------------------------------ the compare kernel
def test_compare_equal_tables_and_planted_differences():
    torch = _torch()
    B, nty, ntx = 3, 5, 15   # nt = 75: two bitmap words, 53 pad bits
    want = _rand((B, nty, ntx), np.uint32, 41).view(np.int32)
    w = torch.from_numpy(want).cuda()
    count, bitmap = checksum.compare_tiles(w.clone(), w)
    assert count.dtype == torch.int32 and bitmap.dtype == torch.int64 and tuple(bitmap.shape) == (B, 2)
    assert count.cpu().tolist() == [0, 0, 0] and not bitmap.cpu().numpy().any()
    planted = {0: [], 1: [0, 63, 64, 74], 2: [5]}
    got = want.copy().reshape(B, -1)
    mask = np.zeros((B, nty * ntx), dtype=bool)
    for b, ts in planted.items():
        for t in ts:
            got[b, t] ^= 1 << (t % 31)
            mask[b, t] = True
    # given, garbage-filled outputs: every word is written, pad bits included
    out = (torch.full((B,), -1, dtype=torch.int32, device="cuda"), torch.full((B, 2), -1, dtype=torch.int64, device="cuda"))
    count, bitmap = checksum.compare_tiles(torch.from_numpy(got.reshape(B, nty, ntx)).cuda(), w, out=out)
    assert count is out[0] and bitmap is out[1]
    assert count.cpu().tolist() == [0, 4, 1]
    words = bitmap.cpu().numpy().view(np.uint64)
    for b in range(B):
        assert np.array_equal(words[b], S.bitmap_words(mask[b])), b
        assert np.array_equal(checksum.bitmap_mask(words[b], nty, ntx), mask[b].reshape(nty, ntx))
    with pytest.raises(ValueError):
        checksum.compare_tiles(w, w[:, :, :-1].contiguous())
    with pytest.raises(ValueError):
        checksum.compare_tiles(w, w.to(torch.int64))
    with pytest.raises(ValueError):
        checksum.compare_tiles(w, w.cpu())


def test_capture_and_replay():
    torch = _torch()
    a, b = _rand((2, 64, 136), np.uint16, 51), _rand((2, 64, 136), np.uint16, 52)
    b[1, :, :64] = a[1, :, :64]   # after the update slice 1 differs from a in tile columns 1 and 2 only
    x = torch.from_numpy(a).cuda()
    ref = checksum.crc32_tiles(x, 64).clone()
    checksum.compare_tiles(ref, ref)   # both kernels have run once before the capture
    table = torch.zeros((2, 1, 3), dtype=torch.int32, device="cuda")
    outs = (torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros((2, 1), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        before = torch.cuda.memory_allocated()
        checksum.crc32_tiles(x, 64, out=table)
        checksum.compare_tiles(table, ref, out=outs)
        assert torch.cuda.memory_allocated() == before   # neither call allocates
    g.replay()
    assert np.array_equal(table.cpu().numpy().view(np.uint32), S.tile_table(a, 64))
    assert outs[0].cpu().tolist() == [0, 0] and not outs[1].cpu().numpy().any()
    x.copy_(torch.from_numpy(b).cuda())
    g.replay()
    eager_table = checksum.crc32_tiles(x, 64)
    eager = checksum.compare_tiles(eager_table, ref)
    assert torch.equal(table, eager_table) and np.array_equal(table.cpu().numpy().view(np.uint32), S.tile_table(b, 64))
    assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])
    assert outs[0].cpu().tolist() == [3, 2] and outs[1].cpu().view(-1).tolist() == [0b111, 0b110]


# ------------------------------------------------------------------ localisation through MED-PEE decode
SHAPE = (3, 40, 56)
TILE = 8
PIX = (1, 18, 26)   # the altered stego pixel: slice 1, an even-even (context) pixel of tile (2, 3)
NBITS = {1: 24, 2: 70}


@pytest.fixture(scope="module")
def covers():
    return np.stack([synth.ct12(SHAPE[1], SHAPE[2], 900 + i) for i in range(SHAPE[0])])


def _payloads(scheme):
    return [np.random.default_rng(50 + b).integers(0, 2, NBITS[scheme], dtype=np.uint8) for b in range(SHAPE[0])]


def _codec(scheme=1, gate=None):
    return pee.PeeCodec(*SHAPE, dtype="uint16", T=T, maxval=MAXVAL, scheme=scheme, gate=gate)


def _alter(enc, pix=PIX, add=64):
    s = enc.stego.cpu().numpy().copy()
    s[pix] += add
    enc.stego = _torch().from_numpy(s).cuda()
    return s


def _tagged(fn):
    """fn()'s result and the sorted list of kernel tags its launches recorded (codec_profile_*)."""
    lib, cap = _lib.load(), 256
    _lib.check(lib.codec_profile_begin(cap), "codec_profile_begin")
    out = fn()
    _torch().cuda.synchronize()
    ms, tags = (C.c_float * cap)(), (C.c_int32 * cap)()
    n = lib.codec_profile_end(ms, tags, cap)
    return out, sorted(_lib.KERNEL_TAGS.get(tags[i], str(tags[i])) for i in range(max(n, 0)))


@pytest.mark.parametrize("gate", [None, 64])
def test_scheme_1_reports_the_altered_pixels_own_tile(covers, gate):
    torch = _torch()
    codec = _codec(1, gate)
    dev = torch.from_numpy(covers).cuda()
    enc = codec.embed(dev, _payloads(1), checksum="tiles", tile=TILE)
    assert enc.tile == (TILE, TILE) and enc.cover_tile_crc.dtype == torch.int32
    assert np.array_equal(enc.cover_tile_crc.cpu().numpy().view(np.uint32), S.tile_table(covers, TILE))
    assert checksum.crc_list(enc.cover_crc) == [checksum.cover_crc32_host(c) for c in covers]
    # unaltered: clean, and the launches of a checksum=True decode -- no tile pass, no compare
    plain = codec.embed(dev, _payloads(1), checksum=True)
    assert plain.cover_tile_crc is None and plain.tile is None
    (bits, cover), tags = _tagged(lambda: codec.decode(enc, verify="require"))
    _r, tags_plain = _tagged(lambda: codec.decode(plain, verify="require"))
    assert tags == tags_plain and not {"k_tile_crc", "k_tile_crc_bytes", "k_tile_compare"} & set(tags)
    assert np.array_equal(cover.cpu().numpy(), covers)
    assert all(np.array_equal(g, w) for g, w in zip(bits, _payloads(1)))
    assert not codec.verify_tiles(enc, cover).any()

    stego = _alter(enc)
    b, y, x = PIX
    if gate is None:
        _st, side = pee_cpu.pee_embed(covers[b], _payloads(1)[b], T, MAXVAL)
        _bits, restored = pee_cpu.pee_extract(stego[b], side)
    else:
        _st, side = G.embed(covers[b], _payloads(1)[b], T, gate, MAXVAL)
        _bits, restored = G.extract(stego[b], side)
    want = S.mismatch_map(covers[b], restored, TILE)
    own = np.zeros(S.grid(SHAPE[1], SHAPE[2], TILE), dtype=bool)
    own[y // TILE, x // TILE] = True
    assert np.array_equal(want, own)   # scheme 1, even tile: the damage never leaves the pixel's tile
    with pytest.raises(IntegrityError) as ei:
        codec.decode(enc)
    e = ei.value
    assert e.bad_cover == [b] and e.tile == (TILE, TILE) and sorted(e.tiles) == [b]
    assert e.tiles[b].dtype == bool and np.array_equal(e.tiles[b], want)
    assert f"({y // TILE}, {x // TILE}) = rows 16..23, columns 24..31" in str(e) and "cover checksum mismatch in slices [1]" in str(e)
    # the same map without raising, beside the data of a verify=False decode
    _bits, cover = codec.decode(enc, verify=False)
    maps = codec.verify_tiles(enc, cover)
    assert maps.dtype == bool and maps.shape == (SHAPE[0],) + own.shape
    assert np.array_equal(maps[b], want) and not maps[0].any() and not maps[2].any()
    assert np.array_equal(maps, S.mismatch_map(covers, cover.cpu().numpy(), TILE))


def test_verify_tiles_rejects_foreign_tables(covers):
    torch = _torch()
    codec = _codec()
    dev = torch.from_numpy(covers).cuda()
    enc = codec.embed(dev, _payloads(1), checksum="tiles", tile=TILE)
    good = enc.cover_tile_crc
    with pytest.raises(ValueError):
        codec.verify_tiles(codec.embed(dev, _payloads(1), checksum=True), dev)   # no table
    for bad in (good[:, :, :-1].contiguous(), good.to(torch.int64), good.cpu(), good[:2].contiguous()):
        enc.cover_tile_crc = bad
        with pytest.raises(ValueError):
            codec.verify_tiles(enc, dev)
    enc.cover_tile_crc, enc.tile = good, (16, 8)   # the table of another grid
    with pytest.raises(ValueError):
        codec.verify_tiles(enc, dev)


def test_scheme_2_damage_stays_within_three_pixels(covers):
    torch = _torch()
    codec = _codec(2)
    enc = codec.embed(torch.from_numpy(covers).cuda(), _payloads(2), checksum="tiles", tile=TILE)
    codec.decode(enc, verify="require")
    stego = _alter(enc)
    b, y, x = PIX
    _st, side = pee_cpu.pee_embed_multi(covers[b], _payloads(2)[b], T, MAXVAL)
    _bits, restored = pee_cpu.pee_extract_multi(stego[b], side)
    want = S.mismatch_map(covers[b], restored, TILE)
    assert want.any()
    with pytest.raises(IntegrityError) as ei:
        codec.decode(enc)
    e = ei.value
    assert e.bad_cover == [b] and sorted(e.tiles) == [b] and np.array_equal(e.tiles[b], want)
    for i, j in np.argwhere(e.tiles[b]):
        r0, r1, c0, c1 = S.box(int(i), int(j), SHAPE[1], SHAPE[2], TILE)
        assert r0 <= y + 3 and r1 > y and c0 <= x + 3 and c1 > x, (i, j)   # holds a pixel of [y, y+3] x [x, x+3]
    _bits, cover = codec.decode(enc, verify=False)
    assert np.array_equal(codec.verify_tiles(enc, cover)[b], want)


def test_flipped_payload_bit_flags_no_tile(covers):
    """The LSB of an expanded candidate carries a payload bit and nothing else: the cover
    restores exactly, only the payload check fails, and no tile pass finds anything."""
    torch = _torch()
    codec = _codec()
    enc = codec.embed(torch.from_numpy(covers).cuda(), _payloads(1), checksum="tiles", tile=TILE)
    y, x, new = _expanded_candidate(enc, enc.stego[1].cpu().numpy(), 1)
    s = enc.stego.cpu().numpy().copy()
    assert abs(int(s[1, y, x]) - new) == 1   # the expanded error's LSB flipped
    s[1, y, x] = new
    enc.stego = torch.from_numpy(s).cuda()
    with pytest.raises(IntegrityError) as ei:
        codec.decode(enc)
    e = ei.value
    assert e.bad_cover == [] and e.bad_payload == [1] and e.tiles == {} and e.tile == (TILE, TILE)
    _bits, cover = codec.decode(enc, verify=False)
    assert np.array_equal(cover.cpu().numpy(), covers)
    assert not codec.verify_tiles(enc, cover).any()


def test_in_place_embed_checksums_the_covers_tiles(covers):
    torch = _torch()
    codec = _codec()
    buf = torch.from_numpy(covers).cuda()
    enc = codec.embed(buf, _payloads(1), stego=buf, checksum="tiles", tile=(16, 8))
    assert enc.stego.data_ptr() == buf.data_ptr() and enc.tile == (16, 8)
    assert np.array_equal(enc.cover_tile_crc.cpu().numpy().view(np.uint32), S.tile_table(covers, (16, 8)))
    assert not np.array_equal(buf.cpu().numpy(), covers)   # the buffer now holds the stego
    _bits, cover = codec.decode(enc, verify="require")
    assert np.array_equal(cover.cpu().numpy(), covers)


# ------------------------------------------------------------------ volume and file
def test_volume_decode_attaches_the_map(covers):
    torch = _torch()
    bits = np.random.default_rng(60).integers(0, 2, 60, dtype=np.uint8)
    vol = pee.encode_volume(torch.from_numpy(covers).cuda(), bits, maxval=MAXVAL, checksum="tiles", tile=TILE)
    assert vol.enc.tile == (TILE, TILE)
    assert np.array_equal(vol.enc.cover_tile_crc.cpu().numpy().view(np.uint32), S.tile_table(covers, TILE))
    got, cover = pee.decode_volume(vol, verify="require")
    assert np.array_equal(got, bits) and np.array_equal(cover.cpu().numpy(), covers)
    _alter(vol.enc)
    b, y, x = PIX
    with pytest.raises(IntegrityError) as ei:
        pee.decode_volume(vol)
    e = ei.value
    assert e.bad_cover == [b] and e.tile == (TILE, TILE) and sorted(e.tiles) == [b]
    own = np.zeros(S.grid(SHAPE[1], SHAPE[2], TILE), dtype=bool)
    own[y // TILE, x // TILE] = True
    assert np.array_equal(e.tiles[b], own) and "rows 16..23, columns 24..31" in str(e)
    _got, cover = pee.decode_volume(vol, verify=False)
    assert np.array_equal(S.mismatch_map(covers, cover.cpu().numpy(), TILE)[b], own)


@pytest.mark.parametrize("scheme", [1, 2])
def test_file_round_trip_and_localised_tamper(covers, scheme, tmp_path):
    img, bits = covers[1], _payloads(scheme)[1]
    H, W = img.shape
    path = str(tmp_path / "t.bin")
    info = pipeline.encode_file_pee(img, bits, path, T=T, maxval=MAXVAL, scheme=scheme, checksum="tiles", tile=TILE)
    assert info["tile"] == (TILE, TILE) and np.array_equal(info["tile_crc32"], S.tile_table(img, TILE))
    assert info["cover_crc32"] == checksum.cover_crc32_host(img)
    raw = open(path, "rb").read()
    pf = pipeline.read_pee_bytes(raw)
    assert pf.md["tile"] == (TILE, TILE) and np.array_equal(pf.md["tile_crc32"], S.tile_table(img, TILE))
    for verify in (True, "require"):
        got, cover = pipeline.decode_bin_pee(path, verify=verify)
        assert np.array_equal(got, bits) and np.array_equal(cover, img)
    # the file is the checksum=True file with the tile extension after C1, nothing else
    plain = str(tmp_path / "c.bin")
    pipeline.encode_file_pee(img, bits, plain, T=T, maxval=MAXVAL, scheme=scheme, checksum=True)
    old = open(plain, "rb").read()
    (hlen,) = struct.unpack(">I", old[4:8])
    ext = container.pee_tile_extension(TILE, TILE, S.tile_table(img, TILE))
    assert raw == old[:4] + struct.pack(">I", hlen + len(ext)) + old[8:8 + hlen] + ext + old[8 + hlen:]
    # one stego pixel altered in the raw body (little-endian uint16, the file's tail)
    _b, y, x = PIX
    tampered = bytearray(raw)
    at = len(raw) - 2 * (H * W - (y * W + x))
    v = struct.unpack("<H", raw[at:at + 2])[0]
    assert v == int(info["stego"][y, x])
    tampered[at:at + 2] = struct.pack("<H", v + 64)
    bad = str(tmp_path / "bad.bin")
    open(bad, "wb").write(bytes(tampered))
    with pytest.raises(IntegrityError) as ei:
        pipeline.decode_bin_pee(bad)
    e = ei.value
    _got, restored = pipeline.decode_bin_pee(bad, verify=False)
    assert e.bad_cover == [0] and e.tile == (TILE, TILE) and sorted(e.tiles) == [0]
    assert np.array_equal(e.tiles[0], S.mismatch_map(img, restored, TILE)) and e.tiles[0][y // TILE, x // TILE]
    assert "MED-PEE file: cover checksum mismatch" in str(e) and "rows 16..23, columns 24..31" in str(e)
    # a reader that knows only C1 (the header cut after it) still reads the file and still fails the slice check
    (hl,) = struct.unpack(">I", tampered[4:8])
    oldreader = bytes(tampered[:4]) + struct.pack(">I", hl - len(ext)) + bytes(tampered[8:8 + hl - len(ext)]) + \
        bytes(tampered[8 + hl:])
    cut = str(tmp_path / "cut.bin")
    open(cut, "wb").write(oldreader)
    with pytest.raises(IntegrityError) as ei:
        pipeline.decode_bin_pee(cut)
    assert ei.value.bad_cover == [0] and ei.value.tiles is None and ei.value.tile is None


def test_checksum_true_file_is_the_parents_format(covers, tmp_path):
    """checksum=True: the fixed header, then container.pee_crc_extension's 10 bytes, the map blob
    and the raw stego -- byte for byte what was written before tile checksums existed."""
    img, bits = covers[0], _payloads(1)[0]
    path = str(tmp_path / "c.bin")
    info = pipeline.encode_file_pee(img, bits, path, T=T, maxval=MAXVAL, checksum=True)
    assert "tile" not in info and "tile_crc32" not in info
    raw = open(path, "rb").read()
    md, blob, _data = container.parse_pee_bytes(raw)
    assert "tile" not in md
    hdr = container.create_pee_header("raw", 2, img.shape[1], img.shape[0], info["T"], info["L"], info["end"],
                                      info["maxval"], info["status"], len(blob)) + \
        container.pee_crc_extension(checksum.cover_crc32_host(img), checksum.payload_crc32(bits))
    assert raw == container.MAGIC + len(hdr).to_bytes(4, "big") + hdr + blob + container.encode_stego_raw(info["stego"])
