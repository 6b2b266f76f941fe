"""codec_crc32_slices on the GPU against zlib, and the checksummed MED-PEE decode
(codec_tcc_amd/checksum.py, PeeCodec.embed(checksum=True) / decode(verify=...), the file
header extension).  zlib is the independent oracle for every checksum; the tampering cases
find their pixels with oracle/pee_cpu.py."""
import zlib

import numpy as np
import pytest

from codec_tcc_amd import IntegrityError, checksum, crc32_slices, pee, pipeline, synth
from oracle import pee_cpu

pytestmark = pytest.mark.gpu

T = 2
MAXVAL = 4095


def _torch():
    import torch
    return torch


def _zlib(a: np.ndarray):
    a = np.ascontiguousarray(a)
    if a.ndim == 2:
        a = a[None]
    return [zlib.crc32(s.astype(s.dtype.newbyteorder("<"), copy=False).tobytes()) for s in a]


def _check(a: np.ndarray):
    t = _torch().from_numpy(np.ascontiguousarray(a)).cuda()
    got = checksum.crc_list(crc32_slices(t))
    assert got == _zlib(a), (a.shape, a.dtype)


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=dtype)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (3, 5, 7)])
def test_uint8_small_and_unaligned_slice_bases(shape):
    _check(_rand(shape, np.uint8, 1))


@pytest.mark.parametrize("shape", [(7, 9), (4, 512, 512)])
def test_uint16_shapes(shape):
    _check(_rand(shape, np.uint16, 2))


def test_uint16_2048_square():
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(3)
    t = torch.randint(-32768, 32768, (2048, 2048), generator=g, device="cuda", dtype=torch.int16).view(torch.uint16)
    assert checksum.crc_list(crc32_slices(t)) == _zlib(t.cpu().numpy())


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_chunk_seams(k, d):
    n = k * checksum.chunk_bytes() + d
    _check(_rand((1, n), np.uint8, 10 * k + d))


@pytest.mark.parametrize("fill", [0, 0xFF])
def test_constant_slices_of_two_sizes(fill):
    """The CRC of a run of equal bytes depends only on its length: seam and length mistakes show."""
    ch = checksum.chunk_bytes()
    got = []
    for n in (1000, ch + 17):
        a = np.full((2, 1, n), fill, dtype=np.uint8)
        _check(a)
        got.append(_zlib(a)[0])
    assert got[0] != got[1]


def test_view_at_an_odd_byte_offset():
    torch = _torch()
    n = 3 * 4099
    buf = torch.from_numpy(_rand((n + 1,), np.uint8, 4)).cuda()
    view = buf[1:].view(3, 1, 4099)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert checksum.crc_list(crc32_slices(view)) == _zlib(view.cpu().numpy())


def test_rejects_non_contiguous_and_wrong_dtype():
    torch = _torch()
    t = torch.from_numpy(np.zeros((2, 8, 8), dtype=np.uint16)).cuda()
    with pytest.raises(ValueError):
        crc32_slices(t[:, :, ::2])
    with pytest.raises(ValueError):
        crc32_slices(t.transpose(1, 2))
    with pytest.raises(ValueError):
        crc32_slices(torch.zeros((2, 8, 8), dtype=torch.float32, device="cuda"))


def test_out_argument_and_graph_capture():
    torch = _torch()
    a = _rand((2, 33, 47), np.uint16, 5)
    b = _rand((2, 33, 47), np.uint16, 6)
    x = torch.from_numpy(a).cuda()
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert crc32_slices(x, out=out) is out
    assert checksum.crc_list(out) == _zlib(a)
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        crc32_slices(x, out=out)
    g.replay()
    assert checksum.crc_list(out) == _zlib(a)
    x.copy_(torch.from_numpy(b).cuda())
    g.replay()
    assert checksum.crc_list(out) == _zlib(b)


# ------------------------------------------------------------------ MED-PEE integration
NBITS = {1: 48, 2: 100}


@pytest.fixture(scope="module")
def covers():
    return np.stack([synth.ct12(64, 64, 700 + i) for i in range(2)])


def _payloads(scheme):
    rng = np.random.default_rng(40 + scheme)
    return [rng.integers(0, 2, NBITS[scheme], dtype=np.uint8) for _ in range(2)]


def _codec(scheme):
    return pee.PeeCodec(2, 64, 64, dtype="uint16", T=T, maxval=MAXVAL, scheme=scheme)


def _embed(covers, scheme, **kw):
    codec = _codec(scheme)
    enc = codec.embed(_torch().from_numpy(covers).cuda(), _payloads(scheme), **kw)
    return codec, enc


def _poke(enc, b, y, x, fn):
    """Replace stego pixel (b, y, x) by fn(its value) (through the host: one pixel)."""
    s = enc.stego.cpu().numpy().copy()
    s[b, y, x] = fn(int(s[b, y, x]))
    enc.stego = _torch().from_numpy(s).cuda()


def _expanded_candidate(enc, stego: np.ndarray, b: int):
    """(y, x, new value) of an expanded candidate of slice b whose payload bit flips when the
    pixel is replaced: the last pass that embedded bits, index <= end, not in the map,
    -2T <= e' < 2T, pred + (e' xor 1) inside [0, maxval]."""
    prs = enc.pass_records()
    p = max(q for q in range(len(prs)) if prs[q][b].L > 0)
    r = prs[p][b]
    x, a, bb, c = pee_cpu._grids(stego, p)
    pred = pee_cpu.med(a, bb, c).ravel()
    e2 = x.ravel() - pred
    lm = np.zeros(e2.size, bool)
    lm[: r.end + 1] = pee.lm_bits(enc, b, p)
    new = pred + (e2 ^ 1)
    ok = (np.arange(e2.size) <= r.end) & ~lm & (e2 >= -2 * T) & (e2 < 2 * T) & (new >= 0) & (new <= MAXVAL)
    k = int(np.flatnonzero(ok)[0])
    y0, x0, _hc, wc = pee_cpu.lattice_origin(p, *stego.shape)
    return y0 + 2 * (k // wc), x0 + 2 * (k % wc), int(new[k])


@pytest.mark.parametrize("scheme", [1, 2])
def test_clean_decode_verifies(covers, scheme):
    codec, enc = _embed(covers, scheme, checksum=True)
    assert checksum.crc_list(enc.cover_crc) == _zlib(covers)
    assert enc.payload_crc == [checksum.payload_crc32(v) for v in _payloads(scheme)]
    for verify in (True, "require"):
        bits, cover = codec.decode(enc, verify=verify)
        assert np.array_equal(cover.cpu().numpy(), covers)
        assert all(np.array_equal(g, w) for g, w in zip(bits, _payloads(scheme)))
    bits, cover = pee.decode(enc)
    assert np.array_equal(cover.cpu().numpy(), covers)


@pytest.mark.parametrize("scheme", [1, 2])
def test_without_checksum_nothing_is_carried(covers, scheme):
    codec, enc = _embed(covers, scheme)
    assert enc.cover_crc is None and enc.payload_crc is None
    bits, cover = codec.decode(enc)
    assert np.array_equal(cover.cpu().numpy(), covers)
    with pytest.raises(IntegrityError):
        codec.decode(enc, verify="require")


@pytest.mark.parametrize("scheme", [1, 2])
def test_context_pixel_flip_fails_the_cover(covers, scheme):
    codec, enc = _embed(covers, scheme, checksum=True)
    _poke(enc, 0, 0, 0, lambda v: v ^ 1)   # row 0 / column 0 hold no candidate of any lattice
    with pytest.raises(IntegrityError, match="cover"):
        codec.decode(enc)


@pytest.mark.parametrize("scheme", [1, 2])
def test_flipped_payload_bit_fails_the_payload_only(covers, scheme):
    codec, enc = _embed(covers, scheme, checksum=True)
    y, x, new = _expanded_candidate(enc, enc.stego[1].cpu().numpy(), 1)
    _poke(enc, 1, y, x, lambda v: new)
    with pytest.raises(IntegrityError) as ei:
        codec.decode(enc)
    msg = str(ei.value)
    assert "payload checksum mismatch in slices [1]" in msg and "cover" not in msg
    # verify=False: what decode returned before checksums -- the exact cover, one bit flipped
    bits, cover = codec.decode(enc, verify=False)
    assert np.array_equal(cover.cpu().numpy(), covers)
    want = _payloads(scheme)
    assert np.array_equal(bits[0], want[0])
    assert bits[1].size == want[1].size and int((bits[1] != want[1]).sum()) == 1


@pytest.mark.parametrize("scheme", [1, 2])
def test_record_T_changed_fails(covers, scheme):
    codec, enc = _embed(covers, scheme, checksum=True)
    torch = _torch()
    meta = enc.meta.view(-1, enc.meta.shape[-1])
    meta[:, :4] = torch.tensor([3, 0, 0, 0], dtype=torch.uint8, device=meta.device)   # T: 2 -> 3 (little-endian)
    assert {r.T for r in enc.records()} == {3}
    with pytest.raises(IntegrityError):
        codec.decode(enc)


@pytest.mark.parametrize("scheme", [1, 2])
def test_in_place_embed_checksums_the_cover(covers, scheme):
    codec = _codec(scheme)
    buf = _torch().from_numpy(covers).cuda()
    enc = codec.embed(buf, _payloads(scheme), stego=buf, checksum=True)
    assert enc.stego.data_ptr() == buf.data_ptr()
    assert checksum.crc_list(enc.cover_crc) == _zlib(covers)
    bits, cover = codec.decode(enc, verify="require")
    assert np.array_equal(cover.cpu().numpy(), covers)


def test_packed_payloads_carry_no_payload_checksum(covers):
    codec = _codec(1)
    packed = codec.pack_payloads(_payloads(1))
    enc = codec.embed(_torch().from_numpy(covers).cuda(), None, packed=packed, checksum=True)
    assert enc.payload_crc is None and enc.cover_crc is not None
    codec.decode(enc)
    with pytest.raises(IntegrityError, match="payload"):
        codec.decode(enc, verify="require")


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("scheme", [1, 2])
def test_file_round_trip_and_tamper(covers, scheme, tmp_path):
    img, bits = covers[0], _payloads(scheme)[0]
    path = str(tmp_path / "c.bin")
    info = pipeline.encode_file_pee(img, bits, path, T=T, maxval=MAXVAL, scheme=scheme, checksum=True)
    assert info["cover_crc32"] == _zlib(img)[0] and info["payload_crc32"] == checksum.payload_crc32(bits)
    for verify in (True, "require"):
        got, cover = pipeline.decode_bin_pee(path, verify=verify)
        assert np.array_equal(got, bits) and np.array_equal(cover, img)
    raw = bytearray(open(path, "rb").read())
    raw[-1] ^= 1   # the last byte of the raw stego
    bad = str(tmp_path / "bad.bin")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(IntegrityError):
        pipeline.decode_bin_pee(bad)
    pipeline.decode_bin_pee(bad, verify=False)


@pytest.mark.parametrize("scheme", [1, 2])
def test_file_without_the_flag_is_unchanged(covers, scheme, tmp_path):
    img, bits = covers[0], _payloads(scheme)[0]
    plain, summed = str(tmp_path / "p.bin"), str(tmp_path / "s.bin")
    info = pipeline.encode_file_pee(img, bits, plain, T=T, maxval=MAXVAL, scheme=scheme)
    assert "cover_crc32" not in info
    if scheme == 1:   # the default file: create_pee_header's bytes, the map blob, the raw stego -- nothing else
        from codec_tcc_amd import container
        md, blob, data = container.parse_pee_bytes(open(plain, "rb").read())
        hdr = container.create_pee_header("raw", 2, 64, 64, info["T"], info["L"], info["end"], info["maxval"],
                                          info["status"], len(blob))
        assert open(plain, "rb").read() == container.MAGIC + len(hdr).to_bytes(4, "big") + hdr + blob + \
            container.encode_stego_raw(info["stego"])
    pipeline.encode_file_pee(img, bits, summed, T=T, maxval=MAXVAL, scheme=scheme, checksum=True)
    a, b = open(plain, "rb").read(), open(summed, "rb").read()
    assert len(b) == len(a) + 10
    got, cover = pipeline.decode_bin_pee(plain)
    assert np.array_equal(got, bits) and np.array_equal(cover, img)
    with pytest.raises(IntegrityError):
        pipeline.decode_bin_pee(plain, verify="require")
