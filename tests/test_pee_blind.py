"""Blind MED-PEE on the GPU (include/codec_tcc_blind.h), bit-exact against the specification
tests/pee_blind_spec.py: stego and info of embed_blind, bits and cover of decode_blind, on the
cases of DESIGN §3k -- flat-slot (B = 3) and lane-order (B = 9) batches with mixed payload lengths,
W % 8 == 0 and odd widths, uint8; spec-written stegos decoded by the GPU and GPU-written ones by
the spec; refusals; integrity; the DICOM round trip; graph replay."""
import numpy as np
import pytest

import pee_blind_cases as CS
import pee_blind_spec as BS
import pee_covers as PC

pytestmark = pytest.mark.gpu

CASE = {c[0]: c for c in CS.CASES}
# uint8 at a width that is no multiple of 8 (the scalar row pass of uint8); E and r are the spec's
CASE["u8_w100"] = ("u8_w100", 64, 100, "uint8", 2, 2, 60, 2, 2)


def _codec(B, H, W, dtype, T, maxval):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, H, W, dtype=dtype, T=T, maxval=maxval)


def _batch(name, B):
    """(covers [B, H, W], payloads, T, maxval): the case's planted cover, in every slice but the
    first with a dozen pixels of the lower half nudged by one so that the slices differ; mixed
    payload lengths including 0 and the case's."""
    _n, h, w, dtype, T, k, n_user, _E, _r = CASE[name]
    mv = CS.top(dtype)
    covers, bits = [], []
    for b in range(B):
        c = CS.planted(h, w, k, dtype)
        if b:   # distinct slices: a few mid-range pixels nudged outside the planted cells
            rng = np.random.default_rng(70 + b)
            ys, xs = rng.integers(h // 2, max(h // 2 + 1, h - 8), 12), rng.integers(0, w, 12)
            c[ys, xs] = np.clip(c[ys, xs].astype(np.int64) + rng.integers(-1, 2, 12), 0, mv).astype(c.dtype)
        covers.append(c)
        n = (n_user, 0, n_user // 2, 1, n_user - 1)[b % 5] if n_user else 0
        bits.append(CS.payload(max(n, 0), 10 * b + 1))
    return np.stack(covers), bits, T, mv


def _run(name, B, checksum=False):
    torch = pytest.importorskip("torch")
    covers, bits, T, mv = _batch(name, B)
    _b, H, W = covers.shape
    codec = _codec(B, H, W, str(covers.dtype), T, mv)
    cov = torch.from_numpy(covers).cuda()
    stego, info = codec.embed_blind(cov, bits, checksum=checksum)
    got_st, got_info = stego.cpu().numpy(), info.cpu().numpy()
    assert got_info.shape == (B, 6)
    for b in range(B):
        st, want, _p = BS.embed(covers[b], bits[b], T, mv, checksum=checksum)
        assert want[0] == 0, (name, b, want)   # every case here is meant to embed
        assert tuple(int(v) for v in got_info[b]) == tuple(want), (name, b, got_info[b], want)
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"{name}: stego of slice {b}")
    out, back = codec.decode_blind(stego)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    for b in range(B):
        np.testing.assert_array_equal(out[b], bits[b], err_msg=f"{name}: bits of slice {b}")
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)   # the embed left the covers alone
    return codec, covers, bits, stego


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("name", ["smooth", "planted1", "planted3", "wide_t2", "wide_t4", "odd", "u8", "u8_w100"])
def test_gpu_blind_parity(name, B):
    """Stego and info bit for bit the spec's and the exact round trip, flat slots (B = 3) and lane
    order (B = 9), both ROI route families (W % 8 == 0 and the odd 37 x 53) and uint8 on both."""
    _n, _h, _w, _dt, _T, _k, _nu, E, r = CASE[name]
    _codec_, covers, bits, _stego = _run(name, B, checksum=name in ("planted3", "odd", "u8"))
    _st, info, p = BS.embed(covers[0], bits[0], _T, CS.top(_dt))
    assert (info[2], p["r"]) == (E, r)   # the table of DESIGN §3k


def test_gpu_blind_ct12_512():
    """The synthetic CT slice at 512 x 512, T = 2, 1000 bits and none: more than one row band and
    more than one chunk of the look-back pass."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import synth
    covers = np.stack([synth.ct12(512, 512, 300 + i) for i in range(2)])
    bits = [CS.payload(1000, 1), CS.payload(0, 2)]
    codec = _codec(2, 512, 512, "uint16", 2, 4095)
    stego, info = codec.embed_blind(torch.from_numpy(covers).cuda(), bits, checksum=True)
    got = stego.cpu().numpy()
    for b in range(2):
        st, want, _p = BS.embed(covers[b], bits[b], 2, 4095, checksum=True)
        assert want[0] == 0 and tuple(info[b].cpu().tolist()) == tuple(want)
        np.testing.assert_array_equal(got[b], st)
    out, back = codec.decode_blind(stego)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    np.testing.assert_array_equal(out[0], bits[0])
    assert out[1].size == 0
    assert codec.blind_capacity(torch.from_numpy(covers).cuda()).cpu().tolist() == [BS.capacity(c, 2, 4095) for c in covers]


def test_gpu_blind_padding_entry():
    """A planted pixel in row i* behind `end` counts towards E but is no map bit: the header ends
    in a padding entry, on the device as in the spec."""
    torch = pytest.importorskip("torch")
    _n, h, w, dtype, T, k, n_user, _E, _r = CASE["wide_t4"]
    cover, p = CS.with_padding(CS.planted(h, w, k, dtype), n_user, T)
    assert cover is not None
    bits = CS.payload(n_user, 5)
    st, info, _p = BS.embed(cover, bits, T, 4095)
    assert info[0] == 0 and int(BS.read_words(st, BS.HDR_WORDS, info[2])[-1]) == BS.NO_ENTRY
    codec = _codec(1, h, w, dtype, T, 4095)
    stego, ginfo = codec.embed_blind(torch.from_numpy(cover[None]).cuda(), [bits])
    np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
    assert tuple(ginfo.cpu().tolist()[0]) == tuple(info)
    out, back = codec.decode_blind(stego)
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], cover)


@pytest.mark.parametrize("name", ["planted3", "odd", "u8"])
def test_gpu_blind_cross_decode(name):
    """The GPU decodes stegos the spec wrote (built with another T: the header's rules), and the
    spec decodes the GPU's."""
    torch = pytest.importorskip("torch")
    B = 3
    covers, bits, T, mv = _batch(name, B)
    _b, H, W = covers.shape
    spec = np.stack([BS.embed(covers[b], bits[b], T, mv, checksum=True)[0] for b in range(B)])
    other = _codec(B, H, W, str(covers.dtype), T + 3, None)   # decode takes T and maxval from the headers
    out, back = other.decode_blind(torch.from_numpy(spec).cuda())
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    for b in range(B):
        np.testing.assert_array_equal(out[b], bits[b])
    stego, _info = _codec(B, H, W, str(covers.dtype), T, mv).embed_blind(torch.from_numpy(covers).cuda(), bits,
                                                                         checksum=True)
    for b, s in enumerate(stego.cpu().numpy()):
        got, cov, hdr = BS.decode(s)
        np.testing.assert_array_equal(got, bits[b])
        np.testing.assert_array_equal(cov, covers[b])
        assert hdr["flags"] == 1 and hdr["crc"] == BS.cover_crc(covers[b])


def test_gpu_blind_capacity():
    """blind_capacity equals the spec's, and is the boundary: capacity bits embed, one more is refused."""
    torch = pytest.importorskip("torch")
    covers = np.stack([CS.planted(64, 96, 3), CS.smooth(64, 96), PC.cover("checker", 64, 96, "uint16", 4095)])
    codec = _codec(3, 64, 96, "uint16", 4, 4095)
    cov = torch.from_numpy(covers).cuda()
    caps = codec.blind_capacity(cov).cpu().tolist()
    assert caps == [BS.capacity(c, 4, 4095) for c in covers] and caps[2] == -1 and min(caps[:2]) > 0
    assert codec.blind_capacity(cov, max_entries=2).cpu().tolist() == [BS.capacity(c, 4, 4095, 2) for c in covers]
    fit = [CS.payload(max(n, 0), 3) for n in caps]
    _stego, info = codec.embed_blind(cov, fit, check=False)
    assert info[:, 0].cpu().tolist() == [0, 0, 1]
    over = [CS.payload(n + 1, 4) for n in caps]
    _stego, info = codec.embed_blind(cov, over, check=False)
    assert info[:, 0].cpu().tolist() == [1, 1, 1]


def test_gpu_blind_refusals():
    """Slices that do not fit are reported, copied through unchanged, and a batch that holds one
    does not decode; max_entries below E gives status 2."""
    torch = pytest.importorskip("torch")
    covers = np.stack([CS.smooth(64, 96), PC.cover("checker", 64, 96, "uint16", 4095), CS.smooth(64, 96)])
    bits = [CS.payload(500, 1), CS.payload(10, 2), CS.payload(40, 3)]
    codec = _codec(3, 64, 96, "uint16", 2, 4095)
    cov = torch.from_numpy(covers).cuda()
    want = [BS.embed(c, b, 2, 4095) for c, b in zip(covers, bits)]
    assert [w[1][0] for w in want] == [1, 1, 0]
    with pytest.raises(ValueError, match=r"capacity in slices \[0, 1\]"):
        codec.embed_blind(cov, bits)
    stego, info = codec.embed_blind(cov, bits, check=False)
    assert [tuple(r) for r in info.cpu().tolist()] == [tuple(w[1]) for w in want]
    got = stego.cpu().numpy()
    np.testing.assert_array_equal(got[:2], covers[:2])
    np.testing.assert_array_equal(got[2], want[2][0])
    with pytest.raises(ValueError, match=r"header in slices \[0, 1\]"):
        codec.decode_blind(stego)
    # max_entries below E: status 2, in the spec and on the device
    c4 = _codec(1, 64, 96, "uint16", 4, 4095)
    planted = CS.planted(64, 96, 3)
    b100 = [CS.payload(100, 7)]
    assert BS.embed(planted, b100[0], 4, 4095, max_entries=2)[1] == (2, 100, 3, 0, -1, 0)
    with pytest.raises(ValueError, match="max_entries in slices \\[0\\]"):
        c4.embed_blind(torch.from_numpy(planted[None]).cuda(), b100, max_entries=2)
    stego, info = c4.embed_blind(torch.from_numpy(planted[None]).cuda(), b100, max_entries=2, check=False)
    assert tuple(info.cpu().tolist()[0]) == (2, 100, 3, 0, -1, 0)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], planted)
    stego, info = c4.embed_blind(torch.from_numpy(planted[None]).cuda(), b100, max_entries=3)
    assert tuple(info.cpu().tolist()[0]) == BS.embed(planted, b100[0], 4, 4095, max_entries=3)[1]


def _flipped(stego, b, y, x):
    """A copy of the device stack with bit 0 of one pixel flipped."""
    import torch
    host = stego.cpu().numpy().copy()
    host[b, y, x] ^= 1
    return torch.from_numpy(host).cuda()


def test_gpu_blind_integrity():
    """A plain cover: ValueError (no header).  One pixel flipped outside the region under
    checksum=True: IntegrityError for that slice only.  A flipped header bit: ValueError."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import IntegrityError
    codec, covers, bits, stego = _run("planted1", 3, checksum=True)
    with pytest.raises(ValueError, match=r"header in slices \[0, 1, 2\]") as ei:
        codec.decode_blind(torch.from_numpy(covers).cuda())
    assert not isinstance(ei.value, IntegrityError)
    H, W = covers.shape[1:]
    bad = _flipped(stego, 1, 0, 0)   # a context pixel far above the region: the extract still runs, the cover differs
    with pytest.raises(IntegrityError) as ei:
        codec.decode_blind(bad)
    assert ei.value.bad_cover == [1]
    out, back = codec.decode_blind(bad, verify=False)
    for b in (0, 2):
        np.testing.assert_array_equal(out[b], bits[b])
        np.testing.assert_array_equal(back.cpu().numpy()[b], covers[b])
    for bit in (0, 32 + 7, 32 + 9, 2 * 32 + 30, 3 * 32 + 20, 4 * 32 + 30):   # magic, T, flags, n_user, E, end
        bad = _flipped(stego, 2, *divmod(H * W - 1 - bit, W))
        with pytest.raises(ValueError, match=r"header in slices \[2\]") as ei:
            codec.decode_blind(bad)
        assert not isinstance(ei.value, IntegrityError)
    # a flip that leaves a well-formed header (T = 4 -> 12): the extract runs within its bounds and the CRC tells
    bad = _flipped(stego, 2, *divmod(H * W - 1 - (32 + 3), W))
    with pytest.raises(IntegrityError) as ei:
        codec.decode_blind(bad)
    assert ei.value.bad_cover == [2]


def test_gpu_blind_dicom_round_trip(tmp_path):
    """encode_dicom_pee writes a plain DICOM whose pixels are the spec's stego; decode_dicom_pee
    returns payload and cover from the file alone."""
    import golden_io
    from codec_tcc_amd import dicom, framing, pipeline
    img = golden_io.images()["pe"]   # 512 x 512 uint16
    path = str(tmp_path / "blind.dcm")
    res = pipeline.encode_dicom_pee(img, "a blind payload", path, T=2, checksum=True, maxval=4095)
    bits = framing.to_bits("a blind payload")
    st, info, _p = BS.embed(img, bits, 2, 4095, checksum=True)
    assert info[0] == 0 and res["status"] == 0 and res["L"] == bits.size
    pixels, _attrs = dicom.read_dicom(path)
    np.testing.assert_array_equal(pixels, st)
    got, cover = pipeline.decode_dicom_pee(path)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(cover, img)
    plain = str(tmp_path / "plain.dcm")
    dicom.save_dicom(img, plain)
    with pytest.raises(ValueError, match="header"):
        pipeline.decode_dicom_pee(plain)


def test_gpu_blind_top_level():
    """encode_blind / decode_blind beside encode / decode: numpy in, the spec's stego out."""
    import codec_tcc_amd as pkg
    cover = CS.planted(64, 96, 1)
    bits = CS.payload(120, 9)
    stego, info = pkg.encode_blind(cover, [bits], T=4, maxval=4095, checksum=True)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], BS.embed(cover, bits, 4, 4095, checksum=True)[0])
    out, back = pkg.decode_blind(stego.cpu().numpy())
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], cover)


def test_gpu_blind_graph_replay():
    """embed_blind(check=False) with packed= payloads captured once and replayed on refreshed
    covers gives the eager call's stego, which is the spec's."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import graphs
    covers, bits, T, mv = _batch("planted1", 3)
    _b, H, W = covers.shape
    codec = _codec(3, H, W, "uint16", T, mv)
    cov = torch.from_numpy(covers).cuda()
    packed = codec.pack_payloads(bits)
    stego = torch.empty_like(cov)
    keep = {}

    def step():
        keep["out"] = codec.embed_blind(cov, None, stego=stego, packed=packed, checksum=True, check=False)
    g = graphs.capture(step)
    for flip in (0, 1):
        host = covers[::-1].copy() if flip else covers
        pl = bits[::-1] if flip else bits
        cov.copy_(torch.from_numpy(host).cuda())
        words, _lengths, lens_t = codec.pack_payloads(pl)
        packed[0].copy_(words)
        packed[2].copy_(lens_t)
        stego.zero_()
        g.replay()
        torch.cuda.synchronize()
        got, info = stego.cpu().numpy(), keep["out"][1].cpu().tolist()
        for b in range(3):
            st, want, _p = BS.embed(host[b], pl[b], T, mv, checksum=True)
            np.testing.assert_array_equal(got[b], st)
            assert tuple(info[b]) == tuple(want)
