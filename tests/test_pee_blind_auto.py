"""Blind MED-PEE with capacity control on the GPU (include/codec_tcc_blind_auto.h), bit-exact against
the specification tests/pee_blind_auto_spec.py: stego, info, the chosen T and the capacity curve of
embed_blind_auto / blind_capacity_curve on the cases of DESIGN §3l -- flat-slot (B = 3) and
lane-order (B = 9) batches that mix chosen T's and refusals; decode_blind of the result on a codec
built with another T; tmax = 1 and 16; graph replay; the DICOM round trip; the top-level call."""
import numpy as np
import pytest

import pee_blind_auto_cases as AC
import pee_blind_auto_spec as AS
import pee_blind_cases as CS
import pee_blind_spec as BS

pytestmark = pytest.mark.gpu

_spec = {}


def _slice(name, b):
    """(cover, bits, checksum-independent spec results) of slice b of the case's batch: the case's
    lengths in turn; from the second turn on the cover has a dozen pixels of its lower half nudged
    by one, so that the slices of a batch differ.  Built once, shared by B = 3 and B = 9."""
    if (name, b) not in _spec:
        _n, me, lengths = AC.CASE[name]
        img = AC.cover(name)
        mv = CS.top(img.dtype)
        if b >= len(lengths):
            h, w = img.shape
            img = img.copy()
            rng = np.random.default_rng(90 + b)
            ys, xs = rng.integers(h // 2, max(h // 2 + 1, h - 8), 12), rng.integers(0, w, 12)
            img[ys, xs] = np.clip(img[ys, xs].astype(np.int64) + rng.integers(-1, 2, 12), 0, mv).astype(img.dtype)
        bits = AC.payload(lengths[b % len(lengths)][0], 10 * b + 1)
        stego, info, T, _p = AS.embed(img, bits, AC.TMAX, mv, True, me)
        _spec[(name, b)] = (img, bits, stego, info, T, AS.capacity_curve(img, AC.TMAX, mv, me))
    return _spec[(name, b)]


def _codec(B, img, T, tmax=AC.TMAX):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, img.shape[0], img.shape[1], dtype=str(img.dtype), T=T, tmax=tmax, maxval=CS.top(img.dtype))


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("name", [c[0] for c in AC.CASES])
def test_gpu_blind_auto_parity(name, B):
    """Stego, info, chosen T and capacity curve bit for bit the spec's; every refused slice is its
    cover; the embedded ones decode, on a codec built with another T, to payloads and covers."""
    torch = pytest.importorskip("torch")
    _n, me, lengths = AC.CASE[name]
    want = [_slice(name, b) for b in range(B)]
    covers = np.stack([w[0] for w in want])
    for b in range(min(B, len(lengths))):
        assert want[b][4] == lengths[b][1]   # the table of DESIGN §3l
    codec = _codec(B, covers[0], "auto" if B == 3 else 11)
    cov = torch.from_numpy(covers).cuda()
    stego, info, ts = codec.embed_blind_auto(cov, [w[1] for w in want], tmax=AC.TMAX, checksum=True, max_entries=me,
                                             check=False)
    curve = codec.blind_capacity_curve(cov, tmax=AC.TMAX, max_entries=me)
    got_st, got_info, got_ts, got_curve = stego.cpu().numpy(), info.cpu().numpy(), ts.cpu().tolist(), curve.cpu().tolist()
    assert got_info.shape == (B, 6) and len(got_ts) == B
    print(name, B, "T* =", got_ts, "spec", [w[4] for w in want])
    for b, (img, _bits, st, winfo, T, wcurve) in enumerate(want):
        assert got_ts[b] == T, (name, b, got_ts[b], T)
        assert tuple(int(v) for v in got_info[b]) == tuple(winfo), (name, b, got_info[b], winfo)
        assert got_curve[b] == wcurve, (name, b)
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"{name}: stego of slice {b}")
        if T == 0:
            np.testing.assert_array_equal(got_st[b], img)
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)   # the embed left the covers alone
    keep = [b for b in range(B) if want[b][4]]
    if keep:
        other = _codec(len(keep), covers[0], 13)   # decode takes T and maxval from the headers
        out, back = other.decode_blind(torch.from_numpy(got_st[keep]).cuda())
        np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
        for k, b in enumerate(keep):
            np.testing.assert_array_equal(out[k], want[b][1], err_msg=f"{name}: bits of slice {b}")


def test_gpu_blind_auto_tmax_1_is_the_fixed_route():
    """tmax = 1 is embed_blind at T = 1: stego and info, embedded and refused slices alike."""
    torch = pytest.importorskip("torch")
    img = AC.cover("smooth_u8")
    covers = np.stack([img, img, img])
    bits = [AC.payload(200, 1), AC.payload(0, 2), AC.payload(400, 3)]   # capacity 288 at T = 1
    cov = torch.from_numpy(covers).cuda()
    codec = _codec(3, img, 1)
    stego, info, ts = codec.embed_blind_auto(cov, bits, tmax=1, check=False)
    fixed, finfo = codec.embed_blind(cov, bits, check=False)
    assert ts.cpu().tolist() == [1, 1, 0] and info[:, 0].cpu().tolist() == [0, 0, 1]
    np.testing.assert_array_equal(stego.cpu().numpy(), fixed.cpu().numpy())
    assert info.cpu().tolist() == finfo.cpu().tolist()
    np.testing.assert_array_equal(stego.cpu().numpy()[0], BS.embed(img, bits[0], 1, 255)[0])
    assert codec.blind_capacity_curve(cov, tmax=1)[:, 0].cpu().tolist() == codec.blind_capacity(cov).cpu().tolist()


def test_gpu_blind_auto_tmax_16():
    """tmax = 16 chooses what tmax = 8 chooses, and the curve's first eight columns agree."""
    torch = pytest.importorskip("torch")
    img = AC.cover("smooth")
    lengths = [n for n, _t in AC.CASE["smooth"][2]]
    covers = np.stack([img] * len(lengths))
    bits = [AC.payload(n, q + 1) for q, n in enumerate(lengths)]
    cov = torch.from_numpy(covers).cuda()
    codec = _codec(len(lengths), img, 2, tmax=16)
    s16, i16, t16 = codec.embed_blind_auto(cov, bits, check=False)   # tmax=None: the codec's 16
    s8, i8, t8 = codec.embed_blind_auto(cov, bits, tmax=8, check=False)
    want16 = [AS.choose(img, n, 16, 4095)[0] for n in lengths]
    assert t16.cpu().tolist() == want16 and t8.cpu().tolist() == [t for _n, t in AC.CASE["smooth"][2]]
    assert want16[:-1] == t8.cpu().tolist()[:-1] and want16[-1] > 8   # 1200 bits: refused at 8, taken above
    np.testing.assert_array_equal(s16.cpu().numpy()[:-1], s8.cpu().numpy()[:-1])
    assert i16.cpu().tolist()[:-1] == i8.cpu().tolist()[:-1]
    np.testing.assert_array_equal(s16.cpu().numpy()[-1], AS.embed(img, bits[-1], 16, 4095)[0])
    c16 = codec.blind_capacity_curve(cov, tmax=16)
    assert c16.cpu().tolist()[0] == AS.capacity_curve(img, 16, 4095)
    assert c16[:, :8].cpu().tolist()[0] == AS.capacity_curve(img, 8, 4095)
    with pytest.raises(ValueError, match="tmax"):
        codec.embed_blind_auto(cov, bits, tmax=17)
    with pytest.raises(ValueError, match="tmax"):
        codec.blind_capacity_curve(cov, tmax=0)


def test_gpu_blind_auto_refusals_are_named():
    """check=True names the slices no T serves; the fixed-T call still refuses T='auto'."""
    torch = pytest.importorskip("torch")
    img = AC.cover("smooth")
    covers = np.stack([img, img])
    cov = torch.from_numpy(covers).cuda()
    codec = _codec(2, img, "auto")
    with pytest.raises(ValueError, match=r"embed_blind_auto: .*capacity in slices \[1\]"):
        codec.embed_blind_auto(cov, [AC.payload(100, 1), AC.payload(1200, 2)])
    with pytest.raises(ValueError, match="fixed T"):
        codec.embed_blind(cov, [AC.payload(100, 1), AC.payload(100, 2)])
    with pytest.raises(ValueError, match="out of place"):
        codec.embed_blind_auto(cov, [AC.payload(100, 1), AC.payload(100, 2)], stego=cov)


def test_gpu_blind_auto_graph_replay():
    """embed_blind_auto(check=False) with packed= payloads captured once and replayed twice, on
    refreshed covers and lengths, gives the spec's stego, info and T each time."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import graphs
    img = AC.cover("smooth")
    lengths = (100, 500, 1200)
    covers = np.stack([img, AC.cover("planted3"), img])
    bits = [AC.payload(n, q + 1) for q, n in enumerate(lengths)]
    codec = _codec(3, img, 2)
    cov = torch.from_numpy(covers).cuda()
    packed = codec.pack_payloads(bits)
    stego = torch.empty_like(cov)
    keep = {}

    def step():
        keep["out"] = codec.embed_blind_auto(cov, None, stego=stego, packed=packed, checksum=True, check=False)
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
        got, info, ts = stego.cpu().numpy(), keep["out"][1].cpu().tolist(), keep["out"][2].cpu().tolist()
        for b in range(3):
            st, want, T, _p = AS.embed(host[b], pl[b], AC.TMAX, 4095, checksum=True)
            np.testing.assert_array_equal(got[b], st)
            assert tuple(info[b]) == tuple(want) and ts[b] == T


def test_gpu_blind_auto_dicom_round_trip(tmp_path):
    """encode_dicom_pee_auto writes a plain DICOM whose pixels are the spec's stego at the chosen
    T, which the result names; decode_dicom_pee reads the file as it is."""
    import golden_io
    from codec_tcc_amd import dicom, framing, pipeline
    img = golden_io.images()["pe"]   # 512 x 512 uint16
    path = str(tmp_path / "blind_auto.dcm")
    res = pipeline.encode_dicom_pee_auto(img, "a blind payload", path, tmax=8, checksum=True, maxval=4095)
    bits = framing.to_bits("a blind payload")
    st, info, T, _p = AS.embed(img, bits, 8, 4095, checksum=True)
    assert T >= 1 and res["T"] == T and res["status"] == 0 and res["L"] == bits.size
    pixels, _attrs = dicom.read_dicom(path)
    np.testing.assert_array_equal(pixels, st)
    got, cover = pipeline.decode_dicom_pee(path)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(cover, img)


def test_gpu_blind_auto_top_level():
    """encode_blind_auto beside encode_blind: numpy in, the spec's stego out, decode_blind reads it."""
    import codec_tcc_amd as pkg
    cover = AC.cover("planted3").copy()   # writable: the call wraps it in a tensor
    bits = AC.payload(200, 9)
    stego, info, ts = pkg.encode_blind_auto(cover, [bits], tmax=8, maxval=4095, checksum=True)
    st, want, T, _p = AS.embed(cover, bits, 8, 4095, checksum=True)
    assert ts.cpu().tolist() == [T] == [4] and tuple(info.cpu().tolist()[0]) == tuple(want)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
    out, back = pkg.decode_blind(stego.cpu().numpy())
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], cover)
