"""Gated blind MED-PEE on the GPU (include/codec_tcc_blind_gate.h), bit-exact against the specification
tests/pee_blind_gate_spec.py: stego, info, the chosen (T, G) and the capacity curve of embed_blind_gated /
blind_capacity_gated on the cases of DESIGN §3o -- flat-slot (B = 3) and lane-order (B = 9) batches that
mix chosen pairs and refusals; decode_blind(stego) alone; the fixed forms; gated and ungated stegos in
one decode; the checksum; graph replay; the two real images; the DICOM round trip; the top-level call."""
import numpy as np
import pytest

import pee_blind_auto_spec as AS
import pee_blind_cases as CS
import pee_blind_gate_cases as GC
import pee_blind_gate_spec as GS
import pee_blind_spec as BS

pytestmark = pytest.mark.gpu

_spec = {}


def _slice(name, b):
    """(cover, bits, stego, info, T, G, curve) of slice b of the case's batch by the spec, built once
    and shared by B = 3 and B = 9."""
    if (name, b) not in _spec:
        _n, me, _lengths = GC.CASE[name]
        img, bits = GC.batch_slice(name, b)
        mv = CS.top(img.dtype)
        stego, info, T, G, _p = GS.embed(img, bits, GC.TMAX, mv, True, me)
        _spec[(name, b)] = (img, bits, stego, info, T, G, GS.capacity_curve(img, GC.TMAX, mv, me))
    return _spec[(name, b)]


def _codec(B, img, T=2, tmax=16, **kw):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, img.shape[0], img.shape[1], dtype=str(img.dtype), T=T, tmax=tmax, maxval=CS.top(img.dtype), **kw)


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("name", [c[0] for c in GC.CASES])
def test_gpu_blind_gate_parity(name, B):
    """Stego, info, chosen (T, G) and capacity curve bit for bit the spec's; every refused slice is its
    cover; the embedded ones decode, by decode_blind(stego) alone on a codec built with another T, to
    payloads and covers."""
    torch = pytest.importorskip("torch")
    _n, me, lengths = GC.CASE[name]
    want = [_slice(name, b) for b in range(B)]
    covers = np.stack([w[0] for w in want])
    for b in range(min(B, len(lengths))):
        assert (want[b][4], want[b][5]) == lengths[b][1:]   # the table of DESIGN §3o
    codec = _codec(B, covers[0], "auto" if B == 3 else 11, gate=(4 if B == 9 else None))   # its own T and gate are ignored
    cov = torch.from_numpy(covers).cuda()
    stego, info, ts, gs = codec.embed_blind_gated(cov, [w[1] for w in want], tmax=GC.TMAX, checksum=True, max_entries=me,
                                                  check=False)
    curve = codec.blind_capacity_gated(cov, tmax=GC.TMAX, max_entries=me)
    got_st, got_info, got_curve = stego.cpu().numpy(), info.cpu().numpy(), curve.cpu().tolist()
    got_ts, got_gs = ts.cpu().tolist(), gs.cpu().tolist()
    assert got_info.shape == (B, 6) and len(got_ts) == len(got_gs) == B and curve.shape == (B, GC.TMAX, 16)
    print(name, B, "(T*, G*) =", list(zip(got_ts, got_gs)), "spec", [(w[4], w[5]) for w in want])
    for b, (img, _bits, st, winfo, T, G, wcurve) in enumerate(want):
        assert (got_ts[b], got_gs[b]) == (T, G), (name, b, got_ts[b], got_gs[b], T, G)
        assert tuple(int(v) for v in got_info[b]) == tuple(winfo), (name, b, got_info[b], winfo)
        assert got_curve[b] == wcurve, (name, b)
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"{name}: stego of slice {b}")
        if T == 0:
            np.testing.assert_array_equal(got_st[b], img)
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)   # the embed left the covers alone
    keep = [b for b in range(B) if want[b][4]]
    if keep:
        other = _codec(len(keep), covers[0], 13)   # decode takes T, maxval and the gate from the headers
        out, back = other.decode_blind(torch.from_numpy(got_st[keep]).cuda())
        np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
        for k, b in enumerate(keep):
            np.testing.assert_array_equal(out[k], want[b][1], err_msg=f"{name}: bits of slice {b}")


def test_gpu_blind_gate_fixed_forms():
    """T=, gate= and both on the 64 x 96 cases: the spec's pair, stego and info, refusals included."""
    torch = pytest.importorskip("torch")
    for name in sorted({f[0] for f in GC.FIXED}):
        rows = [f for f in GC.FIXED if f[0] == name]
        img = GC.cover(name)
        mv = CS.top(img.dtype)
        codec = _codec(1, img)
        cov = torch.from_numpy(img[None].copy()).cuda()
        for _nm, n, T, gate, want in rows:
            bits = GC.payload(n, 3)
            st, winfo, t, g, _p = GS.embed(img, bits, GC.TMAX, mv, True, 256, T=T, gate=gate)
            assert (t, g) == want
            stego, info, ts, gs = codec.embed_blind_gated(cov, [bits], tmax=GC.TMAX, T=T, gate="auto" if gate is None else gate,
                                                          checksum=True, check=False)
            assert (ts.cpu().tolist(), gs.cpu().tolist()) == ([t], [g]), (name, n, T, gate)
            assert tuple(info.cpu().tolist()[0]) == tuple(winfo)
            np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
            if t:
                out, back = codec.decode_blind(stego)
                np.testing.assert_array_equal(out[0], bits)
                np.testing.assert_array_equal(back.cpu().numpy()[0], img)
    with pytest.raises(ValueError, match="ladder"):
        codec.embed_blind_gated(cov, [bits], gate=5)
    with pytest.raises(ValueError, match="1..tmax"):
        codec.embed_blind_gated(cov, [bits], T=5)   # the default tmax is 4
    with pytest.raises(ValueError, match="out of place"):
        codec.embed_blind_gated(cov, [bits], stego=cov)
    with pytest.raises(ValueError, match=r"embed_blind_gated: .*capacity in slices \[0\]"):
        codec.embed_blind_gated(cov, [GC.payload(5000, 1)])


def test_gpu_blind_gate_mixed_decode_and_spec_stego():
    """One decode_blind call over embed_blind, embed_blind_auto and gated stegos, and over a stego the
    spec made: each slice is read by its own header."""
    torch = pytest.importorskip("torch")
    img = GC.cover("half_u16")
    bits = [GC.payload(n, q + 1) for q, n in enumerate((30, 127, 127, 303))]
    one = torch.from_numpy(img[None].copy()).cuda()
    codec = _codec(1, img, 8)
    s_fixed, _i = codec.embed_blind(one, [bits[0]], checksum=True)
    s_auto, _i, t_auto = codec.embed_blind_auto(one, [bits[1]], tmax=8)
    s_gate, _i, t_gate, g_gate = codec.embed_blind_gated(one, [bits[2]], tmax=8, checksum=True)
    assert t_auto.cpu().tolist() == [5] and (t_gate.cpu().tolist(), g_gate.cpu().tolist()) == ([5], [12])
    s_spec = GS.embed(img, bits[3], 8, 4095)[0]   # (7, 16), made on the host
    stack = torch.cat([s_fixed, s_auto, s_gate, torch.from_numpy(s_spec[None]).cuda()])
    out, back = _codec(4, img, 3).decode_blind(stack)
    for b in range(4):
        np.testing.assert_array_equal(out[b], bits[b])
        np.testing.assert_array_equal(back.cpu().numpy()[b], img)


def test_gpu_blind_gate_checksum_detects_a_flipped_pixel():
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import IntegrityError
    img = GC.cover("half_u8")
    codec = _codec(1, img)
    stego, _info, ts, gs = codec.embed_blind_gated(torch.from_numpy(img[None].copy()).cuda(), [GC.payload(276, 1)], tmax=8,
                                                   checksum=True)
    assert (ts.cpu().tolist(), gs.cpu().tolist()) == ([2], [32])
    bad = stego.clone()
    bad[0, 10, 10] ^= 2   # an even pixel above the region: no candidate, context of one
    with pytest.raises(IntegrityError):
        codec.decode_blind(bad)
    out, _back = codec.decode_blind(bad, verify=False)
    assert len(out[0]) == 276


def test_gpu_blind_gate_graph_replay():
    """embed_blind_gated(check=False) with packed= payloads captured once and replayed twice, on
    refreshed covers and lengths, gives the spec's stego, info and pair each time: no choice sticks."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import graphs
    lengths = (127, 100, 488)
    covers = np.stack([GC.cover("half_u16"), GC.cover("planted_mix"), GC.cover("half_u16")])
    bits = [GC.payload(n, q + 1) for q, n in enumerate(lengths)]
    codec = _codec(3, covers[0])
    cov = torch.from_numpy(covers).cuda()
    packed = codec.pack_payloads(bits)
    stego = torch.empty_like(cov)
    keep = {}

    def step():
        keep["out"] = codec.embed_blind_gated(cov, None, tmax=GC.TMAX, stego=stego, packed=packed, checksum=True, check=False)
    g = graphs.capture(step)
    seen = []
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
        ts, gs = keep["out"][2].cpu().tolist(), keep["out"][3].cpu().tolist()
        for b in range(3):
            st, want, T, G, _p = GS.embed(host[b], pl[b], GC.TMAX, 4095, checksum=True)
            np.testing.assert_array_equal(got[b], st)
            assert tuple(info[b]) == tuple(want) and (ts[b], gs[b]) == (T, G)
        seen.append(list(zip(ts, gs)))
    assert seen == [[(5, 12), (5, 128), (0, -1)], [(0, -1), (5, 128), (5, 12)]]


# ---------------------------------------------------------------- the two real images
def _images():
    import golden_io
    return golden_io.images()


@pytest.mark.parametrize("n,floor", [(4096, 3.0), (8192, 3.0), (16384, 3.0)])
def test_gpu_blind_gate_quality_on_pe(n, floor):
    """pe (512 x 512, 12 bits): the GPU's gated stego is the spec's, and through quality.quality its
    PSNR is at least 3.0 dB above embed_blind_auto's at tmax 8 (the spec's own figures: DESIGN §3o)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import quality
    img = _images()["pe"]
    bits = GS.RS.payload_bits(n, 1)
    codec = _codec(1, img)
    cov = torch.from_numpy(img[None].copy()).cuda()
    s_gate, _i, ts, gs = codec.embed_blind_gated(cov, [bits], tmax=8)
    s_auto, _i2, ta = codec.embed_blind_auto(cov, [bits], tmax=8)
    st, _info, T, G, _p = GS.embed(img, bits, 8, 4095)
    np.testing.assert_array_equal(s_gate.cpu().numpy()[0], st)
    np.testing.assert_array_equal(s_auto.cpu().numpy()[0], AS.embed(img, bits, 8, 4095)[0])
    assert (ts.cpu().tolist(), gs.cpu().tolist()) == ([T], [G]) and G < 65535
    p_gate = quality.quality(cov, s_gate, 4095)[0]["psnr"]   # at the image's full scale
    p_auto = quality.quality(cov, s_auto, 4095)[0]["psnr"]
    print(f"pe {n} bits: gated (T={T}, G={G}) {p_gate:.2f} dB, auto T={ta.cpu().tolist()[0]} {p_auto:.2f} dB, "
          f"gain {p_gate - p_auto:.2f} dB")
    assert p_gate - p_auto >= floor
    out, back = codec.decode_blind(s_gate)
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], img)


def test_gpu_blind_gate_torax_takes_what_auto_refuses():
    """torax (512 x 512, 8 bits) at 8192 bits, tmax 8, max_entries 256: embed_blind_auto refuses, the
    gated call embeds the spec's stego and round-trips."""
    torch = pytest.importorskip("torch")
    img = _images()["torax"]
    bits = GS.RS.payload_bits(8192, 2)
    codec = _codec(1, img)
    cov = torch.from_numpy(img[None].copy()).cuda()
    _s, info_a, ta = codec.embed_blind_auto(cov, [bits], tmax=8, max_entries=256, check=False)
    assert ta.cpu().tolist() == [0] and info_a.cpu().tolist()[0][0] != 0
    stego, info, ts, gs = codec.embed_blind_gated(cov, [bits], tmax=8, max_entries=256)
    st, winfo, T, G, _p = GS.embed(img, bits, 8, 255)
    assert (ts.cpu().tolist(), gs.cpu().tolist()) == ([T], [G]) == ([1], [0])
    assert tuple(info.cpu().tolist()[0]) == tuple(winfo)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
    out, back = codec.decode_blind(stego)
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], img)


def test_gpu_blind_gate_dicom_round_trip(tmp_path):
    """encode_dicom_pee_gated writes a plain DICOM whose pixels are the spec's stego at the chosen
    pair, which the result names; decode_dicom_pee reads the file unchanged."""
    from codec_tcc_amd import dicom, framing, pipeline
    img = _images()["pe"]
    path = str(tmp_path / "blind_gate.dcm")
    res = pipeline.encode_dicom_pee_gated(img, "a gated blind payload", path, tmax=8, checksum=True, maxval=4095)
    bits = framing.to_bits("a gated blind payload")
    st, _info, T, G, _p = GS.embed(img, bits, 8, 4095, checksum=True)
    assert T >= 1 and (res["T"], res["G"]) == (T, G) and res["status"] == 0 and res["L"] == bits.size
    pixels, _attrs = dicom.read_dicom(path)
    np.testing.assert_array_equal(pixels, st)
    got, cover = pipeline.decode_dicom_pee(path)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(cover, img)


def test_gpu_blind_gate_top_level():
    """encode_blind_gated beside encode_blind_auto: numpy in, the spec's stego out, decode_blind reads it."""
    import codec_tcc_amd as pkg
    cover = GC.cover("planted_mix").copy()   # writable: the call wraps it in a tensor
    bits = GC.payload(100, 9)
    stego, info, ts, gs = pkg.encode_blind_gated(cover, [bits], tmax=8, maxval=4095, checksum=True)
    st, want, T, G, _p = GS.embed(cover, bits, 8, 4095, checksum=True)
    assert (ts.cpu().tolist(), gs.cpu().tolist()) == ([T], [G]) == ([5], [128])
    assert tuple(info.cpu().tolist()[0]) == tuple(want)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], st)
    out, back = pkg.decode_blind(stego.cpu().numpy())
    np.testing.assert_array_equal(out[0], bits)
    np.testing.assert_array_equal(back.cpu().numpy()[0], cover)
