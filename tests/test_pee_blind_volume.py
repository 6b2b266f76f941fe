"""Blind volume payloads on the GPU (include/codec_tcc_blind_vol.h), bit-exact against the
specification tests/pee_blind_volume_spec.py: stego, plan info, per-slice info, T and frames of
embed_blind_volume on the stacks of tests/pee_blind_volume_cases.py; decode_blind_volume of the
result on a codec built with another T, in permuted order, with unmarked slices among the carriers,
with a carrier dropped; the refusals; more slices than a workgroup has threads; shares longer than one
block; the default dispatch at B = CU count; graph replay."""
import numpy as np
import pytest

import pee_blind_volume_cases as VC
import pee_blind_volume_spec as VS

pytestmark = pytest.mark.gpu


def _codec(B, img, T=2, tmax=8, maxval=None):
    from codec_tcc_amd.pee import PeeCodec
    mv = maxval if maxval is not None else (4095 if img.dtype == np.uint16 else 255)
    return PeeCodec(B, img.shape[-2], img.shape[-1], dtype=str(img.dtype), T=T, tmax=tmax, maxval=mv)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _check_embed(out, want, covers):
    """stego, plan info, n, off, frames, per-slice info and T against a spec result"""
    stego, info, ts = out
    p = want["plan"]
    v = info["volume"].cpu().tolist()
    B = covers.shape[0]
    assert v == [p["status"], p["T"], p["capacity"], p["capacity_max"], p["carriers"], p["N"], VS.VS.POLICIES.index(p["policy"]),
                 B], (v, p)
    assert info["n"].cpu().tolist() == p["n"].tolist() and info["off"].cpu().tolist() == p["off"].tolist()
    assert ts.cpu().tolist() == want["ts"], (ts.cpu().tolist(), want["ts"])
    got_frames = (info["frames"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    assert got_frames == [[int(x) for x in f] for f in want["frames"]]
    got_info = info["slices"].cpu().numpy()
    for b in range(B):
        assert tuple(int(x) for x in got_info[b]) == tuple(want["info"][b]), (b, got_info[b], want["info"][b])
    got = stego.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], want["stego"][b], err_msg=f"stego of slice {b}")
    return got


@pytest.mark.parametrize("policy", VC.POLICIES)
@pytest.mark.parametrize("B", VC.BATCHES)
@pytest.mark.parametrize("shape", list(VC.SHAPES))
def test_gpu_blind_volume_parity(shape, B, policy):
    """every length of the case: the embed bit for bit the spec's; a refused volume is its covers; a
    planned one decodes, reversed, on a codec built with another T, to the stream and the covers"""
    pytest.importorskip("torch")
    covers = VC.stack(shape, B)
    _h, _w, _dt, mv, tmax = VC.SHAPES[shape]
    cov = _gpu(covers)
    codec = _codec(B, covers, T="auto" if B == 3 else 11, tmax=16, maxval=mv)
    for which in VC.LENGTH_NAMES:
        want = VC.result(shape, B, policy, which)
        bits = VC.bits(shape, B, which)
        out = codec.embed_blind_volume(cov, bits, volume_id=VC.VOLUME_ID, policy=policy, tmax=tmax, checksum=True, check=False)
        got = _check_embed(out, want, covers)
        print(shape, B, policy, which, "N =", bits.size, "T* =", want["plan"]["T"], "n =", want["plan"]["n"].tolist(),
              "ts =", want["ts"])
        if which == "over":
            assert want["plan"]["status"] == 1
            np.testing.assert_array_equal(got, covers)
            with pytest.raises(ValueError, match=rf"N = {bits.size} .*S\(tmax\) = {bits.size - 1}"):
                codec.embed_blind_volume(cov, bits, volume_id=1, policy=policy, tmax=tmax)
            continue
        other = _codec(B, covers, T=13, maxval=mv)
        back_bits, back = other.decode_blind_volume(_gpu(got[::-1]))
        np.testing.assert_array_equal(back_bits, bits)
        np.testing.assert_array_equal(back.cpu().numpy(), covers[::-1])
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)   # the embeds left the covers alone


@pytest.fixture(scope="module")
def embedded():
    """(covers, bits, stego on the host) of the u16, B = 9, even, two-thirds-of-capacity case with checksums"""
    pytest.importorskip("torch")
    covers, bits = VC.stack("u16", 9), VC.bits("u16", 9, "most")
    codec = _codec(9, covers)
    stego, info, _ts = codec.embed_blind_volume(_gpu(covers), bits, volume_id=VC.VOLUME_ID, tmax=8, checksum=True)
    want = VC.result("u16", 9, "even", "most")
    got = stego.cpu().numpy()
    np.testing.assert_array_equal(got, want["stego"])
    return covers, bits, got, want


def test_gpu_blind_volume_order_free_decode(embedded):
    covers, bits, stego, want = embedded
    perm = [4, 8, 0, 7, 1, 3, 6, 2, 5]
    got, back = _codec(9, covers, T=5).decode_blind_volume(_gpu(stego[perm]))
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[perm])
    # unmarked slices appended: tolerated, returned as they are
    extra = np.concatenate([stego[perm], VS.stack(3, 64, 96, seed=700)])
    got, back = _codec(12, covers).decode_blind_volume(_gpu(extra))
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back.cpu().numpy()[9:], extra[9:])
    np.testing.assert_array_equal(back.cpu().numpy()[:9], covers[perm])


def test_gpu_blind_volume_dropped_carrier(embedded):
    covers, bits, stego, want = embedded
    p = want["plan"]
    drop = 3
    lo, hi = int(p["off"][drop]), int(p["off"][drop] + p["n"][drop])
    assert hi > lo
    keep = [b for b in range(9) if b != drop][::-1]
    codec = _codec(8, covers)
    with pytest.raises(ValueError, match=rf"missing stream bits \[\({lo}, {hi}\)\] of {bits.size}"):
        codec.decode_blind_volume(_gpu(stego[keep]))
    got, back, missing = codec.decode_blind_volume(_gpu(stego[keep]), partial=True)
    assert missing == [(lo, hi)] == VS.decode(stego[keep], partial=True)[2]["missing"]
    exp = bits.copy()
    exp[lo:hi] = 0
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
    # the last carrier dropped: the stream keeps its full length
    last = max(b for b in range(9) if p["n"][b] > 0)
    keep = [b for b in range(9) if b != last]
    got, _back, missing = codec.decode_blind_volume(_gpu(stego[keep]), partial=True)
    assert missing == [(int(p["off"][last]), bits.size)] and got.size == bits.size
    assert not got[int(p["off"][last]):].any()
    np.testing.assert_array_equal(got[:int(p["off"][last])], bits[:int(p["off"][last])])


def test_gpu_blind_volume_decode_refusals(embedded):
    from codec_tcc_amd import IntegrityError
    covers, bits, stego, want = embedded
    codec = _codec(9, covers)
    cov = _gpu(covers)
    # two volumes mixed
    other, _i, _t = codec.embed_blind_volume(cov, bits, volume_id=VC.VOLUME_ID + 1, tmax=8, checksum=True)
    mixed = stego.copy()
    mixed[4] = other.cpu().numpy()[4]
    with pytest.raises(ValueError, match="different volumes"):
        codec.decode_blind_volume(_gpu(mixed))
    # a duplicated carrier (in the place of another carrier)
    dup = stego.copy()
    dup[4] = stego[3]
    with pytest.raises(ValueError, match="duplicated"):
        codec.decode_blind_volume(_gpu(dup))
    # a plain blind slice among them
    plain, _info = codec.__class__(1, 64, 96, dtype="uint16", T=4, maxval=4095).embed_blind(cov[:1], [bits[:100]])
    bad = stego.copy()
    bad[1] = plain.cpu().numpy()[0]
    with pytest.raises(ValueError, match=r"flags = 0x0"):
        codec.decode_blind_volume(_gpu(bad))
    # decode_blind keeps refusing the flag it does not know
    with pytest.raises(ValueError, match="flags = 0x5"):
        _codec(1, covers).decode_blind(_gpu(stego[:1]))
    # no carrier at all
    with pytest.raises(ValueError, match="no slice carries"):
        codec.decode_blind_volume(cov)
    # one flipped stego pixel inside a share's embedding region
    hit = stego.copy()
    hit[0, 3, 5] ^= 1
    with pytest.raises(IntegrityError):
        codec.decode_blind_volume(_gpu(hit))
    got, _back = codec.decode_blind_volume(_gpu(hit), verify=False)
    assert got.size == bits.size


def test_gpu_blind_volume_embed_refusals():
    """ValueError before any launch"""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    from pee_launches import launches
    covers = VC.stack("u16", 3)
    cov = _gpu(covers)
    bits = VC.bits("u16", 3, "most")
    seen = set()
    with launches(seen):
        for codec, kw, text in ((PeeCodec(3, 64, 96, T=2, maxval=4095, gate=8), {}, "gate"),
                                (PeeCodec(3, 64, 96, T=2, maxval=4095, scheme=2), {}, "scheme 1"),
                                (_codec(3, covers), {"stego": cov}, "out of place"),
                                (_codec(3, covers), {"policy": "odd"}, "policy"),
                                (_codec(3, covers), {"tmax": 17}, "tmax"),
                                (_codec(3, covers), {"volume_id": -1}, "volume_id")):
            with pytest.raises(ValueError, match=text):
                codec.embed_blind_volume(cov, bits, **kw)
        with pytest.raises(ValueError, match="1 .. 2\\^31 - 1"):
            _codec(3, covers).embed_blind_volume(cov, np.zeros(0, np.uint8))
        with pytest.raises(ValueError, match="key"):
            _codec(3, covers).embed_blind_volume(cov, bits, key=b"k" * 32)
    assert seen == set()
    from codec_tcc_amd import blind_volume
    with pytest.raises(ValueError, match="65535"):
        blind_volume.check_args(scheme=1, tmax=8, gate=None, B=65536, H=8, W=32, maxval=255, nbits=5)
    with pytest.raises(ValueError, match="key"):
        blind_volume.check_args(scheme=1, tmax=8, gate=None, B=3, H=64, W=96, maxval=255, nbits=5, key=b"k" * 32)


def test_gpu_blind_volume_many_slices():
    """1100 slices (the plan's scan, the slot table and the order's running maximum take a second round
    of 1024): plan, T and stego of sampled slices against the spec; decode in reversed order"""
    pytest.importorskip("torch")
    covers = VC.many_stack()
    B = covers.shape[0]
    cur = VS.curves(covers, 5, 4095)
    c = VS.transform(cur)
    N = int(c[:, 4].sum()) - 777           # T* = tmax = 5: all but the checkerboards carry
    p = VS.plan(cur, N, "even")
    skipped = np.flatnonzero(p["n"] == 0)
    assert p["status"] == 0 and p["T"] == 5 and p["carriers"] >= 1025 and skipped.size >= 1 and (skipped > 1024).any()
    bits = VS.stream_bits(N, 99)
    codec = _codec(B, covers, tmax=5)
    cov = _gpu(covers)
    stego, info, ts = codec.embed_blind_volume(cov, bits, volume_id=7, tmax=5, check=False)
    assert info["volume"].cpu().tolist() == [0, 5, p["capacity"], p["capacity_max"], p["carriers"], N, 0, B]
    assert info["n"].cpu().tolist() == p["n"].tolist() and info["off"].cpu().tolist() == p["off"].tolist()
    got, got_ts = stego.cpu().numpy(), ts.cpu().tolist()
    np.testing.assert_array_equal(got[skipped], covers[skipped])
    for b in (0, 5, 1023, 1024, 1025, B - 1):   # both rounds; slice 5 is a checkerboard
        nb, ob = int(p["n"][b]), int(p["off"][b])
        if nb == 0:
            assert got_ts[b] == 0
            continue
        user = np.concatenate([VS.BS.words_to_bits(VS.frame(7, b, B, ob, N, None)), bits[ob:ob + nb]])
        st, _i, T, _p = VS.AS.embed(covers[b], user, 5, 4095)
        VS.set_volume_flag(st)
        assert got_ts[b] == T
        np.testing.assert_array_equal(got[b], st, err_msg=f"slice {b}")
    back_bits, back = codec.decode_blind_volume(_gpu(got[::-1]))
    np.testing.assert_array_equal(back_bits, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[::-1])
    # the carrier of index 1030 dropped: the gap is found past the first round of slots
    b = next(k for k in range(1030, B) if p["n"][k] > 0)
    keep = [k for k in range(B) if k != b]
    _bits, _back, missing = _codec(B - 1, covers, tmax=5).decode_blind_volume(_gpu(got[keep]), partial=True)
    assert missing == [(int(p["off"][b]), int(p["off"][b] + p["n"][b]))]


def test_gpu_blind_volume_long_shares():
    """2 x 512 x 512: a share of more than 16384 bits (more than one block of the ROI embed)"""
    pytest.importorskip("torch")
    covers = VC.long_stack()
    cur = VS.curves(covers, 4, 4095)
    N = int(VS.transform(cur)[:, 1].sum()) - 100   # T* = 2
    bits = VS.stream_bits(N, 5)
    want = VS.embed(covers, bits, volume_id=9, policy="fill", tmax=4, maxval=4095, checksum=True)
    assert want["plan"]["status"] == 0 and max(want["plan"]["n"]) > 16384 and want["plan"]["carriers"] == 2
    codec = _codec(2, covers, tmax=4)
    out = codec.embed_blind_volume(_gpu(covers), bits, volume_id=9, policy="fill", tmax=4, checksum=True)
    got = _check_embed(out, want, covers)
    back_bits, back = codec.decode_blind_volume(_gpu(got[::-1]))
    np.testing.assert_array_equal(back_bits, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[::-1])


def test_gpu_blind_volume_default_dispatch_at_cu_count():
    """B = CU count of 67 x 264 slices (tests/pee_batch_cases.py's blind covers), no knob set: the launch
    families recorded, the plan against the spec's, sampled stegos, the round trip"""
    pytest.importorskip("torch")
    import pee_batch_cases as BC
    from pee_launches import launches
    B = BC.ncu()
    if B > BC.MAX_NCU:
        pytest.skip(f"{B} CUs: the case is sized for a few hundred slices")
    covers = np.stack([BC.blind_cover(b) for b in range(B)])
    cur = VS.curves(covers, BC.TMAX, 4095, BC.BLIND_ME)
    N = int(VS.transform(cur)[:, 3].sum()) - 5000   # T* = 4 of 8
    p = VS.plan(cur, N, "even")
    assert p["status"] == 0 and p["T"] == 4
    bits = VS.stream_bits(N, 3)
    codec = _codec(B, covers, T=11, maxval=4095)
    cov = _gpu(covers)
    seen = set()
    with launches(seen):
        stego, info, ts = codec.embed_blind_volume(cov, bits, volume_id=11, tmax=BC.TMAX, checksum=True,
                                                   max_entries=BC.BLIND_ME, check=False)
    assert seen == {"k_blind_rows_auto", "k_bvol_plan", "k_bvol_rows", "k_pee_embed1", "k_crc32", "k_crc32_combine"}, seen
    assert info["n"].cpu().tolist() == p["n"].tolist() and info["off"].cpu().tolist() == p["off"].tolist()
    got, got_ts = stego.cpu().numpy(), ts.cpu().tolist()
    crc = VS.stream_crc(bits)
    for b in (0, 4, 10, B // 2, B - 1):   # plain, planted, bright, middle, last
        nb, ob = int(p["n"][b]), int(p["off"][b])
        user = np.concatenate([VS.BS.words_to_bits(VS.frame(11, b, B, ob, N, crc)), bits[ob:ob + nb]])
        st, _i, T, _p = VS.AS.embed(covers[b], user, BC.TMAX, 4095, True, BC.BLIND_ME)
        VS.set_volume_flag(st)
        assert got_ts[b] == T and T != 0
        np.testing.assert_array_equal(got[b], st, err_msg=f"slice {b}")
    seen = set()
    with launches(seen):
        back_bits, back = codec.decode_blind_volume(_gpu(got[::-1]))
    assert seen == {"k_pee_extract1", "k_bvol_order", "k_bvol_gather", "k_crc32", "k_crc32_combine"}, seen
    np.testing.assert_array_equal(back_bits, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[::-1])


def test_gpu_blind_volume_graph_replay():
    """embed_blind_volume(check=False, packed=) captured once and replayed on refreshed covers and
    stream gives the eager result and the spec's"""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing, graphs
    covers = VC.stack("u16", 9)
    bits = VC.bits("u16", 9, "most")
    codec = _codec(9, covers)
    cov = _gpu(covers)
    words = torch.from_numpy(framing.pack_bits([bits])[0].reshape(-1)).cuda()
    stego = torch.empty_like(cov)
    keep = {}

    def step():
        keep["out"] = codec.embed_blind_volume(cov, None, volume_id=VC.VOLUME_ID, tmax=8, stego=stego, check=False,
                                               packed=(words, bits.size))
    g = graphs.capture(step)
    for flip in (0, 1):
        host = covers[::-1].copy() if flip else covers
        pl = bits[::-1].copy() if flip else bits
        cov.copy_(_gpu(host))
        words.copy_(torch.from_numpy(framing.pack_bits([pl])[0].reshape(-1)).cuda())
        stego.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = VS.embed(host, pl, volume_id=VC.VOLUME_ID, tmax=8, maxval=4095)
        _check_embed((stego, keep["out"][1], keep["out"][2]), want, host)
        eager = codec.embed_blind_volume(cov, pl, volume_id=VC.VOLUME_ID, tmax=8, check=False)[0]
        assert torch.equal(eager, stego)


def test_gpu_blind_volume_dicom_series(tmp_path):
    """encode_dicom_series_pee writes one plain DICOM per slice whose pixels are the spec's stegos;
    decode_dicom_series_pee reads them back in another order"""
    from codec_tcc_amd import dicom, pipeline
    covers = np.array(VC.stack("u16", 3))
    bits = VC.bits("u16", 3, "most")
    res = pipeline.encode_dicom_series_pee(list(covers), bits, str(tmp_path / "series"), tmax=8, maxval=4095,
                                           volume_id=VC.VOLUME_ID)
    want = VC.result("u16", 3, "even", "most")
    assert res["T"] == want["plan"]["T"] and res["n"] == want["plan"]["n"].tolist() and res["ts"] == want["ts"]
    for b, path in enumerate(res["paths"]):
        np.testing.assert_array_equal(dicom.read_dicom(path)[0], want["stego"][b])
    order = [2, 0, 1]
    got, back = pipeline.decode_dicom_series_pee([res["paths"][k] for k in order])
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back, covers[order])
    with pytest.raises(ValueError, match="missing stream bits"):
        pipeline.decode_dicom_series_pee(res["paths"][:2])


def test_gpu_blind_volume_top_level():
    import codec_tcc_amd as pkg
    covers = np.array(VC.stack("u8", 3))
    bits = VC.bits("u8", 3, "most")
    stego, info, ts = pkg.encode_blind_volume(covers, bits, volume_id=VC.VOLUME_ID, tmax=8, checksum=True)
    np.testing.assert_array_equal(stego.cpu().numpy(), VC.result("u8", 3, "even", "most")["stego"])
    got, back = pkg.decode_blind_volume(stego.cpu().numpy()[::-1].copy())
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers[::-1])
    with pytest.raises(ValueError, match="S\\(tmax\\)"):
        pkg.encode_blind_volume(covers, VC.bits("u8", 3, "over"), tmax=8)
