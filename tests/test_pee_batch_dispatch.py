"""Every MED-PEE feature at the batch sizes where codec_pee.hip's dispatch changes route, with no
knob set: what a user's batch of a few hundred slices runs.

The cases are tests/pee_batch_cases.py's (tests/test_pee_batch_cases_host.py checks their
conditions on the CPU): 67 x 264 slices, two look-back chunks each, all different, payload
lengths of period 7 and per-slice T / G / rectangles of period 5 against the lanes' 8 and the slot
groups' 32.  Every test compares EVERY slice bit for bit with the feature's specification,
round-trips every slice, and asserts the launch families recorded around its calls
(tests/pee_launches.py).  The expected families were written down from the dispatch's text
before the first run; they are the "route by batch size" table of DESIGN.md.

  batch       below = CUs - 1      fills = CUs      ragged = CUs + 9     two_rounds = ceil(1.7 CUs)
  ungated     look-back            slice-serial     look-back            slice-serial
  gated, ROI, blind: the look-back at every size -- they have no slice-serial route

  family                              batches               specification
  scheme 1 fixed T, oop / in place    all four              oracle/pee_cpu.py
  scheme 1 T="auto"                   fills, ragged         pee_cpu.select_T + pee_embed(truncate)
  scheme 2 fixed T and T="auto"       fills, ragged         pee_cpu.pee_embed_multi (test_pee2_auto.py's
                                                            chip-filling test samples 8 of its 256 slices)
  checksum=True / "tiles"             ragged                zlib, tests/tile_crc_spec.py
  embed(key=), index0 = 2^31 - B      fills, ragged         tests/aead_spec.py
  gate fixed (T, G); gate="auto"      fills, ragged         tests/pee_gate_spec.py
  ROI, roi.roi_bbox                   fills, ragged         tests/pee_roi_spec.py
  volumes even / fill / gate / key    fills, ragged         tests/pee_volume_spec.py, pee_gvol_spec.py
  blind fixed T / auto                fills, ragged         tests/pee_blind_spec.py, pee_blind_auto_spec.py
  keyed blind                         ragged                tests/pee_blind_keyed_spec.py
  quality.moments                     ragged                oracle/quality_cpu.py
  gated in place, 258 x 512           ragged                the in-place look-back's persistent grid wraps
"""
import copy
import zlib

import numpy as np
import pytest

import pee_batch_cases as BC
import tile_crc_spec as TS
from oracle import pee_cpu as P
from oracle import quality_cpu as O
from pee_launches import launches
from test_pee import _check_multi_vs_oracle
from test_pee2_auto import _check_auto_vs_spec, _check_round_trip
from test_pee_gate import _check_enc as gate_check_enc, _round_trip as gate_round_trip
from test_pee_gvol import _check_gvol
from test_pee_launch_variants import _run_scheme1
from test_pee_roi import _round_trip as roi_round_trip
from test_pee_volume import _check_volume

pytestmark = pytest.mark.gpu

H, W = BC.H, BC.W
ALL = ("below", "fills", "ragged", "two_rounds")
TWO = ("fills", "ragged")

# ---- the launch families, from reading the dispatch (codec_pee.hip: pee_embed_t, pee_extract_t,
# codec_pee_embed_auto, codec_pee_multi_*; the feature units' host code)
LB = {"k_pee_embed1", "k_pee_extract1"}
SS = {"k_pee_embed_ss", "k_pee_extract_ss"}
SERIAL = {"below": False, "fills": True, "ragged": False, "two_rounds": True}   # pee_fills_chip
FIXED = {name: SS if s else LB for name, s in SERIAL.items()}
# T="auto": fused into one slice-serial launch where the batch fills the chip and the pixels are
# uint16_t (resident out of place, the AUTO ring in place); else the capacity pass, then the
# per-slice-T embed on the fixed-T routes
AUTO = {("uint16", False, "fills"): {"k_pee_embed_res", "k_pee_extract_ss"},
        ("uint16", True, "fills"): {"k_pee_embed_ss_auto", "k_pee_extract_ss"},
        ("uint8", False, "fills"): {"k_pee_capacity"} | SS, ("uint8", True, "fills"): {"k_pee_capacity"} | SS,
        **{(dt, ip, "ragged"): {"k_pee_capacity"} | LB for dt in ("uint16", "uint8") for ip in (False, True)}}
# scheme 2: pass 0 through scheme 1's embed, then the slice-serial launch (chip-filling) or the
# per-pass tile launches; T="auto" is one launch at every size, its extract is scheme 2's
LAT_X = {"fills": {"k_pee_lat_ss_extract"}, "ragged": {"k_pee_lat_dcount", "k_pee_lat_recover"}}
SCHEME2 = {"fills": {"k_pee_embed_ss", "k_pee_lat_ss_embed"} | LAT_X["fills"],
           "ragged": {"k_pee_embed1", "k_pee_lat_count", "k_pee_lat_embed"} | LAT_X["ragged"]}
SCHEME2_AUTO = {name: {"k_pee_lat_auto"} | LAT_X[name] for name in TWO}
CRC = {"k_crc32", "k_crc32_combine"}
TAGS = {"k_poly1305_prep", "k_poly1305", "k_poly1305_finish"}
EMBED = {name: {"k_pee_embed_ss" if s else "k_pee_embed1"} for name, s in SERIAL.items()}
EXTRACT = {name: {"k_pee_extract_ss" if s else "k_pee_extract1"} for name, s in SERIAL.items()}
GATE_AUTO = {"k_pee_gate_table"} | LB
VOLUME = {name: {"k_pee_capacity", "k_vol_plan", "k_vol_scatter", "k_vol_gather"} | FIXED[name] for name in TWO}
GVOLUME = {"k_pee_gate_table", "k_gvol_plan", "k_vol_scatter", "k_vol_plan", "k_vol_gather"} | LB
BLIND = {"k_blind_rows", "k_pee_embed1"} | CRC
BLIND_AUTO = {"k_blind_rows_auto", "k_pee_embed1"} | CRC
BLIND_DECODE = {"k_pee_extract1"} | CRC


@pytest.fixture(scope="module")
def sizes():
    """(CU count, the named batch sizes) of the card"""
    pytest.importorskip("torch")
    n = BC.ncu()
    if n > BC.MAX_NCU:
        pytest.skip(f"{n} CUs: the cases are sized for batches of a few hundred slices (CU count <= {BC.MAX_NCU})")
    return n, BC.batches(n)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _stack(rows, i=0):
    return np.stack([r[i] for r in rows])


# ------------------------------------------------------------------ scheme 1
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "ip"])
@pytest.mark.parametrize("dtype", ["uint16", "uint8"])
@pytest.mark.parametrize("name", ALL)
def test_scheme1_fixed_T(sizes, name, dtype, inplace):
    from codec_tcc_amd.pee import PeeCodec
    ncu, bs = sizes
    B = bs[name]
    assert BC.fills_chip(B, ncu) == SERIAL[name]
    rows = [BC.fixed(dtype, b) for b in range(B)]
    codec = PeeCodec(B, H, W, dtype=dtype, T=BC.T_FIXED, maxval=BC.maxval(dtype))
    _run_scheme1(codec, _stack(rows), [r[1] for r in rows], [(r[2], r[3]) for r in rows], [BC.T_FIXED] * B, inplace,
                 FIXED[name])


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "ip"])
@pytest.mark.parametrize("dtype", ["uint16", "uint8"])
@pytest.mark.parametrize("name", TWO)
def test_scheme1_auto_T(sizes, name, dtype, inplace):
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    rows = [BC.auto(dtype, b) for b in range(B)]
    ts = [r[2] for r in rows]
    codec = PeeCodec(B, H, W, dtype=dtype, T="auto", tmax=BC.TMAX, maxval=BC.maxval(dtype))
    _run_scheme1(codec, _stack(rows), [r[1] for r in rows], [(r[3], r[4]) for r in rows], ts, inplace,
                 AUTO[(dtype, inplace, name)])
    assert codec.t_slices.cpu().tolist() == ts


# ------------------------------------------------------------------ scheme 2
@pytest.mark.parametrize("name", TWO)
def test_scheme2_fixed_T(sizes, name):
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    rows = [BC.scheme2("uint16", b) for b in range(B)]
    covers, bits = _stack(rows), [r[1] for r in rows]
    codec = PeeCodec(B, H, W, dtype="uint16", T=BC.T_FIXED, maxval=4095, scheme=2)
    seen = set()
    with launches(seen):
        enc = codec.embed(_gpu(covers), bits)
    _check_multi_vs_oracle(enc, covers, bits, BC.T_FIXED, 4095)
    np.testing.assert_array_equal(enc.stego.cpu().numpy(), _stack(rows, 2))
    with launches(seen):
        words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    assert seen == SCHEME2[name]
    host = words.cpu().numpy()
    for b, r in enumerate(rows):
        n = r[3]["L"]
        np.testing.assert_array_equal(framing.unpack_bits(host[b], n), bits[b][:n], err_msg=f"payload {b}")
    np.testing.assert_array_equal(back.cpu().numpy(), covers)


@pytest.mark.parametrize("name", TWO)
def test_scheme2_auto_T(sizes, name):
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    rows = [BC.scheme2_auto("uint16", b) for b in range(B)]
    covers, bits = _stack(rows), [r[1] for r in rows]
    codec = PeeCodec(B, H, W, dtype="uint16", T="auto", tmax=BC.TMAX, maxval=4095, scheme=2)
    seen = set()
    with launches(seen):
        enc = codec.embed(_gpu(covers), bits)
    _check_auto_vs_spec(codec, enc, [(r[2], r[3], r[4]) for r in rows])
    with launches(seen):
        _check_round_trip(codec, enc, covers, bits)
    assert seen == SCHEME2_AUTO[name]


# ------------------------------------------------------------------ checksums
def test_checksums(sizes):
    """checksum=True and "tiles": every slice's cover CRC, payload CRC and tile table; a clean
    decode(verify="require"); one pixel changed in slices 32 and B - 1 names exactly those
    slices and their tiles"""
    import torch
    from codec_tcc_amd import IntegrityError, checksum
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1]["ragged"]
    rows = [BC.fixed("uint16", b, True) for b in range(B)]
    covers, bits = _stack(rows), [r[1] for r in rows]
    cov = _gpu(covers)
    codec = PeeCodec(B, H, W, dtype="uint16", T=BC.T_FIXED, maxval=4095)
    want_crc = [zlib.crc32(c.astype("<u2").tobytes()) & 0xFFFFFFFF for c in covers]
    want_pay = [zlib.crc32(np.packbits(p, bitorder="little").tobytes()) & 0xFFFFFFFF for p in bits]
    seen = set()
    with launches(seen):
        plain = codec.embed(cov, bits, checksum=True)
    assert seen == CRC | EMBED["ragged"]
    assert checksum.crc_list(plain.cover_crc) == want_crc and plain.payload_crc == want_pay and plain.cover_tile_crc is None
    seen = set()
    with launches(seen):
        enc = codec.embed(cov, bits, checksum="tiles", tile=BC.TILE)
    assert seen == CRC | {"k_tile_crc"} | EMBED["ragged"]
    assert checksum.crc_list(enc.cover_crc) == want_crc and enc.payload_crc == want_pay and enc.tile == (BC.TILE, BC.TILE)
    np.testing.assert_array_equal(enc.cover_tile_crc.cpu().numpy().view(np.uint32), TS.tile_table(covers, BC.TILE))
    np.testing.assert_array_equal(enc.stego.cpu().numpy(), _stack(rows, 2))
    seen = set()
    with launches(seen):
        got, back = codec.decode(enc, verify="require")
    assert seen == CRC | EXTRACT["ragged"]           # no tile pass while every cover verifies
    assert torch.equal(back, cov)
    for b in range(B):
        np.testing.assert_array_equal(got[b], bits[b], err_msg=f"payload {b}")
    # a context pixel (even row, even column) of slices 32 and B - 1
    bad = [32, B - 1]
    stego = enc.stego.cpu().numpy().copy()
    want = {}
    for b in bad:
        stego[b, 10 + (b % 2) * 20, 40] += 64
        _bits, restored = P.pee_extract(stego[b], rows[b][3])
        want[b] = TS.mismatch_map(covers[b], restored, BC.TILE)
        assert want[b].any()
    enc.stego = _gpu(stego)
    seen = set()
    with launches(seen):
        with pytest.raises(IntegrityError) as ei:
            codec.decode(enc)
    assert seen == CRC | EXTRACT["ragged"] | {"k_tile_crc", "k_tile_compare"}
    e = ei.value
    assert e.bad_cover == bad and e.tile == (BC.TILE, BC.TILE) and sorted(e.tiles) == bad
    for b in bad:
        np.testing.assert_array_equal(e.tiles[b], want[b], err_msg=f"tiles of slice {b}")


# ------------------------------------------------------------------ keyed
def _packed_rows(rows_list, lengths):
    import torch
    pw = max(1, max(len(r) for r in rows_list))
    host = np.zeros((len(rows_list), pw), np.uint64)
    for b, r in enumerate(rows_list):
        host[b, :len(r)] = np.array(r, dtype=np.uint64)
    return (torch.from_numpy(host.view(np.int64)).cuda(), list(lengths), torch.tensor(list(lengths), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("name", TWO)
def test_keyed_embed(sizes, name):
    """embed(key=) at index0 = 2^31 - B, the last admissible: every tag is the specification's, the
    stego is the plain embed of the specification's ciphertext; decode(key=) returns every payload
    and cover; a changed pixel in slice B - 1 fails that slice alone and releases none of its row"""
    import torch
    from codec_tcc_amd import IntegrityError, aead
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    idx0 = BC.index0(B)
    codec = PeeCodec(B, H, W, dtype="uint16", T=BC.T_FIXED, maxval=4095)
    for fit in (False, True):
        rows = [BC.keyed(b, B, fit) for b in range(B)]
        covers, bits = _stack(rows), [r[1] for r in rows]
        cov = _gpu(covers)
        seen = set()
        with launches(seen):
            enc = codec.embed(cov, bits, key=BC.KEY, nonce=BC.NONCE, index0=idx0)
        assert seen == {"k_chacha20_rows"} | TAGS | EMBED[name]
        assert aead.tag_bytes(enc.tag) == [r[3] for r in rows]
        assert (enc.nonce, enc.index0, enc.payload_crc) == (BC.NONCE, idx0, None)
        np.testing.assert_array_equal(enc.stego.cpu().numpy(), _stack(rows, 4))
        assert [(m.status, m.end) for m in enc.records()] == [(r[5]["status"], r[5]["end"]) for r in rows]
        plain = codec.embed(cov, None, packed=_packed_rows([r[2] for r in rows], [len(p) for p in bits]))
        assert torch.equal(enc.stego, plain.stego) and torch.equal(enc.meta, plain.meta)
        if not fit:   # the batch holds overflowed slices: decode names them, as for an unkeyed embedding
            over = [b for b, r in enumerate(rows) if r[5]["status"] == 1]
            with pytest.raises(ValueError, match="capacity") as ev:
                codec.decode(enc, key=BC.KEY)
            assert over and str(over) in str(ev.value)
            continue
        seen = set()
        with launches(seen):
            got, back = codec.decode(enc, key=BC.KEY)
        assert seen == EXTRACT[name] | TAGS | {"k_aead_release"}
        assert torch.equal(back, cov)
        for b in range(B):
            np.testing.assert_array_equal(got[b], bits[b], err_msg=f"payload {b}")
        assert len(bits[B - 1]) > 0
        other = copy.copy(enc)
        other.stego = enc.stego.clone()
        other.stego.view(torch.int16)[B - 1, 40, 40] ^= 1
        with pytest.raises(IntegrityError) as ei:
            codec.decode(other, key=BC.KEY)
        assert ei.value.keyed and ei.value.slices == [B - 1]
        for b in range(B):   # the other slices' plaintext came through; the failed slice's row is the device's zeros
            assert (not ei.value.rows[b].any()) == (b == B - 1 or not bits[b].any()), b


# ------------------------------------------------------------------ gate and ROI
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "ip"])
@pytest.mark.parametrize("dtype", ["uint16", "uint8"])
@pytest.mark.parametrize("name", TWO)
def test_gate_fixed_T_and_G(sizes, name, dtype, inplace):
    """per-slice (T, G): everything test_pee_gate.py's _check_enc compares, and its round trip; the
    look-back at a chip-filling batch too"""
    B = sizes[1][name]
    rows = [BC.gate(dtype, b) for b in range(B)]
    seen = set()
    with launches(seen):
        gate_round_trip(_stack(rows), [r[2] for r in rows], [r[3] for r in rows], BC.maxval(dtype), inplace=inplace,
                        bits=[r[1] for r in rows])
    assert seen == LB


@pytest.mark.parametrize("name", TWO)
def test_gate_auto(sizes, name):
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    rows = [BC.gate_auto(b) for b in range(B)]
    covers, bits, Ts, Gs = _stack(rows), [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
    codec = PeeCodec(B, H, W, dtype="uint16", T="auto", tmax=BC.GATE_TMAX, maxval=4095, gate="auto")
    seen = set()
    with launches(seen):
        enc = codec.embed(_gpu(covers), bits)
    assert codec.t_slices.cpu().tolist() == Ts and codec.g_slices.cpu().tolist() == Gs
    ref = gate_check_enc(enc, covers, bits, Ts, Gs, 4095)
    with launches(seen):
        words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    assert seen == GATE_AUTO
    assert not codec.lookback_failed(enc.payload_words)
    host = words.cpu().numpy()
    for b, (_st, side) in enumerate(ref):
        np.testing.assert_array_equal(framing.unpack_bits(host[b], side["L"]), bits[b][:side["L"]], err_msg=f"payload {b}")
    np.testing.assert_array_equal(back.cpu().numpy(), covers)


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "ip"])
@pytest.mark.parametrize("name", TWO)
def test_roi(sizes, name, inplace):
    """per-slice rectangles with per-slice (T, G), the rectangles taken from roi_bbox of the batch's
    masks: the records' rectangle words, the protected pixels, every other output"""
    from codec_tcc_amd.roi import roi_bbox
    import pee_roi_spec as R
    B = sizes[1][name]
    rows = [BC.roi(b) for b in range(B)]
    seen = set()
    with launches(seen):
        rects = roi_bbox(_gpu(np.stack([BC.bbox_mask(b // 5 + b) for b in range(B)]))).cpu().tolist()
    assert seen == {"k_roi_bbox"}
    assert [tuple(r) for r in rects] == [R.normalize(r[4], H, W) for r in rows]
    seen = set()
    with launches(seen):
        roi_round_trip(_stack(rows), [r[2] for r in rows], [r[3] for r in rows], 4095, rects=rects, inplace=inplace,
                       bits=[r[1] for r in rows])
    assert seen == LB


def test_gated_in_place_persistent_grid(sizes):
    """258 x 512: nine chunks a slice, so the in-place look-back's slots exceed its 2048 persistent
    workgroups and every workgroup walks more than one; nine (cover, length) pairs in turn"""
    B = sizes[1]["ragged"]
    pairs = [BC.grid_pair(q) for q in range(9)]
    covers = np.stack([pairs[b % 9][0] for b in range(B)])
    seen = set()
    with launches(seen):
        gate_round_trip(covers, [BC.T_FIXED] * B, [24] * B, 4095, inplace=True, bits=[pairs[b % 9][1] for b in range(B)])
    assert seen == LB


# ------------------------------------------------------------------ volumes
@pytest.mark.parametrize("policy", ["even", "fill"])
@pytest.mark.parametrize("name", TWO)
def test_volume(sizes, name, policy):
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    covers, bits = BC.volume_covers(B), BC.volume_bits(B)
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=BC.GATE_TMAX, maxval=4095)
    seen = set()
    with launches(seen):
        vol = codec.embed_volume(_gpu(covers), bits, policy=policy)
        p = _check_volume(codec, vol, covers, bits, policy, 4095, tmax=BC.GATE_TMAX)
    assert seen == VOLUME[name]
    assert p["status"] == 0 and p["n"][BC.SATURATED] == 0 and (p["n"] == 0).sum() > (1 if policy == "fill" else 0)


@pytest.mark.parametrize("name", TWO)
def test_volume_gate_auto(sizes, name):
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    covers, bits = np.array(BC.volume_covers(B)), BC.volume_bits(B, True)   # (a writable copy: the helper wraps it in a tensor)
    codec = PeeCodec(B, H, W, dtype="uint16", T=3, tmax=BC.GATE_TMAX, maxval=4095)
    seen = set()
    with launches(seen):
        vol = codec.embed_volume(_gpu(covers), bits, policy="even", gate="auto")
        p = _check_gvol(codec, vol, covers, bits, "even", 4095, "auto", tmax=BC.GATE_TMAX)
    assert seen == GVOLUME
    assert p["status"] == 0 and p["n"][BC.SATURATED] == 0


@pytest.mark.parametrize("name", TWO)
def test_volume_keyed(sizes, name):
    """embed_volume(key=): the stego is the plain volume embed of the specification's ciphertext
    stream, the stream's tag and every cover's tag are the specification's, decode_volume(key=)
    returns the stream and the stack"""
    import torch
    import aead_spec as AES
    from codec_tcc_amd import aead, framing
    from codec_tcc_amd.pee import PeeCodec
    B = sizes[1][name]
    idx0 = BC.index0(B)
    covers, bits = BC.volume_covers(B), BC.volume_bits(B)
    n = len(bits)
    words = [int(v) for v in framing.pack_bits([bits])[0].reshape(-1).view(np.uint64)]
    ct = AES.crypt_row(BC.KEY, BC.NONCE, AES.STREAM_INDEX, words, n)
    cov = _gpu(covers)
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=BC.GATE_TMAX, maxval=4095)
    seen = set()
    with launches(seen):
        vol = codec.embed_volume(cov, bits, policy="even", key=BC.KEY, nonce=BC.NONCE, index0=idx0)
    assert seen == {"k_chacha20_rows", "k_pee_capacity", "k_vol_plan", "k_vol_scatter"} | TAGS | EMBED[name]
    assert vol.embedded_bits == n
    plain = codec.embed_volume(cov, None, policy="even", packed=(_gpu(np.array(ct, dtype=np.uint64).view(np.int64)), n))
    assert torch.equal(vol.enc.stego, plain.enc.stego) and torch.equal(vol.enc.meta, plain.enc.meta)
    ct_bits = np.unpackbits(np.frombuffer(AES.row_bytes(ct, n), dtype=np.uint8), bitorder="little")[:n]
    _check_volume(codec, plain, covers, ct_bits, "even", 4095, tmax=BC.GATE_TMAX)   # and that one is the spec's
    assert aead.tag_bytes(vol.tag) == [AES.tag(BC.KEY, BC.NONCE, AES.STREAM_INDEX, b"", ct, n)]
    assert aead.tag_bytes(vol.enc.tag) == [AES.tag(BC.KEY, BC.NONCE, idx0 + b, covers[b].tobytes(), [], 0) for b in range(B)]
    seen = set()
    with launches(seen):
        got, back = codec.decode_volume(vol, key=BC.KEY)
    assert seen == EXTRACT[name] | {"k_vol_plan", "k_vol_gather", "k_aead_release"} | TAGS
    assert torch.equal(back, cov)
    np.testing.assert_array_equal(got, bits)


# ------------------------------------------------------------------ blind
def _blind_codec(B, T):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, H, W, dtype="uint16", T=T, tmax=BC.TMAX, maxval=4095)


@pytest.mark.parametrize("name", TWO)
def test_blind_fixed_T(sizes, name):
    """stego, info and capacity of every slice; the embedded ones decode in reversed slice order on a
    codec built with another T"""
    B = sizes[1][name]
    rows = [BC.blind(b) for b in range(B)]
    covers = _stack(rows)
    cov = _gpu(covers)
    codec = _blind_codec(B, BC.BLIND_T)
    seen = set()
    with launches(seen):
        stego, info = codec.embed_blind(cov, [r[1] for r in rows], checksum=True, max_entries=BC.BLIND_ME, check=False)
    assert seen == BLIND
    seen = set()
    with launches(seen):
        cap = codec.blind_capacity(cov, BC.BLIND_ME)
    assert seen == {"k_blind_rows"}
    got_st, got_info, got_cap = stego.cpu().numpy(), info.cpu().numpy(), cap.cpu().tolist()
    for b, (img, _bits, st, winfo, wcap) in enumerate(rows):
        assert tuple(int(v) for v in got_info[b]) == winfo, (b, got_info[b], winfo)
        assert got_cap[b] == wcap, b
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"stego of slice {b}")
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)
    keep = [b for b in range(B) if rows[b][3][0] == 0][::-1]
    other = _blind_codec(len(keep), 13)
    seen = set()
    with launches(seen):
        out, back = other.decode_blind(_gpu(got_st[keep]))
    assert seen == BLIND_DECODE
    np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
    for k, b in enumerate(keep):
        np.testing.assert_array_equal(out[k], rows[b][1], err_msg=f"bits of slice {b}")


@pytest.mark.parametrize("name", TWO)
def test_blind_auto_T(sizes, name):
    B = sizes[1][name]
    rows = [BC.blind_auto(b) for b in range(B)]
    covers = _stack(rows)
    cov = _gpu(covers)
    codec = _blind_codec(B, 11)
    seen = set()
    with launches(seen):
        stego, info, ts = codec.embed_blind_auto(cov, [r[1] for r in rows], tmax=BC.TMAX, checksum=True,
                                                 max_entries=BC.BLIND_ME, check=False)
    assert seen == BLIND_AUTO
    seen = set()
    with launches(seen):
        curve = codec.blind_capacity_curve(cov, tmax=BC.TMAX, max_entries=BC.BLIND_ME)
    assert seen == {"k_blind_rows_auto"}
    got_st, got_info, got_ts, got_curve = stego.cpu().numpy(), info.cpu().numpy(), ts.cpu().tolist(), curve.cpu().tolist()
    for b, (img, _bits, st, winfo, T, wcurve) in enumerate(rows):
        assert got_ts[b] == T, (b, got_ts[b], T)
        assert tuple(int(v) for v in got_info[b]) == winfo, (b, got_info[b], winfo)
        assert got_curve[b] == wcurve, b
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"stego of slice {b}")
    keep = [b for b in range(B) if rows[b][4]]
    other = _blind_codec(len(keep), 13)
    seen = set()
    with launches(seen):
        out, back = other.decode_blind(_gpu(got_st[keep]))
    assert seen == BLIND_DECODE
    np.testing.assert_array_equal(back.cpu().numpy(), covers[keep])
    for k, b in enumerate(keep):
        np.testing.assert_array_equal(out[k], rows[b][1], err_msg=f"bits of slice {b}")


def test_blind_keyed(sizes):
    """fixed T and tmax = 8 at index0 = 2^31 - B under two nonces: stego, info and T of every slice;
    decode_blind_keyed of one batch that takes its even slices from the first embed and its odd
    ones from the second"""
    B = sizes[1]["ragged"]
    idx0 = BC.index0(B)
    both = []
    for auto_t, nonce, rows_tag in ((False, BC.NONCE, "k_blind_rows"), (True, BC.NONCE_2, "k_blind_rows_auto")):
        rows = [BC.blind_keyed(b, B, auto_t, nonce) for b in range(B)]
        covers = _stack(rows)
        codec = _blind_codec(B, BC.BLIND_T)
        seen = set()
        with launches(seen):
            stego, info, ts = codec.embed_blind_keyed(_gpu(covers), [r[1] for r in rows], key=BC.KEY, nonce=nonce, index0=idx0,
                                                      tmax=BC.TMAX if auto_t else None, max_entries=BC.BLIND_ME, check=False)
        assert seen == {"k_chacha20_rows", rows_tag, "k_pee_embed1"} | TAGS
        got_st, got_info, got_ts = stego.cpu().numpy(), info.cpu().numpy(), ts.cpu().tolist()
        for b, (img, _bits, st, winfo, T) in enumerate(rows):
            assert got_ts[b] == T, (auto_t, b, got_ts[b], T)
            assert tuple(int(v) for v in got_info[b]) == winfo, (auto_t, b, got_info[b], winfo)
            np.testing.assert_array_equal(got_st[b], st, err_msg=f"stego of slice {b}")
        both.append((rows, got_st))
    pick = [(b, both[b % 2]) for b in range(B) if both[b % 2][0][b][3][0] == 0]
    assert {b % 2 for b, _s in pick} == {0, 1} and len(pick) > 64
    mixed = np.stack([st[b] for b, (_rows, st) in pick])
    other = _blind_codec(len(pick), 13)
    seen = set()
    with launches(seen):
        out, back = other.decode_blind_keyed(_gpu(mixed), BC.KEY)
    assert seen == {"k_pee_extract1", "k_aead_release"} | TAGS
    back = back.cpu().numpy()
    for k, (b, (rows, _st)) in enumerate(pick):
        np.testing.assert_array_equal(out[k], rows[b][1], err_msg=f"bits of slice {b}")
        np.testing.assert_array_equal(back[k], rows[b][0], err_msg=f"cover of slice {b}")


# ------------------------------------------------------------------ quality
def test_quality_moments(sizes):
    from codec_tcc_amd import quality as Q
    B = sizes[1]["ragged"]
    rows = [BC.fixed("uint16", b) for b in range(B)]
    seen = set()
    with launches(seen):
        got = Q.moments(_gpu(_stack(rows)), _gpu(_stack(rows, 2)))
    assert seen == {"k_quality"}
    for b, r in enumerate(rows):
        m = O.moments(r[0], r[2])
        assert [int(x) for x in got[b]] == [m[k] for k in Q.KEYS], b
