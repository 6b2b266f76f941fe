"""The alignment-selected routes, and the buffer contract on real codecs.

The C ABI picks its kernel family from the low bits of the pixel pointers (pee_route's vec,
codec_pee_capacity's and codec_gate.hip's vec, pee_extract_t's 16-byte copy test,
pee_lss_copy_mode, the LSB use_fast_scan and restore branch, the quality kernel's vec).  Torch
allocations are aligned to 256 bytes and more, so a test that uploads an array always takes the
aligned side of every one of them.  Here every array is placed in a contiguous view at a chosen
element offset of a sentinel-filled buffer (Placed): W % 8 == 0 throughout, so the pointer alone
decides the route.  Every result is compared bit for bit with oracle/pee_cpu.py (the gated
cases with tests/pee_gate_spec.py / pee_gvol_spec.py, the LSB case with oracle/ref_cpu.py) by the
checks of test_pee_adversarial / test_pee_gate / test_pee_volume / test_pee_gvol; the buffers'
margins must still hold the sentinel afterwards, and the source of an out-of-place call its
upload.  At B = 3 the launch families recorded around each call (test_pee_launch_variants) pin
the selection itself: an image off its 8-pixel vector boundary (16 B for uint16, 8 B for uint8)
must not reach the look-back, slice-serial or resident kernels, and the uint8 pointer with
ptr % 16 == 8 still must.

The second half (test_rejected_*) hands every public entry memory it cannot take, with
codec_tcc_amd._lib.load replaced by a stub whose every attribute raises: no rejected argument
may reach the library.  The rules themselves are pinned on CPU tensors in
tests/test_buffer_contract.py.
"""
import dataclasses
import functools

import numpy as np
import pytest

import pee_covers as PC
import pee_gate_spec as G
import pee_volume_spec as V
from test_pee_adversarial import (KINDS, MULTI_TMAX, _auto_case, _check_extract, _check_multi, _check_scheme1,
                                  _fixed_case, _multi_auto_case, _multi_case)
from test_pee_launch_variants import TWOPASS, _launches

pytestmark = pytest.mark.gpu

PAD = 64                                            # margin elements on both sides of a placed view
SENTINEL = {"uint16": 0xA5C3, "uint8": 0xA5}
OFFSETS = {"uint16": (0, 1, 4), "uint8": (0, 1, 8)}   # elements: ptr % 16 = 0, 2, 8 / 0, 1, 8
VECTOR_BYTES = {"uint16": 16, "uint8": 8}           # one 8-pixel vector: pee_route's alignment
# the families an image off its vector boundary must not reach
VECTOR_ROUTES = {"k_pee_embed1", "k_pee_extract1", "k_pee_embed_ss", "k_pee_extract_ss", "k_pee_embed_res"}
SHAPES = [(72, 512),    # 2.25 look-back chunks
          (65, 96)]     # odd H: the last-row copy beside an offset base
# (source, destination) as indices into OFFSETS[dtype]; None: in place
PAIRS = [(0, 0), (1, 1), (1, 0), (0, 1), (2, 2)]
IN_PLACE = [(0, None), (1, None), (2, None)]


def _pid(place):
    return "ip%d" % place[0] if place[1] is None else "c%d-s%d" % place


class Placed:
    """A [B, H, W] view `k` elements past the 64-element margin of a sentinel-filled device
    buffer; host: what the view holds (None: the sentinel, an output buffer)."""

    def __init__(self, shape, dtype, k, host=None):
        import torch
        dt = np.dtype(dtype)
        self.n, self.k, self.host, self.sentinel = int(np.prod(shape)), int(k), host, SENTINEL[dt.name]
        buf = np.full(self.n + 2 * PAD, self.sentinel, dt)
        if host is not None:
            assert host.dtype == dt and host.shape == tuple(shape)
            buf[PAD + k:PAD + k + self.n] = host.ravel()
        self.flat = torch.from_numpy(buf).cuda()
        self.view = self.flat[PAD + k:PAD + k + self.n].view(*shape)
        assert self.view.is_contiguous()
        assert self.view.data_ptr() % 16 == (k * dt.itemsize) % 16, "the allocation is not 16-byte aligned"

    def check(self, unchanged=False):
        """Both margins still hold the sentinel; unchanged: the view still holds its upload."""
        got = self.flat.cpu().numpy()
        lo, hi = PAD + self.k, PAD + self.k + self.n
        for name, part, base in (("before", got[:lo], 0), ("after", got[hi:], hi)):
            bad = np.flatnonzero(part != self.sentinel)
            assert bad.size == 0, f"{bad.size} margin elements {name} the view (k = {self.k}) were written; first at " \
                                  f"buffer element {base + int(bad[0])} (view {lo}..{hi})"
        if unchanged:
            np.testing.assert_array_equal(got[lo:hi], self.host.ravel(), err_msg="the source of an out-of-place call changed")


def _pair(shape, dtype, place, host):
    """(source holding `host`, destination) placed as `place` says; in place: the same object."""
    ks = OFFSETS[dtype]
    src = Placed(shape, dtype, ks[place[0]], host)
    return src, (src if place[1] is None else Placed(shape, dtype, ks[place[1]]))


def _check_pair(src, dst):
    src.check(unchanged=src is not dst)
    if dst is not src:
        dst.check()


def _assert_not_vacuous(sides, nc):
    """From the oracle alone: a truncated slice, an empty one, a non-empty location map and an
    `end` before the last candidate."""
    assert any(s["status"] == 1 for s in sides)
    assert any(s["L"] == 0 for s in sides)
    assert any(int(np.asarray(s["lm"]).sum()) > 0 for s in sides)
    assert any(0 <= s["end"] < nc - 1 for s in sides)


@functools.lru_cache(maxsize=None)
def _fixed(h, w, dtype, maxval, T, nb):
    """The first nb slices of test_pee_adversarial's fixed-T batch (variant 0: zero / half / cap /
    over payload lengths by kind): covers, payloads, sides, stegos."""
    cov, pays, exp = _fixed_case(h, w, dtype, maxval, T, 0)
    sides, stegos = [s for _st, s in exp[:nb]], [st for st, _s in exp[:nb]]
    _assert_not_vacuous(sides, (h // 2) * (w // 2))
    return cov[:nb], list(pays[:nb]), sides, stegos


# ------------------------------------------------------------------ 1, 2: scheme 1, fixed T
FIXED_ROWS = [("uint16", 4095, 2), ("uint8", None, 2)]
# 8 slices: the grouped look-back order; 3: flat slots, with the route witness, again under CODEC_PEE_SS=1
BATCHES = [(8, False), (3, False), (3, True)]


@pytest.mark.parametrize("place", PAIRS + IN_PLACE, ids=_pid)
@pytest.mark.parametrize("nb,ss", BATCHES, ids=["b8", "b3", "b3-ss"])
@pytest.mark.parametrize("dtype,maxval,T", FIXED_ROWS, ids=["u16", "u8"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_fixed_T_placements(h, w, dtype, maxval, T, nb, ss, place, monkeypatch):
    """Embed with (cover k, stego k'), extract with (stego k, cover_out k') and both in place at
    every k.  B = 3: with both images on their vector boundary the call records exactly the
    look-back kernel (CODEC_PEE_SS=1: the slice-serial one), else only two-pass families."""
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    if ss:
        monkeypatch.setenv("CODEC_PEE_SS", "1")
    cov, pays, sides, stegos = _fixed(h, w, dtype, maxval, T, nb)
    codec = PeeCodec(nb, h, w, dtype=dtype, T=T, maxval=maxval)
    inplace = place[1] is None
    src, dst = _pair(cov.shape, dtype, place, cov)
    seen = set()
    with _launches(seen):
        enc = codec.embed(src.view, pays, stego=dst.view)
    assert enc.stego.data_ptr() == dst.view.data_ptr()
    _check_scheme1(enc, cov, sides, stegos, what=_pid(place))
    _check_pair(src, dst)
    off = src.view.data_ptr() % VECTOR_BYTES[dtype] != 0 or dst.view.data_ptr() % VECTOR_BYTES[dtype] != 0
    assert off == (place[0] == 1 or place[1] == 1 or (dtype == "uint16" and 2 in place))
    if nb == 3:
        _witness(seen, off, "k_pee_embed_ss" if ss else "k_pee_embed1")
    # the extract reads the oracle's stego at the source's offset and restores into the destination's
    xin, xout = _pair(cov.shape, dtype, place, np.stack(stegos))
    seen = set()
    with _launches(seen):
        _check_extract(codec, dataclasses.replace(enc, stego=xin.view), cov, pays, [s["L"] for s in sides], inplace,
                       cover=None if inplace else xout.view)
    assert not codec.lookback_failed(enc.payload_words)
    _check_pair(xin, xout)
    if nb == 3:
        _witness(seen, off, "k_pee_extract_ss" if ss else "k_pee_extract1")


def _witness(seen, off, vector_family):
    if off:
        assert seen and not (seen & VECTOR_ROUTES) and seen <= TWOPASS, seen
    else:
        assert seen == {vector_family}, seen


# ------------------------------------------------------------------ 3: scheme 1, T = "auto"
@pytest.mark.parametrize("place", [(0, 0), (1, 0), (0, 1), (2, 2)], ids=_pid)
def test_auto_T_placements(place, monkeypatch):
    """130 x 512 uint16, tmax 5, slice-serial forced: aligned, the resident kernel; with the
    cover or the stego offset, the capacity pass + per-slice-T embed -- the same t_slices,
    records and stego, the oracle's at select_T's T.  capacity() and gate_table() on the placed
    cover equal capacity_curve and the gate spec's table."""
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_SS", "1")
    h, w, maxval, tmax = 130, 512, 4095, 5
    cov, pays, curves, exp = _auto_case(h, w, "uint16", maxval, tmax, 0)
    ts, stegos, sides = [e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]
    _assert_not_vacuous(sides, (h // 2) * (w // 2))
    codec = PeeCodec(len(KINDS), h, w, dtype="uint16", T="auto", tmax=tmax, maxval=maxval)
    src, dst = _pair(cov.shape, "uint16", place, cov)
    seen = set()
    with _launches(seen):
        enc = codec.embed(src.view, list(pays), stego=dst.view)
    if place == (0, 0):
        assert seen == {"k_pee_embed_res"}, seen
    else:
        assert "k_pee_capacity" in seen and not (seen & VECTOR_ROUTES), seen
    assert codec.t_slices.cpu().tolist() == ts
    _check_scheme1(enc, cov, sides, stegos, ts=ts, what=_pid(place))
    np.testing.assert_array_equal(codec.capacity(src.view).cpu().numpy(), curves)
    n, hs = (t.cpu().numpy() for t in codec.gate_table(src.view))
    for b, c in enumerate(cov):
        sn, sh = G.table(c, tmax, maxval)
        np.testing.assert_array_equal(n[b], sn, err_msg=f"n of slice {b}")
        np.testing.assert_array_equal(hs[b], sh, err_msg=f"hs of slice {b}")
    _check_pair(src, dst)
    xout = Placed(cov.shape, "uint16", OFFSETS["uint16"][place[0]])   # stego at the destination's k, cover at the source's
    _check_extract(codec, enc, cov, pays, [s["L"] for s in sides], False, cover=xout.view)
    xout.check()
    dst.check()


@pytest.mark.parametrize("place", [(2, 2), (2, 0)], ids=_pid)
def test_auto_T_uint8_at_8_bytes(place, monkeypatch):
    """uint8 with ptr % 16 == 8: codec_pee_embed_auto asks for 16 bytes whatever the pixel size
    and runs the capacity pass first; codec_pee_embed_ts then takes the 8-byte vectors."""
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_SS", "1")
    h, w, maxval, tmax = 130, 512, 127, 16
    cov, pays, curves, exp = _auto_case(h, w, "uint8", maxval, tmax, 0)
    ts, stegos, sides = [e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]
    codec = PeeCodec(len(KINDS), h, w, dtype="uint8", T="auto", tmax=tmax, maxval=maxval)
    src, dst = _pair(cov.shape, "uint8", place, cov)
    assert src.view.data_ptr() % 16 == 8
    seen = set()
    with _launches(seen):
        enc = codec.embed(src.view, list(pays), stego=dst.view)
    assert seen == {"k_pee_capacity", "k_pee_embed_ss"}, seen
    assert codec.t_slices.cpu().tolist() == ts
    _check_scheme1(enc, cov, sides, stegos, ts=ts, what=_pid(place))
    np.testing.assert_array_equal(codec.capacity(src.view).cpu().numpy(), curves)
    _check_pair(src, dst)
    xout = Placed(cov.shape, "uint8", 8)
    _check_extract(codec, enc, cov, pays, [s["L"] for s in sides], False, cover=xout.view)
    xout.check()


# ------------------------------------------------------------------ 4: scheme 2
MULTI_ROWS = [("uint16", 4095, 16), ("uint8", 127, 4)]
MULTI_PLACES = [(0, 0), (1, 0), (0, 1), (2, 2)]
# the per-pass tile launches; the slice-serial launch after scheme 1's pass 0 (no copy of its
# own); the copy and all four passes in the one launch (pee_lss_copy_mode 1 or 2 by the pointers)
LATTICE_MODES = {"tile": {"CODEC_PEE_LAT_SS": "0"},
                 "lss-p0s1": {"CODEC_PEE_LAT_SS": "1", "CODEC_PEE_LAT_SS_P0": "1"},
                 "lss-copy": {"CODEC_PEE_LAT_SS": "1", "CODEC_PEE_LAT_SS_P0": "0"}}


def _extract_multi(codec, enc, cov, pays, sides, stegos, dtype, place):
    """stego (the oracle's) at the source's offset, the cover out at the destination's."""
    from codec_tcc_amd import framing
    xin, xout = _pair(cov.shape, dtype, place, np.stack(stegos))
    words, back = codec.extract(xin.view, enc.meta, enc.lm, payload_words=enc.payload_words, cover=xout.view)
    assert back.data_ptr() == xout.view.data_ptr()
    host = words.cpu().numpy()
    for i, side in enumerate(sides):
        np.testing.assert_array_equal(framing.unpack_bits(host[i], side["L"]), pays[i][: side["L"]])
    np.testing.assert_array_equal(back.cpu().numpy(), cov)
    _check_pair(xin, xout)


@pytest.mark.parametrize("place", MULTI_PLACES, ids=_pid)
@pytest.mark.parametrize("mode", list(LATTICE_MODES))
@pytest.mark.parametrize("dtype,maxval,T", MULTI_ROWS, ids=["u16", "u8"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_scheme2_placements(h, w, dtype, maxval, T, mode, place, monkeypatch):
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    for k, v in LATTICE_MODES[mode].items():
        monkeypatch.setenv(k, v)
    cov, pays, exp = _multi_case(h, w, dtype, maxval, T)
    sides, stegos = [s for _st, s in exp], [st for st, _s in exp]
    assert any(s["status"] == 1 for s in sides) and any(s["status"] == 0 and s["L"] > 0 for s in sides)
    assert any(ps["lm"].any() for s in sides for ps in s["passes"])
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T=T, maxval=maxval, scheme=2)
    src, dst = _pair(cov.shape, dtype, place, cov)
    enc = codec.embed(src.view, list(pays), stego=dst.view)
    _check_multi(enc, sides, stegos, T=T)
    _check_pair(src, dst)
    _extract_multi(codec, enc, cov, pays, sides, stegos, dtype, place)


@pytest.mark.parametrize("place", MULTI_PLACES, ids=_pid)
@pytest.mark.parametrize("dtype,maxval", [("uint16", 4095), ("uint8", 127)], ids=["u16", "u8"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_scheme2_auto_placements(h, w, dtype, maxval, place):
    """k_pee_lat_auto (tmin 1, tmax 6): its copy mode follows the pointers."""
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    cov, pays, exp = _multi_auto_case(h, w, dtype, maxval)
    ts, stegos, sides = [e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]
    assert len(set(ts)) > 1 and any(s["status"] == 1 for s in sides) and any(s["L"] == 0 for s in sides)
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T="auto", tmin=1, tmax=MULTI_TMAX, maxval=maxval, scheme=2)
    src, dst = _pair(cov.shape, dtype, place, cov)
    enc = codec.embed(src.view, list(pays), stego=dst.view)
    assert codec.t_slices.cpu().tolist() == ts
    _check_multi(enc, sides, stegos, ts=ts)
    _check_pair(src, dst)
    _extract_multi(codec, enc, cov, pays, sides, stegos, dtype, place)


# ------------------------------------------------------------------ 5: the gate's table pass
@pytest.mark.parametrize("place", [(1, 0), (1, 1), (0, 1)], ids=_pid)
def test_gate_auto_placements(place):
    """gate="auto", T="auto": codec_gate.hip's table pass picks its kernel by the cover's
    pointer, the embed by both (test_pee_gate.py::test_gpu_gate_auto_embeds_the_specs_choice's
    covers and payloads)."""
    pytest.importorskip("torch")
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    from test_pee_gate import _check_enc, _ct12
    covers = _ct12(4, 130, 512, 370)
    covers[3] = PC.cover("top_band", 130, 512, "uint16", 4095, 2, 9)
    lengths = [500, 0, 4000, 10 ** 6]
    bits = [G.payload_bits(n, 3 + i) for i, n in enumerate(lengths)]
    picks = [G.select(*G.table(c, 16, 4095), L, 0) for c, L in zip(covers, lengths)]
    Ts, Gs = [p[0] for p in picks], [G.GATES[p[1]] for p in picks]
    codec = PeeCodec(4, 130, 512, T="auto", tmax=16, maxval=4095, gate="auto")
    src, dst = _pair(covers.shape, "uint16", place, covers)
    enc = codec.embed(src.view, bits, stego=dst.view)
    assert codec.t_slices.cpu().tolist() == Ts and codec.g_slices.cpu().tolist() == Gs
    ref = _check_enc(enc, covers, bits, Ts, Gs, 4095)
    assert any(side["status"] == 1 for _st, side in ref) and any(side["L"] == 0 for _st, side in ref)
    _check_pair(src, dst)
    xout = Placed(covers.shape, "uint16", OFFSETS["uint16"][place[0]])
    words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words, cover=xout.view)
    host = words.cpu().numpy()
    for b, (_st, side) in enumerate(ref):
        np.testing.assert_array_equal(framing.unpack_bits(host[b], side["L"]), bits[b][:side["L"]])
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    xout.check()
    dst.check()


# ------------------------------------------------------------------ 6: volume payloads
@pytest.mark.parametrize("place", [(1, 0), (0, 1), (1, 1), (1, None)], ids=_pid)
@pytest.mark.parametrize("gate", [None, "auto"], ids=["ungated", "gate-auto"])
def test_volume_placements(gate, place):
    """embed_volume / decode_volume (policy "even", B = 3) with the covers and the stego each
    offset, and in place at an offset: plan, per-slice records, stream bits and restored stack
    by test_pee_volume's / test_pee_gvol's own checks."""
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    from test_pee_gvol import _check_gvol
    from test_pee_volume import _check_volume
    covers = V.ct12_batch("5x64x96")[:3].copy()
    bits = V.stream_bits(150 if gate is None else 60, 31)
    codec = PeeCodec(3, 64, 96, dtype="uint16", T=3, tmax=16, maxval=4095)
    src, dst = _pair(covers.shape, "uint16", place, covers)
    vol = codec.embed_volume(src.view, bits, policy="even", stego=dst.view, gate=gate)
    assert vol.enc.stego.data_ptr() == dst.view.data_ptr()
    if gate is None:
        p = _check_volume(codec, vol, covers, bits, "even", 4095)
    else:
        p = _check_gvol(codec, vol, covers, bits, "even", 4095, gate)
    assert p["total"] == len(bits) and len(set(int(v) for v in p["n"])) > 1   # the whole stream, unevenly shared
    _check_pair(src, dst)


# ------------------------------------------------------------------ 7: the LSB codec
def test_lsb_placements():
    """Codec.encode with the cover one pixel off and an aligned stego (use_fast_scan needs
    both: the generic scan, no vector one, is recorded), Codec.decode with stego and cover 4 bytes off (the scalar restore), against
    oracle/ref_cpu.py as test_gpu_parity.py::test_batch_vs_oracle; a stego 2 bytes off is
    refused (codec_encode's 4-byte rule) and nothing is written."""
    pytest.importorskip("torch")
    from codec_tcc_amd import Codec, framing, synth
    from codec_tcc_amd import codec as K
    from oracle import ref_cpu as R
    bsz, h, w = 3, 120, 136
    covers = np.stack([synth.ct12(h, w, 100 + i) for i in range(bsz)])
    msgs = [synth.payload(64 + 37 * i, i) for i in range(bsz)]
    codec = Codec(bsz, h, w, dtype="uint16", beta=0.4, block=16)
    fast_scans = {"k_scan_fast", "k_scan_rows", "k_scan_read", "k_scan_rows_read", "k_scan_decide"}
    seen = set()
    with _launches(seen):   # the control: both images aligned
        codec.encode(Placed(covers.shape, "uint16", 0, covers).view, msgs, stego=Placed(covers.shape, "uint16", 0).view)
    assert seen & fast_scans and "k_scan_generic" not in seen, seen
    src, dst = Placed(covers.shape, "uint16", 1, covers), Placed(covers.shape, "uint16", 0)
    seen = set()
    with _launches(seen):
        enc = codec.encode(src.view, msgs, stego=dst.view)
    assert "k_scan_generic" in seen and not (seen & fast_scans), seen
    recs = enc.records()
    stego = enc.stego.cpu().numpy()
    for i in range(bsz):
        exp = R.encode_slice(covers[i], R.message_to_bits(msgs[i]), beta=0.4, sb=16)
        assert (recs[i].s, recs[i].start_offset) == (exp["s"], exp["start_offset"])
        np.testing.assert_array_equal(stego[i], exp["stego"])
    _check_pair(src, dst)
    xin, xout = Placed(covers.shape, "uint16", 2, stego), Placed(covers.shape, "uint16", 2)
    assert xin.view.data_ptr() % 16 == 4
    words, back = codec.decode(xin.view, enc.maps, enc.meta, payload_words=enc.payloads.payload_words,
                               map_words=enc.payloads.map_words, cover=xout.view)
    host = words.cpu().numpy()
    for i in range(bsz):
        assert framing.bits_to_str(framing.unpack_bits(host[i], recs[i].total_used)) == R.message_to_bits(msgs[i])
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    _check_pair(xin, xout)
    odd = Placed(covers.shape, "uint16", 1)
    with pytest.raises((RuntimeError, ValueError), match="4-byte aligned"):
        codec.encode(src.view, msgs, stego=odd.view)
    K._torch().cuda.synchronize()
    odd.check()
    assert (odd.flat.cpu().numpy() == odd.sentinel).all()
    src.check(unchanged=True)


# ------------------------------------------------------------------ 8: quality, one image offset
@pytest.mark.parametrize("dt,h,w,bsz", [("uint16", 520, 504, 2), ("uint8", 64, 96, 4)])
@pytest.mark.parametrize("ka,kb", [(0, 1), (1, 0)])
def test_quality_mixed_placement(dt, h, w, bsz, ka, kb):
    """One image aligned, the other one element off: the scalar kernel, exact moments
    (tests/test_quality.py has both aligned and both off)."""
    pytest.importorskip("torch")
    from codec_tcc_amd import quality as Q
    from oracle import quality_cpu as O
    from test_quality import _moment_pair
    a, b = _moment_pair(dt, h, w, bsz)
    assert (h * w) % 8 == 0
    pa, pb = Placed(a.shape, dt, ka, a), Placed(b.shape, dt, kb, b)
    got = Q.moments(pa.view, pb.view)
    for i in range(bsz):
        m = O.moments(a[i], b[i])
        assert [int(x) for x in got[i]] == [m[k] for k in Q.KEYS]
    pa.check(unchanged=True)
    pb.check(unchanged=True)


# ================================================================== rejections that cannot launch
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"reached the library ({name})")


@pytest.fixture
def no_library(monkeypatch):
    """After this, any use of the library is an AssertionError (build the codec first)."""
    def arm():
        from codec_tcc_amd import _lib
        monkeypatch.setattr(_lib, "load", lambda *a, **k: _NoLibrary())
    return arm


RB, RH, RW = 3, 16, 64


def _bad_pixels(torch, kind, dtype=None):
    """A tensor of the codec's shape and dtype that the library cannot take, and the exception."""
    dtype = dtype or torch.uint16
    if kind == "cpu":
        return torch.zeros((RB, RH, RW), dtype=dtype), TypeError
    if kind == "strided":
        return torch.zeros((RB, RH, 2 * RW), dtype=dtype, device="cuda")[:, :, ::2], ValueError
    if kind == "crop":
        return torch.zeros((RB, RH + 4, RW + 8), dtype=dtype, device="cuda")[:, :RH, :RW], ValueError
    raise KeyError(kind)


def _overlapping(torch, dtype=None):
    """(a, b): b starts one row into a."""
    flat = torch.zeros(RB * RH * RW + RW, dtype=dtype or torch.uint16, device="cuda")
    n = RB * RH * RW
    return flat[:n].view(RB, RH, RW), flat[RW:RW + n].view(RB, RH, RW)


def _good(torch, codec, scheme=1):
    from codec_tcc_amd import _lib
    lead = (4, RB) if scheme == 2 else (RB,)
    dev = "cuda"
    return dict(pix=torch.zeros((RB, RH, RW), dtype=torch.uint16, device=dev),
                lm=torch.zeros(lead + (codec.lm_words,), dtype=torch.int64, device=dev),
                meta=torch.zeros(lead + (_lib.PEE_META_BYTES,), dtype=torch.uint8, device=dev),
                packed=(torch.zeros((RB, 2), dtype=torch.int64, device=dev), [0] * RB,
                        torch.zeros(RB, dtype=torch.int32, device=dev)))


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("kind", ["cpu", "strided", "crop"])
def test_rejected_pixels_reach_no_library(kind, scheme, no_library):
    """covers / stego / cover of every entry: a CPU tensor, a [:, :, ::2] view, a crop."""
    import torch
    from codec_tcc_amd.pee import PeeCodec, PeeEncoded, PeeVolume
    codec = PeeCodec(RB, RH, RW, dtype="uint16", T=2, scheme=scheme)
    g = _good(torch, codec, scheme)
    bad, exc = _bad_pixels(torch, kind)
    no_library()
    with pytest.raises(exc, match="^covers "):
        codec.embed(bad, None, packed=g["packed"])
    with pytest.raises(exc, match="^covers "):
        codec.embed(bad, [b"a"] * RB, checksum=True)           # the checksum launch comes after the check
    with pytest.raises(exc, match="^stego "):
        codec.embed(g["pix"], None, stego=bad, packed=g["packed"], checksum=True)
    with pytest.raises(exc, match="^stego "):
        codec.extract(bad, g["meta"], g["lm"], payload_words=2)
    with pytest.raises(exc, match="^cover "):
        codec.extract(g["pix"], g["meta"], g["lm"], payload_words=2, cover=bad)
    enc = PeeEncoded(stego=bad, lm=g["lm"], meta=g["meta"], lengths=[0] * RB, payload_words=2, config=codec.config,
                     scheme=scheme)
    with pytest.raises(exc, match="^stego "):
        codec.decode(enc)
    if scheme == 1:
        with pytest.raises(exc, match="^covers "):
            codec.capacity(bad)
        with pytest.raises(exc, match="^covers "):
            codec.gate_table(bad)
        with pytest.raises(exc, match="^covers "):
            codec.capacity(bad, gate=5)
        with pytest.raises(exc, match="^covers "):
            codec.embed_volume(bad, b"abc", checksum=True)
        with pytest.raises(exc, match="^stego "):
            codec.embed_volume(g["pix"], b"abc", stego=bad, gate="auto")
        with pytest.raises(exc, match="^stego "):
            codec.decode_volume(PeeVolume(enc=enc, total_bits=24, policy="even", plan=None, info=None))


@pytest.mark.parametrize("scheme", [1, 2])
def test_rejected_overlap_and_side_buffers_reach_no_library(scheme, no_library):
    """A destination one row into its source; an lm a word short; a payload a row short; side
    buffers on the CPU."""
    import torch
    from codec_tcc_amd.pee import PeeCodec, PeeEncoded, PeeVolume
    codec = PeeCodec(RB, RH, RW, dtype="uint16", T=2, scheme=scheme)
    g = _good(torch, codec, scheme)
    a, b = _overlapping(torch)
    short_lm = torch.zeros(tuple(g["lm"].shape[:-1]) + (codec.lm_words - 1,), dtype=torch.int64, device="cuda")
    assert codec.lm_words > 1 and short_lm.shape[-1] == codec.lm_words - 1   # one word too few
    auto2 = PeeCodec(RB, RH, RW, dtype="uint16", T="auto", tmax=4, scheme=2) if scheme == 2 else None
    no_library()
    with pytest.raises(ValueError, match="^stego overlaps covers"):
        codec.embed(a, None, stego=b, packed=g["packed"])
    with pytest.raises(ValueError, match="^stego overlaps covers"):
        codec.embed(b, [b"a"] * RB, stego=a, checksum=True)
    with pytest.raises(ValueError, match="^cover overlaps stego"):
        codec.extract(a, g["meta"], g["lm"], payload_words=2, cover=b)
    with pytest.raises(ValueError, match="^lm must be"):
        codec.embed(g["pix"], None, lm=short_lm, packed=g["packed"], checksum=True)
    with pytest.raises(ValueError, match="^lm must be"):
        codec.extract(g["pix"], g["meta"], short_lm, payload_words=2)
    with pytest.raises(ValueError, match="^meta must be"):
        codec.embed(g["pix"], None, meta=g["meta"][..., :-1], packed=g["packed"])
    with pytest.raises(ValueError, match="^payload must be"):
        codec.extract(g["pix"], g["meta"], g["lm"], payload_words=2,
                      payload=torch.zeros((RB - 1, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match=r"^packed\[0\] must be"):
        codec.embed(g["pix"], None, packed=(g["packed"][0][:RB - 1],) + g["packed"][1:])
    with pytest.raises(TypeError, match="^lm is on cpu"):
        codec.extract(g["pix"], g["meta"], g["lm"].cpu(), payload_words=2)
    with pytest.raises(TypeError, match=r"^packed\[2\] is on cpu"):
        codec.embed(g["pix"], None, packed=g["packed"][:2] + (g["packed"][2].cpu(),))
    enc = PeeEncoded(stego=g["pix"], lm=short_lm, meta=g["meta"], lengths=[0] * RB, payload_words=2, config=codec.config,
                     scheme=scheme)
    with pytest.raises(ValueError, match="^lm must be"):
        codec.decode(enc)
    if scheme == 1:
        with pytest.raises(ValueError, match="^stego overlaps covers"):
            codec.embed_volume(a, b"abc", stego=b)
        with pytest.raises(ValueError, match="^lm must be"):
            codec.decode_volume(PeeVolume(enc=enc, total_bits=24, policy="even", plan=None, info=None))
        with pytest.raises(TypeError, match=r"^packed\[0\] is on cpu"):
            codec.embed_volume(g["pix"], None, packed=(torch.zeros(1, dtype=torch.int64), 24))
        lm, side = codec.volume_buffers()
        with pytest.raises(ValueError, match="volume_buffers"):
            codec.embed_volume(g["pix"], b"abc", buffers=(lm[:, :-1], side), checksum=True)
    else:   # scheme 2 with T="auto" keeps its own in-place refusal, now ahead of the checksum launch
        with pytest.raises(ValueError, match="out of place only"):
            auto2.embed(g["pix"], [b"a"] * RB, stego=g["pix"], checksum=True)


def test_rejected_convenience_entries_reach_no_library(no_library):
    """pee.encode / encode_volume with a CPU torch tensor (numpy arrays are uploaded, tensors are
    taken where they are) and quality.moments with one image on the CPU."""
    import torch
    from codec_tcc_amd import pee, quality
    cpu = torch.zeros((RB, RH, RW), dtype=torch.uint16)
    gpu = cpu.cuda()
    no_library()
    with pytest.raises(TypeError, match="^covers is on cpu"):
        pee.encode(cpu, [b"a"] * RB)
    with pytest.raises(TypeError, match="^covers is on cpu"):
        pee.encode(cpu[0], [b"a"], scheme=2, T="auto")
    with pytest.raises(TypeError, match="^covers is on cpu"):
        pee.encode_volume(cpu, b"abc")
    for a, b in ((cpu, gpu), (gpu, cpu), (cpu, cpu)):
        with pytest.raises(TypeError, match="on a GPU, got cpu"):
            quality.moments(a, b)
    with pytest.raises(TypeError, match="on a GPU"):
        quality.moments(gpu.cpu().numpy(), gpu)


def test_rejected_lsb_buffers_reach_no_library(no_library):
    """Codec (LSB): the pixel rules for stego= and cover= as for the covers, and maps / meta /
    payload on the codec's device, of the element size, contiguous and large enough."""
    import torch
    from codec_tcc_amd import Codec, _lib
    from codec_tcc_amd.codec import make_payloads
    codec = Codec(RB, RH, RW, dtype="uint16")
    pl = make_payloads([b"ab"] * RB, codec.device)
    pix = torch.zeros((RB, RH, RW), dtype=torch.uint16, device="cuda")
    maps = torch.zeros((RB, pl.map_words), dtype=torch.int64, device="cuda")
    meta = torch.zeros((RB, _lib.META_BYTES), dtype=torch.uint8, device="cuda")
    kw = dict(payload_words=pl.payload_words, map_words=pl.map_words)
    no_library()
    for kind in ("cpu", "strided", "crop"):
        bad, exc = _bad_pixels(torch, kind)
        with pytest.raises(exc, match="^covers"):
            codec.encode(bad, pl)
        with pytest.raises(exc, match="^stego"):
            codec.encode(pix, pl, stego=bad)
        with pytest.raises(exc, match="^stego"):
            codec.decode(bad, maps, meta, **kw)
        with pytest.raises(exc, match="^cover"):
            codec.decode(pix, maps, meta, cover=bad, **kw)
    with pytest.raises(ValueError, match="^maps must be"):
        codec.encode(pix, pl, maps=maps[:RB - 1])
    with pytest.raises(ValueError, match="^maps must be"):
        codec.decode(pix, maps.to(torch.int32), meta, **kw)
    with pytest.raises(ValueError, match="^meta must be"):
        codec.encode(pix, pl, meta=meta[:, :-1])
    with pytest.raises(ValueError, match="^meta must be"):
        codec.decode(pix, maps, meta[:RB - 1], **kw)
    with pytest.raises(TypeError, match="^meta is on cpu"):
        codec.decode(pix, maps, meta.cpu(), **kw)
    with pytest.raises(ValueError, match="^payload must be"):
        codec.decode(pix, maps, meta, payload=torch.zeros((RB - 1, pl.payload_words), dtype=torch.int64, device="cuda"),
                     **kw)
