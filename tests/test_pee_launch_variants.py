"""Every kernel instantiation codec_pee.hip's dispatch can reach through a knob, run once.

The dispatch names 186 kernel instantiations.  Many sit behind A/B knobs no other test sets
(CODEC_NT is one: every NT = false instance), so a mistyped template argument or argument list
there would pass the rest of the suite.  Each case below sets one knob combination, runs embed
and extract once at a small shape and compares stego, location map and record status / end / T
with oracle/pee_cpu.py (as test_pee.py::test_gpu_matches_oracle does), and the extracted
payload and the restored cover with the inputs.  Each case also opens a profiling window
(codec_profile_begin) around its two calls and asserts that the launch families recorded there
(_lib.KERNEL_TAGS, one tag per route) are exactly the route's: a knob that stopped reaching its
route would fall back to another family and fail here.  The tags name the family, not the
template arguments; inside a family those follow from the same knobs by the dispatch's text.

Shape: B = 2, H = 67, W = 264.  W % 8 == 0 admits the vector routes; 33 x 33 = 1089 items are two
1024-item chunks, the second ragged; the odd H exercises the last-row copy.  Slice 0 carries a
payload of about half its capacity, slice 1 none.  B = 2 is far from filling the chip, so
CODEC_PEE_SS=1 / CODEC_PEE_LAT_SS=1 force the slice-serial routes and CODEC_PEE_FLAT_MAXB=0 the
lane look-back.  k_pee_restore_gs needs items % 256 == 0 and the resident kernel's other
launches larger slices: those cases name their own shape.

Instantiation -> the case (here) or test (elsewhere) that reaches it.  "TT" = uint16_t and
uint8_t, "IP" = in place and out of place, both run.

  scheme 1, fixed T (test_fixed_T)
    k_pee_embed1 / k_pee_extract1<TT, false, false, SC=true>     nt0            (out of place, flat)
    k_pee_embed1 / k_pee_extract1<TT, false, true, false>        nt0            (in place)
    k_pee_embed1 / k_pee_extract1<TT, false, false, false>       nt0_lanes
    k_pee_extract1<TT, false, ...> behind CODEC_PEE_X_NT         xnt0           (the embed stays NT)
    k_pee_scan<TT, false, false>, k_pee_copy<TT, false>          nt0_twopass    (+ dcount, recover)
    k_pee_restore_gs<TT, false, false>                           nt0_twopass_gs (2 x 64 x 256)
    k_pee_embed_ss<TT, false, IP, 4, true>, k_pee_extract_ss<TT, false, IP, 4>      nt0_ss
    k_pee_embed_ss<TT, false, IP, 4, false>                      nt0_ss_gpay
    k_pee_embed_ss<u16, NTL, true, 1, true, false, NTS>, k_pee_extract_ss<u16, NTL, true, 1, true, NTS>
        (NTL, NTS) = (1,1) ss_ip_ntl1_nts1, (0,1) ss_ip_ntl0_nts1, (0,0) ss_ip_ntl0_nts0;
        (1,0) is the default: test_pee.py PATHS["slice_serial"], in place
    k_pee_embed_ss<u16, true, true, 2, true>                     ss_d2
    k_pee_extract_ss<u16, true, false, 2> (late ring of 2), <u16, true, true, 4>    ss_xlate
    k_pee_extract_ss<u16, true, true, 2>, <u16, true, true, 6>   ss_xlate_d2, ss_xlate_d6 (in place)
    k_pee_extract_ss<u16, true, false, D, EARLY>, D = 1, 2, 4    ss_xearly_d1 / _d2 / _d4
    k_pee_extract_ss<u16, true, true, 2, EARLY>                  ss_xearly_d2 (in place)
    every NT = true instance of the above families, k_pee_extract_ss<u16, true, false, 6>,
    <u16, true, true, 4, EARLY>, the non-vector tile kernels (k_pee_count, k_pee_embed<TT, false>,
    k_pee_dcount<TT, false>, k_pee_recover<TT, false>), k_pee_embed_v, k_pee_dcount_w,
    k_pee_dcount<TT, true>, k_pee_embed<TT, true>: test_pee.py PATHS x test_gpu_matches_oracle
    the GATE = true instances (NT only): test_pee_gate.py (its knob sets cover one pass, two
    passes with and without CODEC_PEE_FUSED / _EMBED_V / _WAVE_TILES); at batches of several slot
    groups with a ragged last lane: test_pee_batch_dispatch.py (no knob)
  scheme 1, T = "auto" (test_auto_T)
    k_pee_embed_res<NI, NT, NTS, NTH, LIN> for the seven (NI, NTH, LIN) launches, with
        (NT, NTS) = (true, true): res_nts_*, (false, false): res_nt0_*; (true, false) is the
        default: test_pee.py::test_gpu_embed_auto_fused_edges
        (8, 1024, no) base shape; (8, 512, no) base shape, CODEC_PEE_RES_THREADS=512;
        (8, 1024, LIN) 2 x 256 x 512; (16, 512, no) the same with 512 threads;
        (16, 1024, LIN) 2 x 512 x 512; (16, 1024, no) the same with CODEC_PEE_RES_LIN=0;
        (32, 512, no) the same with 512 threads
    k_pee_embed_ss<u16, false, true, 2, true, AUTO>, <u16, false, false, 4, true, AUTO>   auto_ss_nt0
    the NT = true AUTO instances and k_pee_ehist: test_gpu_embed_auto_fused_edges, test_gpu_capacity_control
  scheme 2 (test_scheme2)
    k_pee_lat_ss<TT, EXTRACT, false, true>                       lat_ss_gpay
    k_pee_lat_ss<u16, EXTRACT, true, false>                      lat_ss_nopf (uint8: the knob is ignored)
    k_pee_lat_ss with the copy and pass 0 in the launch          lat_ss_p0
    k_pee_lat_ss<TT, EXTRACT, true, true>, the lattice tile kernels, k_pee_pass0_fix: test_pee.py
    (test_gpu_multipass_*); k_pee_lat_auto<TT, PL>: test_pee2_auto.py (PL follows the payload
    row length, no knob)

Not reachable by any knob: none found.  Two sites are reached by more than one setting and
launch the same instance: CODEC_PEE_SSX_D=6 in place with early refill runs the ring of 4, and
k_pee_extract_ss<u16, true, true, 1, true, true> is both "early ring of one, NTS = NTL = 1" and
what a plain early ring of one would name.
"""
import functools

import numpy as np
import pytest

from codec_tcc_amd import synth
from oracle import pee_cpu as P

from pee_launches import launches as _launches
from test_pee import _bits, _check_multi_vs_oracle

BASE = (2, 67, 264)
TMAX = 8
SS = {"CODEC_PEE_SS": "1"}
U16 = ("uint16",)

# name -> (knobs, dtypes, placements (True = in place), shape)
FIXED = {
    "nt0": ({"CODEC_NT": "0"}, ("uint16", "uint8"), (False, True), BASE),
    "nt0_lanes": ({"CODEC_NT": "0", "CODEC_PEE_FLAT_MAXB": "0"}, ("uint16", "uint8"), (False, True), BASE),
    "nt0_twopass": ({"CODEC_NT": "0", "CODEC_PEE_ONEPASS": "0"}, ("uint16", "uint8"), (False, True), BASE),
    "nt0_twopass_gs": ({"CODEC_NT": "0", "CODEC_PEE_ONEPASS": "0"}, ("uint16", "uint8"), (False, True), (2, 64, 256)),
    "nt0_ss": ({"CODEC_NT": "0", **SS}, ("uint16", "uint8"), (False, True), BASE),
    "nt0_ss_gpay": ({"CODEC_NT": "0", "CODEC_PEE_SS_PAYLDS": "0", **SS}, ("uint16", "uint8"), (False, True), BASE),
    "xnt0": ({"CODEC_PEE_X_NT": "0"}, ("uint16", "uint8"), (False, True), BASE),
    "ss_ip_ntl1_nts1": ({"CODEC_PEE_IP_NTL": "1", "CODEC_PEE_IP_NTS": "1", **SS}, ("uint16",), (True,), BASE),
    "ss_ip_ntl0_nts1": ({"CODEC_PEE_IP_NTL": "0", "CODEC_PEE_IP_NTS": "1", **SS}, ("uint16",), (True,), BASE),
    "ss_ip_ntl0_nts0": ({"CODEC_PEE_IP_NTL": "0", "CODEC_PEE_IP_NTS": "0", **SS}, ("uint16",), (True,), BASE),
    "ss_d2": ({"CODEC_PEE_SS_D": "2", **SS}, ("uint16",), (True,), BASE),
    "ss_xlate": ({"CODEC_PEE_SSX_EARLY": "0", **SS}, ("uint16",), (False, True), BASE),
    "ss_xlate_d2": ({"CODEC_PEE_SSX_EARLY": "0", "CODEC_PEE_SSX_D": "2", **SS}, ("uint16",), (True,), BASE),
    "ss_xlate_d6": ({"CODEC_PEE_SSX_EARLY": "0", "CODEC_PEE_SSX_D": "6", **SS}, ("uint16",), (True,), BASE),
    "ss_xearly_d1": ({"CODEC_PEE_SSX_EARLY": "1", "CODEC_PEE_SSX_D": "1", **SS}, ("uint16",), (False,), BASE),
    "ss_xearly_d2": ({"CODEC_PEE_SSX_EARLY": "1", "CODEC_PEE_SSX_D": "2", **SS}, ("uint16",), (False, True), BASE),
    "ss_xearly_d4": ({"CODEC_PEE_SSX_EARLY": "1", "CODEC_PEE_SSX_D": "4", **SS}, ("uint16",), (False,), BASE),
}

NTS = {"CODEC_PEE_RES_NTS": "1", **SS}
NT0 = {"CODEC_NT": "0", **SS}
T512 = {"CODEC_PEE_RES_THREADS": "512"}
AUTO = {
    "res_nts": (NTS, U16, (False,), BASE),
    "res_nt0": (NT0, U16, (False,), BASE),
    "res_nts_512": ({**NTS, **T512}, U16, (False,), BASE),
    "res_nt0_512": ({**NT0, **T512}, U16, (False,), BASE),
    "res_nts_lin8": (NTS, U16, (False,), (2, 256, 512)),
    "res_nt0_lin8": (NT0, U16, (False,), (2, 256, 512)),
    "res_nts_512x16": ({**NTS, **T512}, U16, (False,), (2, 256, 512)),
    "res_nt0_512x16": ({**NT0, **T512}, U16, (False,), (2, 256, 512)),
    "res_nts_lin16": (NTS, U16, (False,), (2, 512, 512)),
    "res_nt0_lin16": (NT0, U16, (False,), (2, 512, 512)),
    "res_nts_nolin16": ({**NTS, "CODEC_PEE_RES_LIN": "0"}, U16, (False,), (2, 512, 512)),
    "res_nt0_nolin16": ({**NT0, "CODEC_PEE_RES_LIN": "0"}, U16, (False,), (2, 512, 512)),
    "res_nts_512x32": ({**NTS, **T512}, U16, (False,), (2, 512, 512)),
    "res_nt0_512x32": ({**NT0, **T512}, U16, (False,), (2, 512, 512)),
    "auto_ss_nt0": ({**NT0, "CODEC_PEE_RES": "0"}, U16, (False, True), BASE),
}

LSS = {"CODEC_PEE_LAT_SS": "1"}
SCHEME2 = {
    "lat_ss_gpay": ({"CODEC_PEE_LAT_SS_PL": "0", **LSS}, ("uint16", "uint8"), (False, True), BASE),
    "lat_ss_nopf": ({"CODEC_PEE_LAT_SS_PF": "0", **LSS}, ("uint16", "uint8"), (False, True), BASE),
    "lat_ss_p0": ({"CODEC_PEE_LAT_SS_P0": "0", **LSS}, ("uint16", "uint8"), (False, True), BASE),
}


# the launch families a case's embed + extract must record, and no others
LOOKBACK = {"k_pee_embed1", "k_pee_extract1"}
SLICE_SERIAL = {"k_pee_embed_ss", "k_pee_extract_ss"}
TWOPASS = {"k_pee_scan", "k_pee_locate", "k_pee_embed", "k_pee_copy", "k_pee_dcount", "k_pee_recover"}
ROUTES = {"nt0": LOOKBACK, "nt0_lanes": LOOKBACK, "xnt0": LOOKBACK, "nt0_twopass": TWOPASS,
          "nt0_twopass_gs": TWOPASS - {"k_pee_copy"},   # k_pee_restore_gs copies and recovers in one launch
          **{name: SLICE_SERIAL for name in FIXED if name.startswith("ss_") or name.startswith("nt0_ss")},
          **{name: {"k_pee_embed_res", "k_pee_extract_ss"} for name in AUTO if name.startswith("res_")},
          "auto_ss_nt0": {"k_pee_embed_ss_auto", "k_pee_extract_ss"},
          # pass 0 through scheme 1's embed (look-back at B = 2), then the slice-serial launch
          "lat_ss_gpay": {"k_pee_embed1", "k_pee_lat_ss_embed", "k_pee_lat_ss_extract"},
          "lat_ss_nopf": {"k_pee_embed1", "k_pee_lat_ss_embed", "k_pee_lat_ss_extract"},
          "lat_ss_p0": {"k_pee_lat_ss_embed", "k_pee_lat_ss_extract"}}


def _cases(table):
    return [pytest.param(knobs, dt, ip, shape, ROUTES[name], id=f"{name}-{dt}-{'ip' if ip else 'oop'}")
            for name, (knobs, dtypes, places, shape) in table.items() for dt in dtypes for ip in places]


@functools.lru_cache(maxsize=None)
def _covers(dtype, shape):
    bsz, h, w = shape
    covers = np.stack([synth.GENERATORS["ct12" if dtype == "uint16" else "u8"](h, w, 610 + i) for i in range(bsz)])
    covers.setflags(write=False)
    return covers


@functools.lru_cache(maxsize=None)
def _fixed_ref(dtype, shape, T):
    """covers, payloads (slice 0 half its capacity, the others empty), the oracle's (stego, side) per slice"""
    covers = _covers(dtype, shape)
    payloads = [_bits(P.capacity(covers[0], T) // 2 if i == 0 else 0, 620 + i) for i in range(shape[0])]
    return covers, payloads, [P.pee_embed(c, p, T) for c, p in zip(covers, payloads)]


@functools.lru_cache(maxsize=None)
def _auto_ref(shape):
    covers = _covers("uint16", shape)
    half = int(P.capacity_curve(covers[0], TMAX)[-1]) // 2
    payloads = [_bits(half if i == 0 else 0, 630 + i) for i in range(shape[0])]
    ts = [P.select_T(c, len(p), TMAX) for c, p in zip(covers, payloads)]
    return covers, payloads, ts, [P.pee_embed(c, p, t, truncate=True) for c, p, t in zip(covers, payloads, ts)]


def _run_scheme1(codec, covers, payloads, refs, ts, inplace, route):
    """embed + extract once; everything test_gpu_matches_oracle compares, each record's T and
    the launch families"""
    import torch
    from codec_tcc_amd import _lib, framing
    from codec_tcc_amd.pee import lm_bits
    dev = torch.from_numpy(covers.copy()).cuda()
    seen = set()
    with _launches(seen):
        enc = codec.embed(dev, payloads, stego=dev if inplace else None)
    recs = enc.records()
    stego = enc.stego.cpu().numpy()
    for i, (st, side) in enumerate(refs):
        assert (recs[i].status, recs[i].end, recs[i].T) == (side["status"], side["end"], ts[i]), i
        if recs[i].flags & _lib.PEE_PARTIAL:
            assert side["L"] <= recs[i].capacity <= side["capacity"], i
        else:
            assert recs[i].capacity == side["capacity"], i
        np.testing.assert_array_equal(stego[i], st)
        np.testing.assert_array_equal(lm_bits(enc, i), side["lm"])
        assert recs[i].lm_count == int(side["lm"].sum()), i
    with _launches(seen):
        words, cover = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words,
                                     cover=enc.stego if inplace else None)
    assert seen == route
    host = words.cpu().numpy()
    for i, bits in enumerate(payloads):   # side["L"] = len(bits) but on a slice that overflowed (status 1)
        n = refs[i][1]["L"]
        assert n == len(bits) or refs[i][1]["status"] == 1, i
        np.testing.assert_array_equal(framing.unpack_bits(host[i], n), bits[:n])
    np.testing.assert_array_equal(cover.cpu().numpy(), covers)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,dtype,inplace,shape,route", _cases(FIXED))
def test_fixed_T(knobs, dtype, inplace, shape, route, monkeypatch):
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    T = 2
    covers, payloads, refs = _fixed_ref(dtype, shape, T)
    assert len(payloads[0]) > 0 and refs[0][1]["status"] == 0
    codec = PeeCodec(*shape, dtype=dtype, T=T)
    _run_scheme1(codec, covers, payloads, refs, [T] * shape[0], inplace, route)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,dtype,inplace,shape,route", _cases(AUTO))
def test_auto_T(knobs, dtype, inplace, shape, route, monkeypatch):
    pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    covers, payloads, ts, refs = _auto_ref(shape)
    assert 1 < ts[0] <= TMAX and ts[1] == 1
    codec = PeeCodec(*shape, dtype=dtype, T="auto", tmax=TMAX)
    _run_scheme1(codec, covers, payloads, refs, ts, inplace, route)
    assert codec.t_slices.cpu().tolist() == ts


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,dtype,inplace,shape,route", _cases(SCHEME2))
def test_scheme2(knobs, dtype, inplace, shape, route, monkeypatch):
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    T = 2
    covers = _covers(dtype, shape)
    mv = int(np.iinfo(covers.dtype).max)
    # about half of what the four passes hold: pass 0 full, the payload ends in a later pass
    bits_list = [_bits(2 * P.capacity(covers[0], T, mv) if i == 0 else 0, 640 + i) for i in range(shape[0])]
    codec = PeeCodec(*shape, dtype=dtype, T=T, maxval=mv, scheme=2)
    cov_t = torch.from_numpy(covers.copy()).cuda()
    work = cov_t.clone() if inplace else None
    seen = set()
    with _launches(seen):
        enc = codec.embed(work if inplace else cov_t, bits_list, stego=work)
    _check_multi_vs_oracle(enc, covers, bits_list, T, mv)
    assert enc.embedded()[0] == len(bits_list[0])
    out = enc.stego.clone() if inplace else None
    with _launches(seen):
        words, cover = codec.extract(out if inplace else enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words,
                                     cover=out)
    assert seen == route
    host = words.cpu().numpy()
    for i, bits in enumerate(bits_list):
        np.testing.assert_array_equal(framing.unpack_bits(host[i], len(bits)), bits)
    np.testing.assert_array_equal(cover.cpu().numpy(), covers)
