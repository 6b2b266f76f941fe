"""Blind volume payloads without a GPU: the spec tests/pee_blind_volume_spec.py against its scalar
restatement of the new parts (transform, plan, frame, order, tiling, missing) against the known
answers tests/golden/pee_blind_volume_kat.json, on every case of tests/pee_blind_volume_cases.py;
the spec's own round trip in any slice order; the conditions the GPU test's stacks must meet; the
downward closure that makes a T exist for every carrier; the argument refusals of
codec_tcc_amd/blind_volume.py and the header rules of blind.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import pee_blind_spec as BS
import pee_blind_volume_cases as VC
import pee_blind_volume_spec as VS
from codec_tcc_amd import blind, blind_volume

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(s, B, pol) for s in VC.SHAPES for B in VC.BATCHES for pol in VC.POLICIES]


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "pee_blind_volume_kat.json")) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


@pytest.mark.parametrize("shape,B,policy", CASES)
def test_spec_scalar_and_known_answers_agree(shape, B, policy, kat):
    """plan, frames, T and stego of the spec, the scalar restatement and the known answers agree at
    N = 1, two thirds of the capacity, the capacity (fits) and one bit more (refused, stack unchanged);
    a planned stack decodes, reversed, to the stream and the covers"""
    covers, curve = VC.stack(shape, B), VC.curve(shape, B)
    known = {k["length"]: k for k in kat["cases"] if (k["shape"], k["B"], k["policy"]) == (shape, B, policy)}
    assert sorted(known) == sorted(VC.LENGTH_NAMES) and kat["volume_id"] == VC.VOLUME_ID
    assert VS.transform(curve).tolist() == VS.transform_scalar(curve.tolist())
    for which in VC.LENGTH_NAMES:
        k, bits = known[which], VC.bits(shape, B, which)
        N = int(bits.size)
        res = VC.result(shape, B, policy, which)
        p, ps = res["plan"], VS.plan_scalar(curve.tolist(), N, policy)
        assert (k["N"], k["cover_sha256"], k["curve_sha256"]) == (N, _sha(covers), _sha(curve.tolist()))
        for key in ("status", "T", "capacity", "capacity_max", "carriers"):
            assert p[key] == ps[key] == k[key], (which, key)
        assert p["n"].tolist() == ps["n"] == k["n"] and p["off"].tolist() == ps["off"] == k["off"]
        assert int(p["n"].sum()) == (0 if p["status"] else N)
        crc = VS.stream_crc(bits)
        assert crc == k["stream_crc"]
        for b in range(B):
            if p["n"][b] == 0:
                assert res["frames"][b] == [0] * 6 == k["frames"][b] and res["ts"][b] == 0
                assert res["info"][b] == VS.SKIPPED_INFO
                np.testing.assert_array_equal(res["stego"][b], covers[b])
                continue
            assert [int(v) for v in res["frames"][b]] == k["frames"][b]
            assert BS.words_to_bits(res["frames"][b]).tolist() == VS.frame_bits_scalar(VC.VOLUME_ID, b, B, int(p["off"][b]), N,
                                                                                       crc)
            w = [int(v) for v in BS.read_words(res["stego"][b], 0, 3)]
            assert (w[1] >> 8) & 0xFF == VS.FLAG_VOLUME | BS.FLAG_CRC and w[2] == 192 + p["n"][b] == res["info"][b][1]
            assert w[1] & 0xFF == res["ts"][b] >= 1 and curve[b][res["ts"][b] - 1] >= 192 + p["n"][b]
        assert res["ts"] == k["ts"] and _sha(res["stego"]) == k["stego_sha256"]
        if which == "over":
            assert p["status"] == 1 and N == p["capacity_max"] + 1
            np.testing.assert_array_equal(res["stego"], covers)
            continue
        assert p["status"] == 0 and (which != "fits" or N == p["capacity"] == p["capacity_max"])
        got, back, o = VS.decode(res["stego"][::-1])
        np.testing.assert_array_equal(got, bits)
        np.testing.assert_array_equal(back, covers[::-1])
        assert o["status"] == 0 and o["crc"] == crc


def test_order_scenarios(kat):
    """order() against order_scalar() against the known answers: complete, gaps, duplicate, mixed,
    none, overlap, an index past B"""
    want = {"complete_reversed": 0, "dropped_3": 4, "dropped_first_and_last": 4, "duplicate_3": 3, "mixed": 2, "none": 1,
            "overlap": 3, "index_past_B": 3}
    assert {o["scenario"]: o["status"] for o in kat["orders"]} == want
    for o in kat["orders"]:
        got = VS.order(o["frames"], o["n"])
        status, missing = VS.order_scalar(o["frames"], o["n"])
        assert got["status"] == status == o["status"], o["scenario"]
        assert [list(m) for m in got["missing"]] == [list(m) for m in missing] == o["missing"], o["scenario"]
        table = [(f[1], f[3], n, 1) for f, n in zip(o["frames"], o["n"])]
        if status in (0, 4):   # the codec's host statement of the ranges
            assert [list(m) for m in blind_volume.missing_ranges(table, o["frames"][0][4])] == o["missing"]
    two = next(o for o in kat["orders"] if o["scenario"] == "dropped_first_and_last")
    assert len(two["missing"]) == 2 and two["missing"][0][0] == 0 and two["missing"][1][1] == two["frames"][0][4]


def test_spec_decode_any_order_and_refusals():
    covers, bits = VC.stack("u16", 9), VC.bits("u16", 9, "most")
    res = VC.result("u16", 9, "even", "most")
    st, p = res["stego"], res["plan"]
    perm = [4, 8, 0, 7, 1, 3, 6, 2, 5]
    got, back, _o = VS.decode(st[perm])
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back, covers[perm])
    extra = np.concatenate([st[perm], VS.stack(3, 64, 96, seed=700)])
    got, back, _o = VS.decode(extra)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back[9:], extra[9:])
    keep = [b for b in range(9) if b != 3]
    with pytest.raises(ValueError, match="status 4"):
        VS.decode(st[keep])
    got, _back, o = VS.decode(st[keep], partial=True)
    lo, hi = int(p["off"][3]), int(p["off"][3] + p["n"][3])
    assert o["missing"] == [(lo, hi)] and not got[lo:hi].any()
    np.testing.assert_array_equal(np.delete(got, np.s_[lo:hi]), np.delete(bits, np.s_[lo:hi]))
    dup = st.copy()
    dup[4] = st[3]
    with pytest.raises(ValueError, match="status 3"):
        VS.decode(dup)
    with pytest.raises(ValueError, match="status 1"):
        VS.decode(covers)
    plain = BS.embed(covers[0], bits[:100], 4, 4095)[0]
    with pytest.raises(ValueError, match="no volume slice"):
        VS.decode(np.concatenate([st, plain[None]]))
    with pytest.raises(ValueError, match="flags"):   # the fixed-T spec keeps refusing the flag
        BS.decode(st[0])


def test_stacks_meet_their_conditions():
    """carrier counts, a non-carrier in every stack, all slices different, both routes' widths"""
    for shape, (h, w, _dt, _mv, _tmax) in VC.SHAPES.items():
        assert (w % 8 == 0) == (shape != "odd")
        for B in VC.BATCHES:
            covers, c = VC.stack(shape, B), VS.transform(VC.curve(shape, B))
            assert len({covers[b].tobytes() for b in range(B)}) == B
            assert (VC.curve(shape, B)[1] == -1).all() and (c[1] == 0).all()         # the checkerboard: below a frame at any T
            assert (c[:, -1] > 0).sum() == B - 1
            L = VC.lengths(shape, B)
            assert 1 < L["most"] < L["fits"] == c[:, -1].sum() and L["over"] == L["fits"] + 1
            for pol in VC.POLICIES:
                p = VC.result(shape, B, pol, "most")["plan"]
                assert 2 <= p["carriers"] <= B - 1 and p["n"][1] == 0
                assert VC.result(shape, B, pol, "one")["plan"]["carriers"] == 1
                assert VC.result(shape, B, pol, "fits")["plan"]["carriers"] == B - 1
    even, fill = (VC.result("u16", 9, pol, "most")["plan"] for pol in VC.POLICIES)
    assert even["n"].tolist() != fill["n"].tolist() and fill["carriers"] < even["carriers"]
    assert len(set(VC.result("u16", 9, "even", "most")["ts"])) >= 3   # T differs from slice to slice


def test_status_zero_lengths_are_downward_closed():
    """By brute force on the cases' slices: at each T, the lengths whose blind plan has status 0 are
    exactly 0..capacity(T) -- so a share n_b <= c_b always finds a T (its T* at the latest)."""
    seen = 0
    for shape, B in (("u16", 3), ("u8", 3), ("odd", 9)):
        _h, _w, _dt, mv, tmax = VC.SHAPES[shape]
        for b, cover in enumerate(VC.stack(shape, B)):
            for T in (1, 2, tmax // 2, tmax):
                cap = BS.capacity(cover, T, mv)
                ok = [BS.plan(cover, n, T, mv)["status"] == 0 for n in range(0, max(cap, 0) + 40)]
                assert ok == [n <= cap for n in range(len(ok))], (shape, b, T, cap)
                seen += 1
    assert seen == 60


def test_argument_refusals():
    ok = dict(scheme=1, tmax=8, gate=None, B=6, H=64, W=96, maxval=4095, nbits=100)
    blind_volume.check_args(**ok)
    blind_volume.check_args(**{**ok, "B": 65535, "H": 16, "W": 16, "nbits": 2 ** 31 - 1, "volume_id": 2 ** 32 - 1})
    for change, text in ((dict(key=b"k" * 32), "key"), (dict(gate=3), "gate"), (dict(scheme=2), "scheme 1"),
                         (dict(in_place=True), "out of place"), (dict(nbits=0), "1 .. 2"), (dict(nbits=2 ** 31), "1 .. 2"),
                         (dict(B=65536, H=16, W=16), "65535"), (dict(B=0), "65535"), (dict(tmax=17), "tmax"),
                         (dict(tmax=0), "tmax"), (dict(policy="odd"), "policy"), (dict(roi=(0, 0, 4, 4)), "roi"),
                         (dict(volume_id=-1), "volume_id"), (dict(volume_id=2 ** 32), "volume_id"),
                         (dict(volume_id=1.5), "volume_id"), (dict(B=65535, H=512, W=512), "2\\^31"),
                         (dict(max_entries=-1), "max_entries"), (dict(H=8, W=16), "header bits")):
        with pytest.raises(ValueError, match=text):
            blind_volume.check_args(**{**ok, **change})
    import codec_tcc_amd as pkg
    cover = np.array(VC.stack("u16", 3))
    for kw in (dict(tmax=0), dict(policy="odd"), dict(volume_id=-1), dict(max_entries=-1)):
        with pytest.raises(ValueError):   # before the GPU is asked for: this runs without one
            pkg.encode_blind_volume(cover, b"x", **kw)
    with pytest.raises(ValueError):
        pkg.encode_blind_volume(cover, b"")
    with pytest.raises(ValueError):
        pkg.encode_blind_volume(cover[0], b"x")
    assert {"encode_blind_volume", "decode_blind_volume"} <= set(pkg.__all__)
    assert (blind_volume.FLAG_VOLUME, blind_volume.FRAME_BITS, blind_volume.SKIPPED) == (VS.FLAG_VOLUME, VS.FRAME_BITS,
                                                                                          VS.SKIPPED)
    assert blind_volume.stream_crc(VC.bits("u16", 3, "most")) == VS.stream_crc(VC.bits("u16", 3, "most"))


def test_header_rules():
    """parse_header(s): the default and keyed=True refuse the volume flag; volume=True takes bit 2
    with or without bit 0, refuses a plain, a keyed and a frameless header"""
    res = VC.result("u16", 3, "even", "most")
    st = res["stego"][0]
    w = [int(v) for v in BS.read_words(st, 0, 6)]
    h = blind.parse_header(w, 64, 96, 65535, volume=True)
    assert h["flags"] == 5 and h["n_user"] == 192 + res["plan"]["n"][0] and h["T"] == res["ts"][0]
    with pytest.raises(ValueError, match="flags = 0x5"):
        blind.parse_header(w, 64, 96, 65535)
    with pytest.raises(ValueError, match="flags = 0x5"):
        blind.parse_header(w, 64, 96, 65535, keyed=True)
    for flags, ok in ((4, True), (5, True), (0, False), (1, False), (6, False), (7, False), (12, False)):
        w2 = list(w)
        w2[1] = (w[1] & ~0xFF00) | (flags << 8)
        if ok:
            blind.parse_header(w2, 64, 96, 65535, volume=True)
        else:
            with pytest.raises(ValueError, match="flags"):
                blind.parse_header(w2, 64, 96, 65535, volume=True)
    w3 = list(w)
    w3[2] = 191
    with pytest.raises(ValueError, match="192 frame bits"):
        blind.parse_header(w3, 64, 96, 65535, volume=True)
    hdr = np.array([w + [0, 0], w3 + [0, 0]], dtype=np.uint32)
    with pytest.raises(ValueError, match=r"volume blind MED-PEE header in slices \[1\]"):
        blind.parse_headers(hdr, 64, 96, 2, volume=True)
    got = blind.parse_headers(hdr[:1], 64, 96, 2, volume=True)
    assert int(got["n_user"][0]) == h["n_user"] and int(got["L"][0]) == h["L"]
    with pytest.raises(ValueError, match=r"slices \[0\]"):
        blind.parse_headers(hdr[:1], 64, 96, 2)
