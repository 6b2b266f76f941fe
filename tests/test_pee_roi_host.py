"""ROI-protected MED-PEE without a GPU (include/codec_tcc_roi.h): the vectorised
specification tests/pee_roi_spec.py against its scalar restatement and the known answers, the
properties the scheme promises, and the host layer -- normalize_roi, the record words,
check_records on ROI records, the argument rules of embed(..., roi=)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import pee_gate_spec as G
import pee_roi_scalar as S
import pee_roi_spec as R
from codec_tcc_amd import _lib, pee, roi

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("make_pee_roi_golden", os.path.join(HERE, "golden", "make_pee_roi_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
KAT = json.load(open(os.path.join(HERE, "golden", "pee_roi_kat.json")))["cases"]


def _sha(rows):
    return hashlib.sha256(np.asarray(rows, dtype=np.int64).tobytes()).hexdigest()


def test_kat_covers_what_it_should():
    assert 20 <= len(KAT) <= 60
    assert {c["T"] for c in KAT} == {1, 2, 4} and {c["G"] for c in KAT} == {0, 3, 65535}
    assert {c["kind"] for c in KAT} >= {"ct12", "u8", "u16"}
    assert {(c["h"] % 2, c["w"] % 2) for c in KAT} >= {(0, 0), (1, 1)}
    assert any(c["roi"] == [0, 0, 0, 0] and c["rect"] != [0, 0, 0, 0] for c in KAT)          # an empty one that normalised
    assert any(c["rect"] == [0, 0, c["h"], c["w"]] and c["nbits"] > 0 for c in KAT)           # whole image
    assert any(c["rect_name"] == "end" for c in KAT) and any(c["rule"] == "over" and c["status"] == 1 for c in KAT)
    assert any(c["rect"][0] % 2 and c["rect"][1] % 2 for c in KAT) and any(not c["rect"][0] % 2 and c["rect"][2] for c in KAT)


@pytest.mark.parametrize("i", range(len(KAT)))
def test_spec_equals_scalar_restatement_and_kat(i):
    c = KAT[i]
    img = GEN.make_image(c["kind"], c["h"], c["w"], c["seed"], c["maxval"], c["clip"])
    mv = int(np.iinfo(img.dtype).max) if c["maxval"] is None else c["maxval"]
    bits = GEN.payload_bits(c["nbits"], c["seed"])
    rect = tuple(c["rect"])
    st, side = R.embed(img, bits, c["T"], c["G"], rect, mv)
    st2, side2 = S.embed(img.astype(np.int64).tolist(), bits.tolist(), c["T"], c["G"], rect, mv)
    np.testing.assert_array_equal(st, np.asarray(st2))
    for k in ("L", "end", "capacity", "status", "lm_count"):
        assert side[k] == side2[k] == c[k], k
    assert list(side["roi"]) == list(side2["roi"]) == c["roi"]
    assert list(side["reserved"]) == list(side2["reserved"]) == c["reserved"]
    assert [bool(v) for v in side["lm"]] == side2["lm"]
    assert _sha(st.astype(np.int64).tolist()) == c["stego_sha256"]
    assert _sha([int(v) for v in side["lm"]]) == c["lm_sha256"]
    got, back = R.extract(st, side)
    np.testing.assert_array_equal(back, img)
    np.testing.assert_array_equal(got, bits[:side["L"]])
    y0, x0, y1, x1 = side["roi"]
    np.testing.assert_array_equal(st[y0:y1, x0:x1], img[y0:y1, x0:x1])
    n, hs = R.table(img, c["tmax"], rect, mv)
    n2, hs2 = S.table(img.astype(np.int64).tolist(), c["tmax"], rect, mv)
    assert n.tolist() == n2 == c["n"] and hs.tolist() == hs2 == c["hs"]
    for L, want in c["select"].items():
        assert list(R.select(n, hs, int(L))) == list(S.select(n2, hs2, int(L))) == want, L


def test_regenerating_the_kat_reproduces_the_file():
    assert GEN.build()["cases"] == KAT


def _img(seed=1, h=32, w=48):
    return GEN.make_image("ct12", h, w, seed, 4095, False)


def test_whole_image_rectangle():
    img = _img()
    nc = 16 * 24
    st, side = R.embed(img, G.payload_bits(50, 1), 2, 65535, (0, 0, 32, 48), 4095)
    np.testing.assert_array_equal(st, img)
    assert (side["capacity"], side["status"], side["end"], side["L"]) == (0, 1, nc - 1, 0)
    assert len(side["lm"]) == nc and not side["lm"].any()
    st, side = R.embed(img, [], 2, 65535, (0, 0, 32, 48), 4095)
    assert (side["end"], side["status"]) == (-1, 0)
    np.testing.assert_array_equal(st, img)


@pytest.mark.parametrize("rect", [(0, 0, 0, 0), None, (7, 3, 7, 40), (3, 9, 30, 9)])
@pytest.mark.parametrize("gate", [3, 65535])
def test_empty_rectangle_is_the_gated_embed(rect, gate):
    img = GEN.make_image("ct12", 40, 40, 3, 4095, True)
    bits = G.payload_bits(120, 2)
    st, side = R.embed(img, bits, 2, gate, rect, 4095)
    st0, side0 = G.embed(img, bits, 2, gate, 4095)
    np.testing.assert_array_equal(st, st0)
    for k in side0:
        np.testing.assert_array_equal(side[k], side0[k], err_msg=k)
    assert side["roi"] == (0, 0, 0, 0) and side["reserved"] == (0, gate + 1, 0)
    assert [v.tolist() for v in R.table(img, 8, rect, 4095)] == [v.tolist() for v in G.table(img, 8, 4095)]


def test_protected_unsafe_candidates_are_not_in_the_map():
    img = GEN.make_image("ct12", 40, 40, 3, 4095, True)     # saturated bands in rows 0..19
    _st, free = R.embed(img, G.payload_bits(10 ** 4, 3), 2, 65535, None, 4095)
    st, side = R.embed(img, G.payload_bits(10 ** 4, 3), 2, 65535, (0, 0, 21, 40), 4095)
    assert free["lm_count"] > 0 and side["lm_count"] == 0 and side["end"] == 20 * 20 - 1
    np.testing.assert_array_equal(st[:21], img[:21])


# ---------------------------------------------------------------- normalize_roi
def test_normalize_roi_accepts():
    assert roi.normalize_roi(None, 3, 10, 12) is None
    a = roi.normalize_roi((1, 2, 5, 7), 3, 10, 12)
    assert a.dtype == np.int32 and a.tolist() == [[1, 2, 5, 7]] * 3
    assert a.flags.c_contiguous and a.strides == (16, 4)      # dense row-major: the device array is uploaded as it lies
    assert roi.normalize_roi(np.asarray([[1, 2, 5, 7]] * 3).T.copy().T, 3, 10, 12).strides == (16, 4)
    a = roi.normalize_roi([[0, 0, 10, 12], [4, 4, 4, 9], [3, 5, 9, 5]], 3, 10, 12)
    assert a.tolist() == [[0, 0, 10, 12], [0, 0, 0, 0], [0, 0, 0, 0]]
    torch = pytest.importorskip("torch")
    a = roi.normalize_roi(torch.tensor([[1, 2, 3, 4]] * 2, dtype=torch.int32), 2, 10, 12)
    assert a.tolist() == [[1, 2, 3, 4]] * 2


@pytest.mark.parametrize("bad,match", [
    ((1, 2, 3), "4 values|y0, x0, y1, x1"),
    ([[1, 2, 3, 4]] * 2, r"\[3, 4\]"),
    ((1.5, 2, 3, 4), "integers"),
    ((-1, 2, 3, 4), "slice 0: y0 = -1"),
    ((1, -2, 3, 4), "slice 0: x0 = -2"),
    ((1, 2, 11, 4), "slice 0: y1 = 11"),
    ((1, 2, 3, 13), "slice 0: x1 = 13"),
    ([[0, 0, 1, 1], [5, 2, 3, 4], [0, 0, 1, 1]], "slice 1: y0 = 5"),
    ([[0, 0, 1, 1], [0, 0, 1, 1], [1, 6, 3, 4]], "slice 2: x0 = 6"),
])
def test_normalize_roi_rejects(bad, match):
    with pytest.raises(ValueError, match=match):
        roi.normalize_roi(bad, 3, 10, 12)


def test_roi_calls_refuse_large_shapes():
    with pytest.raises(ValueError, match="65535"):
        roi.normalize_roi((0, 0, 1, 1), 1, 65536, 8)
    with pytest.raises(ValueError, match="65535"):
        pee.check_roi_args((0, 0, 1, 1), 1, 8, 70000)


def test_record_words_round_trip():
    rng = np.random.default_rng(5)
    rects = [(0, 0, 1, 1), (0, 0, 65535, 65535), (65534, 65534, 65535, 65535), (32768, 1, 40000, 2), (1, 32768, 2, 65535)]
    for _ in range(50):
        (y0, y1), (x0, x1) = sorted(rng.integers(0, 65536, 2).tolist()), sorted(rng.integers(0, 65536, 2).tolist())
        rects.append((y0, x0, y1, x1))
    for y0, x0, y1, x1 in rects:
        w0, w2 = roi.pack_words((y0, x0, y1, x1))
        want = (0, 0, 0, 0) if y0 == y1 or x0 == x1 else (y0, x0, y1, x1)
        assert roi.unpack_words(w0, w2) == want
        assert roi.unpack_words(roi.as_signed(w0), roi.as_signed(w2)) == want      # as the int32 fields hold them
        if want != (0, 0, 0, 0):
            assert (w0, w2) == R.words(want)
    assert roi.pack_words((3, 4, 3, 9)) == (0, 0) and roi.unpack_words(12345, 0) == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        roi.pack_words((0, 0, 65536, 1))
    m = pee.make_record(64, 96, T=2, maxval=4095, L=10, end=50, status=0, roi=(40000 % 64, 3, 64, 96))
    assert roi.record_roi(m) == (40000 % 64, 3, 64, 96) and m.reserved[1] == 65536


# ---------------------------------------------------------------- check_records
def _rec(**kw):
    args = dict(T=2, maxval=4095, L=10, end=50, status=0, gate=24, roi=(8, 16, 40, 80))
    args.update(kw)
    return pee.make_record(64, 96, **args)


def _check(r):
    pee.check_records([r], 64, 96, scheme=1, payload_words=4, lm_words=24, bytes=2)


def test_check_records_accepts_roi_records():
    _check(_rec())
    _check(_rec(gate=None))                       # 65536: no gate asked for
    _check(_rec(roi=(0, 0, 64, 96)))
    r = _rec(roi=None)
    r.reserved[0] = 77                            # reserved[2] == 0: judged exactly as before (reserved[0] not looked at)
    _check(r)


def test_check_records_roi_mutants_name_the_field():
    r = _rec()
    r.reserved[2] = (65 << 16) | 80               # y1 > H
    with pytest.raises(ValueError, match=r"reserved\[2\].*y1 = 65"):
        _check(r)
    r = _rec()
    r.reserved[2] = (40 << 16) | 97               # x1 > W
    with pytest.raises(ValueError, match=r"reserved\[2\].*x1 = 97"):
        _check(r)
    r = _rec()
    r.reserved[0] = (8 << 16) | 80                # x0 >= x1 with reserved[2] != 0
    with pytest.raises(ValueError, match=r"reserved\[0\].*x0 = 80"):
        _check(r)
    r = _rec()
    r.reserved[0] = (40 << 16) | 16               # y0 >= y1
    with pytest.raises(ValueError, match=r"reserved\[0\].*y0 = 40"):
        _check(r)
    r = _rec()
    r.reserved[1] = 0                             # no gate word beside a ROI
    with pytest.raises(ValueError, match=r"reserved\[1\] = 0"):
        _check(r)


# ---------------------------------------------------------------- argument rules (before anything is queued)
def test_roi_argument_rules():
    assert pee.check_roi_args(None, 2, 64, 96, scheme=2) is None
    with pytest.raises(ValueError, match="scheme 1"):
        pee.check_roi_args((0, 0, 8, 8), 2, 64, 96, scheme=2)
    with pytest.raises(ValueError, match="tile"):
        pee.check_roi_args((0, 0, 8, 8), 2, 64, 96, tiled=True, tile_given=False)
    assert pee.check_roi_args((0, 0, 8, 8), 2, 64, 96, tiled=True, tile_given=True).tolist() == [[0, 0, 8, 8]] * 2
    with pytest.raises(ValueError, match="tmax"):
        pee.check_roi_args((0, 0, 8, 8), 2, 64, 96, T="auto", tmax=17)


def test_loader_lists_the_roi_header():
    import re
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "codec_tcc_roi.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_ROI) and len(declared) == 5
    assert _lib.KERNEL_TAGS[46] == "k_roi_bbox" and _lib.ROI_MAX_DIM == roi.ROI_MAX_DIM == 65535


# ---------------------------------------------------------------- container scheme byte 4
def _roi_file(ext=b"", roi=(8, 16, 40, 80), gate=65535, h=64, w=96):
    from codec_tcc_amd import container
    stego = np.arange(h * w, dtype=np.uint16).reshape(h, w)
    lmb = container.lm_blob(np.zeros(51, bool))
    hdr = container.create_pee_roi_header("raw", 2, w, h, 2, 10, 50, 4095, 0, len(lmb), gate, roi)
    body = container.encode_stego_raw(stego)
    import struct
    return container.MAGIC + struct.pack(">I", len(hdr + ext)) + hdr + ext + lmb + body, stego, hdr


def test_container_byte_4_round_trips():
    from codec_tcc_amd import container, pipeline
    for gate in (65535, 24, 0):
        raw, stego, hdr = _roi_file(gate=gate)
        assert container.pee_scheme(raw) == 4 == container.PEE_SCHEME_ROI and hdr[3] == 4
        md, blob, data = container.parse_pee_roi_bytes(raw)
        assert (md["roi"], md["gate"], md["scheme"], md["T"], md["L"], md["end"]) == ((8, 16, 40, 80), gate, 4, 2, 10, 50)
        assert "cover_crc32" not in md
        np.testing.assert_array_equal(container.decode_stego_raw(data, 64, 96), stego)
        pf = pipeline.read_pee_bytes(raw)                      # host half of the decode: a checked ROI record
        r = pf.records[0][0]
        assert pf.scheme == 1 and roi.record_roi(r) == (8, 16, 40, 80) and r.reserved[1] == gate + 1
    # the fixed fields are byte 3's, then the rectangle as >HHHH; the extensions follow
    g = container.create_pee_gate_header("raw", 2, 96, 64, 2, 10, 50, 4095, 0, len(container.lm_blob(np.zeros(51, bool))), 24)
    raw, _st, hdr = _roi_file(gate=24)
    assert hdr[:3] == g[:3] and hdr[4:len(g)] == g[4:] and hdr[len(g):] == bytes([0, 8, 0, 16, 0, 40, 0, 80])
    ext = container.pee_crc_extension(0x11223344, 0x55667788) + container.pee_tile_extension(32, 32, np.arange(6).reshape(2, 3))
    md = container.parse_pee_roi_bytes(_roi_file(ext=ext)[0])[0]
    assert (md["cover_crc32"], md["payload_crc32"], md["tile"]) == (0x11223344, 0x55667788, (32, 32))
    assert md["tile_crc32"].tolist() == [[0, 1, 2], [3, 4, 5]]


def test_container_byte_4_is_refused_by_the_other_parsers():
    from codec_tcc_amd import container
    raw = _roi_file()[0]
    for parse in (container.parse_pee_bytes, container.parse_pee_gate_bytes, container.parse_pee2_bytes):
        with pytest.raises(ValueError):
            parse(raw)
    # a reader that knows scheme bytes 0, 2 and 3 alone: the parent's pee_scheme rule
    def old_pee_scheme(data):
        hdr = data[8:]
        if hdr[3] not in (0, 2, 3):
            raise ValueError(f"unknown MED-PEE scheme byte {hdr[3]}")
        return hdr[3]
    with pytest.raises(ValueError, match="scheme byte 4"):
        old_pee_scheme(raw)
    with pytest.raises(ValueError, match="scheme byte 5"):
        container.pee_scheme(raw[:11] + bytes([5]) + raw[12:])


def test_container_byte_4_cut_or_bad_rectangles_are_refused():
    import struct
    from codec_tcc_amd import container, pipeline
    raw, _st, hdr = _roi_file()
    n = len(hdr)
    for cut in (1, 4, 7, 8):      # a header that ends inside the rectangle (or just before it)
        short = container.MAGIC + struct.pack(">I", n - cut) + hdr[:n - cut] + raw[8 + n:]
        with pytest.raises(ValueError, match="truncated"):
            container.parse_pee_roi_bytes(short)
        with pytest.raises(ValueError, match="truncated"):
            pipeline.read_pee_bytes(short)
    for bad in ((8, 16, 65, 80), (8, 16, 40, 97), (40, 16, 40, 80), (8, 80, 40, 16), (0, 0, 0, 0)):
        tampered = raw[:8 + n - 8] + struct.pack(">HHHH", *bad) + raw[8 + n:]
        with pytest.raises(ValueError, match="rectangle"):
            pipeline.read_pee_bytes(tampered)            # before any upload
    with pytest.raises(ValueError, match="rectangle"):
        container.create_pee_roi_header("raw", 2, 96, 64, 2, 10, 50, 4095, 0, 0, 24, (8, 16, 65, 80))
