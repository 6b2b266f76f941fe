"""Blind MED-PEE without a GPU: the vectorised spec tests/pee_blind_spec.py against the scalar
restatement tests/pee_blind_scalar.py against the known answers tests/golden/pee_blind_kat.json;
the capacity as the boundary of "fits"; the header and argument refusals of codec_tcc_amd/blind.py;
the loader's entry list."""
import hashlib
import json
import os

import numpy as np
import pytest

import pee_blind_cases as CS
import pee_blind_scalar as SC
import pee_blind_spec as BS
import pee_covers as PC
from codec_tcc_amd import _lib, blind, build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "pee_blind_kat.json")) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


def _run_cover(run):
    case = next(c for c in CS.CASES if c[0] == run["case"])
    img = CS.case_cover(case)
    if run["pad"]:
        img, _p = CS.with_padding(img, run["n_user"], run["T"])
    return img


def test_spec_matches_known_answers(kat):
    assert len(kat["runs"]) >= 12
    seen = set()
    for run in kat["runs"]:
        img = _run_cover(run)
        assert _sha(img) == run["cover_sha256"]
        bits = CS.payload(run["n_user"], 1)
        st, info, _p = BS.embed(img, bits, run["T"], run["maxval"], run["checksum"], run["max_entries"])
        assert list(info) == run["info"], run
        assert _sha(st) == run["stego_sha256"], run
        seen.add(info[0])
        if info[0] == 0:
            words = [int(v) for v in BS.read_words(st, 0, 6 + info[2])]
            assert words == run["words"]
            assert words[0] == 0x4D504231 and words[1] == run["T"] | (int(run["checksum"]) << 8) | (run["maxval"] << 16)
            assert words[5] == (BS.cover_crc(img) if run["checksum"] else 0)
            got, cov, hdr = BS.decode(st)
            np.testing.assert_array_equal(got, bits)
            np.testing.assert_array_equal(cov, img)
            assert (run["pad"] and words[-1] == BS.NO_ENTRY) or not run["pad"]
        else:
            np.testing.assert_array_equal(st, img)
    assert seen == {0, 1, 2}
    for name, caps in kat["capacity"].items():
        case = next(c for c in CS.CASES if c[0] == name)
        for me, want in caps.items():
            assert BS.capacity(CS.case_cover(case), case[4], CS.top(case[3]), int(me)) == want, (name, me)


@pytest.mark.parametrize("case", CS.CASES, ids=[c[0] for c in CS.CASES])
def test_spec_matches_scalar_restatement(case):
    """Stego, info and the decode of the two independent statements agree, and E and r are the
    table's."""
    _name, _h, _w, dtype, T, _k, n_user, E, r = case
    img = CS.case_cover(case)
    mv = CS.top(dtype)
    for n, checksum in ((n_user, True), (n_user // 3, False)):
        bits = CS.payload(n, 2)
        st, info, p = BS.embed(img, bits, T, mv, checksum)
        assert info[0] == 0 and info[2] == E and p["r"] == r and info[5] == 2 * (img.shape[0] // 2 - r)
        s2, i2 = SC.embed(img.astype(np.int64).tolist(), bits.tolist(), T, mv, img.dtype.itemsize, checksum)
        assert tuple(i2) == tuple(info)
        np.testing.assert_array_equal(np.asarray(s2), st)
        y0 = info[5]
        np.testing.assert_array_equal(st[y0:] >> 1, img[y0:] >> 1)   # the region: LSBs alone change
        g2, c2, h2 = SC.decode(st.astype(np.int64).tolist())
        got, cov, hdr = BS.decode(st)
        assert g2 == bits.tolist() == got.tolist()
        np.testing.assert_array_equal(np.asarray(c2), img)
        np.testing.assert_array_equal(cov, img)
        assert h2 == (hdr["T"], hdr["flags"], hdr["maxval"], hdr["n_user"], hdr["E"], hdr["end"], hdr["crc"])


@pytest.mark.parametrize("name", [c[0] for c in CS.SHAPE_CASES])
def test_spec_matches_scalar_restatement_shapes(name):
    """The same on every cover and payload length of tests/test_pee_blind_shapes.py (tall, wide,
    many-entry, long-payload and narrow slices): stego, info and both decodes of the two
    statements agree, the capacity is the scalar plan's boundary and the figures DESIGN §3k
    quotes, so the spec is pinned at these shapes without a GPU."""
    img, T, mv, me, checksum, lengths, cap = CS.shape_case(name)
    rows = img.astype(np.int64).tolist()
    if name in CS.SHAPE_CAPACITY:
        assert cap == CS.SHAPE_CAPACITY[name]
    assert cap < 0 or SC.plan(rows, cap, T, mv, me)[0] == 0
    assert SC.plan(rows, cap + 1, T, mv, me)[0] in (1, 2)
    table = []
    for q, n in enumerate(lengths):
        bits = CS.payload(n, q + 1)
        st, info, p = BS.embed(img, bits, T, mv, checksum, me)
        assert (info[0] == 0) == (n <= cap)
        if info[0] == 0:
            table.append((info[2], p["r"]))
        s2, i2 = SC.embed(rows, bits.tolist(), T, mv, img.dtype.itemsize, checksum, me)
        assert tuple(i2) == tuple(info)
        np.testing.assert_array_equal(np.asarray(s2), st)
        if info[0]:
            np.testing.assert_array_equal(st, img)
            continue
        assert info[5] == 2 * (img.shape[0] // 2 - p["r"]) and info[3] == 192 + 32 * info[2]
        g2, c2, h2 = SC.decode(st.astype(np.int64).tolist())
        got, cov, hdr = BS.decode(st)
        assert g2 == bits.tolist() == got.tolist()
        np.testing.assert_array_equal(np.asarray(c2), img)
        np.testing.assert_array_equal(cov, img)
        assert h2 == (hdr["T"], hdr["flags"], hdr["maxval"], hdr["n_user"], hdr["E"], hdr["end"], hdr["crc"])
    assert tuple(table) == CS.SHAPE_ER[name]   # the table of DESIGN §3k


@pytest.mark.parametrize("case", CS.CASES, ids=[c[0] for c in CS.CASES])
def test_capacity_is_the_boundary_of_fits(case):
    _name, _h, _w, dtype, T, _k, _n, _E, _r = case
    img = CS.case_cover(case)
    mv = CS.top(dtype)
    for me in (256, 1):
        cap = BS.capacity(img, T, mv, me)
        if cap >= 0:
            st, info, _p = BS.embed(img, CS.payload(cap, 3), T, mv, max_entries=me)
            assert info[0] == 0
            got, cov, _h2 = BS.decode(st)
            assert got.size == cap
            np.testing.assert_array_equal(cov, img)
        assert BS.embed(img, CS.payload(cap + 1, 3), T, mv, max_entries=me)[1][0] in (1, 2)


def test_refused_slices():
    sm = CS.smooth(64, 96)
    st, info, _p = BS.embed(sm, CS.payload(500, 1), 2, 4095)
    assert info == (1, 500, 0, 0, -1, 0)
    np.testing.assert_array_equal(st, sm)
    for kind in ("checker", "checker_inv", "flat_max"):
        c = PC.cover(kind, 64, 96, "uint16", 4095)
        assert BS.embed(c, CS.payload(10, 1), 2, 4095)[1][0] == 1 and BS.capacity(c, 2, 4095) == -1
    assert BS.embed(CS.planted(64, 96, 3), CS.payload(100, 1), 4, 4095, max_entries=2)[1] == (2, 100, 3, 0, -1, 0)
    assert SC.embed(CS.planted(64, 96, 3).tolist(), [0] * 100, 4, 4095, 2, False, 2)[1] == (2, 100, 3, 0, -1, 0)


def test_header_refusals():
    """parse_header: every field the decoder judges, and it is the spec's judgement."""
    img = CS.planted(64, 96, 1)
    st, info, _p = BS.embed(img, CS.payload(150, 1), 4, 4095, checksum=True)
    good = [int(v) for v in BS.read_words(st, 0, 6)]
    h = blind.parse_header(good, 64, 96, 65535)
    assert h == BS.check_header(good, 64, 96, 65535)
    assert (h["T"], h["flags"], h["maxval"], h["n_user"], h["E"], h["end"]) == (4, 1, 4095, 150, 1, info[4])
    assert h["rect"] == (info[5], 0, 64, 96) and h["L"] == info[3] + 150

    def bad(k, v, field):
        w = list(good)
        w[k] = v
        for fn in (blind.parse_header, BS.check_header):
            with pytest.raises(ValueError, match=field):
                fn(w, 64, 96, 65535)
    bad(0, good[0] ^ 1, "magic")
    bad(1, (good[1] & ~0xFF), "T = 0")
    bad(1, (good[1] & ~0xFF) | 65, "T = 65")
    bad(1, good[1] | (2 << 8), "flags")
    bad(1, good[1] & 0xFFFF, "maxval = 0")
    bad(4, 32 * 48, "end")                       # = nc
    bad(4, (32 - 2) * 48, "end")                 # the first candidate of the reserved rows
    bad(3, 32 * 48 + 1, "E = ")
    bad(3, 200, "(n_side|end|E) = ")             # more side bits than rows above `end` leave
    bad(2, good[4] + 2, "n_user")
    bad(4, 0xFFFFFFFF, "n_user")                 # end = -1 with bits to read
    with pytest.raises(ValueError, match="maxval = 4095"):
        blind.parse_header(good, 64, 96, 255)
    with pytest.raises(ValueError, match=r"slices \[1\]"):
        blind.parse_headers(np.array([good + [0, 0], [0] * 8], dtype=np.uint32), 64, 96, 2)
    heads = blind.parse_headers(np.array([good + [0, 0]] * 2, dtype=np.uint32), 64, 96, 2)
    assert all(int(heads[k][1]) == v for k, v in h.items() if k != "rect") and tuple(heads["rect"][1]) == h["rect"]
    # the batched statement of the rules refuses exactly what the per-slice one refuses
    rng = np.random.default_rng(8)
    rows = np.array([good + [0, 0]] * 400, dtype=np.uint32)
    rows[np.arange(400), rng.integers(1, 5, 400)] ^= (1 << rng.integers(0, 32, 400)).astype(np.uint32)
    for row in rows:
        try:
            blind.parse_header(row, 64, 96, 65535)
            one = True
        except ValueError:
            one = False
        try:
            blind.parse_headers(row[None], 64, 96, 2)
            many = True
        except ValueError:
            many = False
        assert one == many, row
    # the records built for all slices at once are make_record's
    from codec_tcc_amd.pee_checks import make_record
    want = make_record(64, 96, T=h["T"], maxval=h["maxval"], L=h["L"], end=h["end"], status=0, roi=h["rect"])
    raw = blind.records_bytes(heads, 64, 96)
    assert raw[:_lib.PEE_META_BYTES] == bytes(want) == raw[_lib.PEE_META_BYTES:]
    assert blind.row_words(150, 256) == (150 + 192 + 32 * 256 + 63) // 64
    assert blind.region(64, 96, 224) == BS.region(64, 96, 224) == (2, (60, 0, 64, 96))


def test_argument_refusals():
    """scheme 2, T='auto', a gate, roi=, key=, big shapes, in place: ValueError before any GPU work."""
    ok = dict(scheme=1, T=2, gate=None, H=64, W=96, maxval=4095)
    blind.check_args(**ok)
    for change, text in ((dict(scheme=2), "scheme 1"), (dict(T="auto"), "fixed T"), (dict(T=65), "1..64"),
                         (dict(gate=3), "gate"), (dict(gate="auto"), "gate"), (dict(roi=(0, 0, 4, 4)), "roi"),
                         (dict(key=b"k" * 32), "key"), (dict(H=65536), "65535"), (dict(W=65536), "65535"),
                         (dict(H=8, W=16), "header bits"), (dict(maxval=0), "maxval"), (dict(max_entries=-1), "max_entries"),
                         (dict(max_entries=65537), "max_entries"), (dict(max_entries=1.5), "max_entries"),
                         (dict(in_place=True), "out of place")):
        with pytest.raises(ValueError, match=text):
            blind.check_args(**{**ok, **change})
    import codec_tcc_amd as pkg
    cover = CS.smooth(64, 96)
    for kw in (dict(scheme=2), dict(T="auto"), dict(gate=8), dict(roi=(0, 0, 8, 8)), dict(key=b"k" * 32)):
        with pytest.raises(ValueError):   # before the GPU is asked for: this runs without one
            pkg.encode_blind(cover, [b"x"], **kw)


def test_loader_lists_the_blind_entries():
    hdr = open(os.path.join(build.INC, "codec_tcc_blind.h")).read()
    assert set(_lib.EXPORTS_BLIND) == {"codec_pee_blind_workspace_bytes", "codec_pee_blind_plan", "codec_pee_blind_embed",
                                       "codec_pee_blind_headers", "codec_pee_blind_extract"}
    assert os.path.join(build.INC, "codec_tcc_blind.h") in build._common_deps()
    assert os.path.join(build.HERE, "csrc", "codec_blind.hip") in build.SRCS
    assert _lib.KERNEL_TAGS[52] == "k_blind_rows" and "#define CODEC_K_BLIND_ROWS 52" in hdr
    assert f"#define CODEC_PEE_BLIND_MAGIC {_lib.BLIND_MAGIC:#010X}u".replace("0X", "0x") in hdr
    assert _lib.BLIND_HDR_WORDS == BS.HDR_WORDS == 6 and _lib.BLIND_MAGIC == BS.MAGIC == SC.MAGIC
