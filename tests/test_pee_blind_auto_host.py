"""Blind MED-PEE with capacity control without a GPU: the spec tests/pee_blind_auto_spec.py against
the scalar restatement tests/pee_blind_auto_scalar.py against the known answers
tests/golden/pee_blind_auto_kat.json, on every case of tests/pee_blind_auto_cases.py; the closed
form over T against the oracle's classification; the argument refusals of codec_tcc_amd/blind.py;
the loader's entry list."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import pee_blind_auto_cases as AC
import pee_blind_auto_scalar as SC
import pee_blind_auto_spec as AS
import pee_blind_cases as CS
import pee_blind_spec as BS
from codec_tcc_amd import _lib, blind, build

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [c[0] for c in AC.CASES]


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "pee_blind_auto_kat.json")) as f:
        return {c["case"]: c for c in json.load(f)["cases"]}


def _sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


@pytest.mark.parametrize("name", NAMES)
def test_spec_scalar_and_known_answers_agree(name, kat):
    """T*, stego, info and the capacity curve of the two independent statements and of the known
    answers agree; T* is the table's; a refused slice is its cover; an embedded one
    decodes, by the fixed-T spec's decode, to the payload and the cover."""
    _n, me, lengths = AC.CASE[name]
    img = AC.cover(name)
    mv = CS.top(img.dtype)
    rows = img.astype(np.int64).tolist()
    k = kat[name]
    assert (k["max_entries"], k["tmax"], k["maxval"], k["cover_sha256"]) == (me, AC.TMAX, mv, _sha(img))
    curve = AS.capacity_curve(img, AC.TMAX, mv, me)
    assert curve == SC.choose(rows, 0, AC.TMAX, mv, me)[2] == k["curve"]
    assert AS.capacity(img, AC.TMAX, mv, me) == max(curve)
    assert len(k["runs"]) == len(lengths)
    for q, ((n, want_t), run) in enumerate(zip(lengths, k["runs"])):
        bits = AC.payload(n, q + 1)
        checksum = q % 2 == 0
        st, info, T, p = AS.embed(img, bits, AC.TMAX, mv, checksum, me)
        assert T == want_t == run["T"], (name, n, T)
        assert (run["n_user"], run["checksum"]) == (n, checksum)
        # the rule itself: no smaller T has status 0, and a refusal is the plan's at tmax
        assert all(BS.plan(img, n, t, mv, me)["status"] != 0 for t in range(1, T if T else AC.TMAX + 1))
        assert (n <= curve[T - 1]) if T else all(n > c for c in curve)
        s2, i2, t2 = SC.embed(rows, bits.tolist(), AC.TMAX, mv, img.dtype.itemsize, checksum, me)
        assert t2 == T and tuple(i2) == tuple(info) == tuple(run["info"])
        np.testing.assert_array_equal(np.asarray(s2), st)
        assert _sha(st) == run["stego_sha256"]
        if T == 0:
            assert info == (BS.plan(img, n, AC.TMAX, mv, me)["status"], n, p["E"], 0, -1, 0)
            np.testing.assert_array_equal(st, img)
            continue
        assert [int(v) for v in BS.read_words(st, 0, 6 + info[2])] == run["words"] == SC.header_words(s2, 6 + info[2])
        assert run["words"][1] == T | (int(checksum) << 8) | (mv << 16)
        np.testing.assert_array_equal(st, BS.embed(img, bits, T, mv, checksum, me)[0])
        got, cov, hdr = BS.decode(st)
        assert hdr["T"] == T
        np.testing.assert_array_equal(got, bits)
        np.testing.assert_array_equal(cov, img)


def test_bright_block_statuses():
    """The T-dependent part of the unsafe count, and a refusal whose status is tmax's, not T = 1's."""
    img = AC.cover("bright_me4")
    assert tuple(int(BS.row_counts(img, T, 4095)[1].sum()) for T in range(1, 9)) == AC.BRIGHT_UNSAFE
    assert tuple(BS.plan(img, 0, T, 4095, 4)["status"] for T in range(1, 9)) == AC.BRIGHT_ME4_STATUS
    for n in (0, 150, 300):
        _st, info, T, _p = AS.embed(img, AC.payload(n, 1), 8, 4095, max_entries=4)
        assert T == 0 and info[0] == 2
    assert AS.choose(img, 0, 4, 4095, 4)[1]["status"] == 1


@pytest.mark.parametrize("name", ["smooth", "planted3", "smooth_u8", "bright_me16", "bright_u8"])
def test_closed_form_is_the_classification(name):
    """The row table of one classification per candidate equals the oracle's row counts at every T
    in 1..16."""
    img = AC.cover(name)
    mv = CS.top(img.dtype)
    tab = SC.table(img.astype(np.int64).tolist(), 16, mv)
    for T in range(1, 17):
        es, uns = BS.row_counts(img, T, mv)
        assert [r[0] for r in tab[T - 1]] == es.tolist() and [r[1] for r in tab[T - 1]] == uns.tolist(), T


def test_tmax_bounds():
    img = AC.cover("smooth")
    assert AS.choose(img, 300, 16, 4095)[0] == AS.choose(img, 300, 8, 4095)[0] == 4
    assert AS.choose(img, 300, 3, 4095)[0] == 0
    st1, info1, T1, _p = AS.embed(img, AC.payload(0, 1), 1, 4095)
    assert T1 == 0 and info1 == BS.embed(img, AC.payload(0, 1), 1, 4095)[1]
    u8 = AC.cover("smooth_u8")
    st, info, T, _p = AS.embed(u8, AC.payload(200, 1), 1, 255)
    assert T == 1
    np.testing.assert_array_equal(st, BS.embed(u8, AC.payload(200, 1), 1, 255)[0])
    for bad in (0, 17):
        with pytest.raises(ValueError):
            AS.choose(img, 0, bad, 4095)
        with pytest.raises(ValueError):
            SC.choose(img.tolist(), 0, bad, 4095)


def test_argument_refusals():
    """tmax 0 and 17 and the inherited refusals, as ValueError before any GPU work; the fixed-T
    calls still refuse T='auto'."""
    ok = dict(scheme=1, tmax=8, gate=None, H=64, W=96, maxval=4095)
    blind.check_args_auto(**ok)
    blind.check_args_auto(**{**ok, "tmax": 1})
    blind.check_args_auto(**{**ok, "tmax": 16})
    for change, text in ((dict(tmax=0), "tmax"), (dict(tmax=17), "tmax"), (dict(tmax=-1), "tmax"), (dict(tmax=2.5), "tmax"),
                         (dict(tmax="auto"), "tmax"), (dict(tmax=True), "tmax"), (dict(scheme=2), "scheme 1"),
                         (dict(scheme=2, tmax=0), "scheme 1"), (dict(gate=3), "gate"), (dict(gate="auto"), "gate"),
                         (dict(roi=(0, 0, 4, 4)), "roi"), (dict(key=b"k" * 32), "key"), (dict(H=65536), "65535"),
                         (dict(W=65536), "65535"), (dict(H=8, W=16), "header bits"), (dict(maxval=0), "maxval"),
                         (dict(max_entries=-1), "max_entries"), (dict(max_entries=65537), "max_entries"),
                         (dict(in_place=True), "out of place"), (dict(tmax=17, gate=3), "tmax")):
        with pytest.raises(ValueError, match=text):
            blind.check_args_auto(**{**ok, **change})
    with pytest.raises(ValueError, match="fixed T"):
        blind.check_args(scheme=1, T="auto", gate=None, H=64, W=96, maxval=4095)
    import codec_tcc_amd as pkg
    cover = CS.smooth(64, 96)
    for kw in (dict(tmax=0), dict(tmax=17), dict(max_entries=-1), dict(maxval=0)):
        with pytest.raises(ValueError):   # before the GPU is asked for: this runs without one
            pkg.encode_blind_auto(cover, [b"x"], **kw)
    with pytest.raises(ValueError):
        pkg.encode_blind_auto(np.zeros((8, 16), np.uint16), [b"x"])
    with pytest.raises(ValueError):
        pkg.encode_blind(cover, [b"x"], T="auto")
    assert "encode_blind_auto" in pkg.__all__
    assert blind.TMAX == AS.TMAX == 16


def test_loader_lists_the_blind_auto_entries():
    path = os.path.join(build.INC, "codec_tcc_blind_auto.h")
    hdr = open(path).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_BLIND_AUTO) == {"codec_pee_blind_auto_workspace_bytes", "codec_pee_blind_plan_auto",
                                                       "codec_pee_blind_embed_auto"}
    assert path in build._common_deps()
    assert _lib.KERNEL_TAGS[53] == "k_blind_rows_auto" and "#define CODEC_K_BLIND_ROWS_AUTO 53" in hdr
    assert f"#define CODEC_PEE_BLIND_TMAX {_lib.BLIND_TMAX}" in hdr
    # the fixed-T header keeps its five entries
    fixed = open(os.path.join(build.INC, "codec_tcc_blind.h")).read()
    assert len(set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", fixed, re.M))) == 5 == len(_lib.EXPORTS_BLIND)
    for name in _lib.EXPORTS_BLIND_AUTO:   # the loader binds them: argument counts as declared
        m = re.search(rf"{name}\s*\(([^)]*)\)", hdr, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib._SIGS_BLIND_AUTO[name][1]), name
