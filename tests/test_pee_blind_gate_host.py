"""Gated blind MED-PEE without a GPU: the spec tests/pee_blind_gate_spec.py against the scalar
restatement tests/pee_blind_gate_scalar.py against the known answers
tests/golden/pee_blind_gate_kat.json; the closed forms (over T, and of the roughness class) against the
oracle's classification and D at every pair; the header rules of codec_tcc_amd/blind.py; the argument
refusals; the loader's entry list; and the rule's choice on every case the GPU tests run."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import pee_blind_auto_cases as AC
import pee_blind_auto_spec as AS
import pee_blind_cases as CS
import pee_blind_gate_cases as GC
import pee_blind_gate_scalar as SC
import pee_blind_gate_spec as GS
import pee_blind_spec as BS
from codec_tcc_amd import _lib, blind, build

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_NAMES = [c[0] for c in GC.CASES if GC.cover(c[0]).size <= 30000]
GATES = GS.GATES


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "pee_blind_gate_kat.json")) as f:
        return {c["case"]: c for c in json.load(f)["cases"]}


def _sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


def test_the_known_answers_cover_the_small_cases(kat):
    assert sorted(kat) == sorted(KAT_NAMES) and len(KAT_NAMES) >= 8


@pytest.mark.parametrize("name", KAT_NAMES)
def test_spec_scalar_and_known_answers_agree(name, kat):
    """(T*, G*), stego, info and the capacity curve of the two independent statements and of the known
    answers agree; the pair is the table's; a refused slice is its cover; an embedded
    one decodes, by the spec's and by the restatement's decoder, to the payload and the cover."""
    _n, me, lengths = GC.CASE[name]
    img = GC.cover(name)
    mv = CS.top(img.dtype)
    rows = img.astype(np.int64).tolist()
    k = kat[name]
    assert (k["max_entries"], k["tmax"], k["maxval"], k["cover_sha256"]) == (me, GC.TMAX, mv, _sha(img))
    curve = GS.capacity_curve(img, GC.TMAX, mv, me)
    assert curve == SC.choose(rows, 0, GC.TMAX, mv, me)[3] == k["curve"]
    assert len(k["runs"]) == len(lengths)
    for q, ((n, want_t, want_g), run) in enumerate(zip(lengths, k["runs"])):
        bits = GC.payload(n, q + 1)
        checksum = q % 2 == 0
        st, info, T, G, p = GS.embed(img, bits, GC.TMAX, mv, checksum, me)
        assert (T, G) == (want_t, want_g) == (run["T"], run["G"]), (name, n, T, G)
        assert (run["n_user"], run["checksum"]) == (n, checksum)
        s2, i2, t2, g2 = SC.embed(rows, bits.tolist(), GC.TMAX, mv, img.dtype.itemsize, checksum, me)
        assert (t2, g2) == (T, G) and tuple(i2) == tuple(info) == tuple(run["info"])
        np.testing.assert_array_equal(np.asarray(s2), st)
        assert _sha(st) == run["stego_sha256"]
        if T == 0:
            assert info == (GS.plan(img, n, GC.TMAX, 15, mv, me)["status"], n, p["E"], 0, -1, 0)
            np.testing.assert_array_equal(st, img)
            continue
        j = GATES.index(G)
        assert [int(v) for v in BS.read_words(st, 0, 6 + info[2])] == run["words"]
        assert run["words"][1] == T | ((int(checksum) | 8 | (j << 4)) << 8) | (mv << 16)
        assert n <= curve[T - 1][j]
        got, cov, hdr = GS.decode(st)
        assert (hdr["T"], hdr["G"]) == (T, G)
        np.testing.assert_array_equal(got, bits)
        np.testing.assert_array_equal(cov, img)
        got2, cov2 = SC.decode(s2)
        assert got2 == bits.tolist() and cov2 == rows
        with pytest.raises(ValueError, match="flags"):   # the ungated spec keeps refusing the gate's flags
            BS.decode(st)


@pytest.mark.parametrize("name", KAT_NAMES)
def test_the_rule_is_the_first_pair_in_order(name):
    """choose() against the rule spelt out with plan(): every pair before the chosen one, in (T, j)
    order, is refused; a refusal has no pair at all."""
    _n, me, lengths = GC.CASE[name]
    img = GC.cover(name)
    mv = CS.top(img.dtype)
    for n, want_t, want_g in lengths:
        ok = [(t, j) for t in range(1, GC.TMAX + 1) for j in range(16) if GS.plan(img, n, t, j, mv, me)["status"] == 0]
        assert ((ok[0][0], GATES[ok[0][1]]) if ok else (0, -1)) == (want_t, want_g), (name, n)


@pytest.mark.parametrize("name,cover", [("smooth", lambda: AC.cover("smooth")), ("planted3", lambda: AC.cover("planted3")),
                                        ("smooth_u8", lambda: AC.cover("smooth_u8")), ("bright", lambda: AC.cover("bright_me16")),
                                        ("half_u16", lambda: GC.cover("half_u16")), ("half_u8", lambda: GC.cover("half_u8")),
                                        ("planted_mix", lambda: GC.cover("planted_mix"))])
def test_closed_forms_are_the_classification(name, cover):
    """One classification per candidate (closed over T, class from the leading bits of D - 1) gives the
    oracle's classify and D <= G counts of every row at every (T, j), T in 1..16; the spec's own
    one-class-per-candidate tables do too."""
    img = cover()
    mv = CS.top(img.dtype)
    tab = SC.table(img.astype(np.int64).tolist(), 16, mv)
    es_t, un_t = GS.tables(img, list(range(1, 17)), mv)
    for T in range(1, 17):
        for j in range(16):
            es, uns = GS.row_counts(img, T, GATES[j], mv)
            assert [r[0] for r in tab[T - 1][j]] == es.tolist() == es_t[T - 1][j].tolist(), (T, j)
            assert [r[1] for r in tab[T - 1][j]] == uns.tolist() == un_t[T - 1][j].tolist(), (T, j)
    for D in list(range(0, 300)) + [4095, 65535]:
        assert SC.rough_class(D) == next(j for j in range(16) if D <= GATES[j]), D


def test_the_last_gate_is_the_ungated_plan():
    """At j = 15 every candidate is active: the plan is pee_blind_spec's, the stego differs from
    embed_blind's in the flags alone."""
    img = GC.cover("half_u16")
    for T in (3, 5, 8):
        for n in (0, 40, 300):
            assert GS.plan(img, n, T, 15, 4095) == BS.plan(img, n, T, 4095)
    bits = GC.payload(40, 2)
    st, info, T, G, _p = GS.embed(img, bits, 8, 4095)
    assert (T, G) == (3, 65535)
    ref, rinfo, _q = BS.embed(img, bits, 3, 4095)
    assert info == rinfo and (BS.read_words(st, 1, 1)[0] >> 8) & 0xFF == 0xF8
    diff = np.flatnonzero(st.ravel() != ref.ravel())
    assert set((img.size - 1 - diff).tolist()) <= set(range(32 + 8 + 3, 32 + 16))   # word 1's flag bits 3-7


def test_planted_mix_needs_fewer_entries():
    """The busy half's extreme pixels are inactive below the last gate: E = 3 at the chosen pairs, 6 in
    the ungated plan at the T embed_blind_auto picks."""
    img = GC.cover("planted_mix")
    for n, T, G in GC.CASE["planted_mix"][2]:
        if T:
            assert GS.choose(img, n, GC.TMAX, 4095)[2]["E"] == GC.PLANTED_MIX_E[0]
    t, p = AS.choose(img, 100, GC.TMAX, 4095)
    assert t == 6 and p["E"] == GC.PLANTED_MIX_E[1]


def test_bright_block_statuses():
    """max_entries 4: every pair is refused, for capacity at some and for the entries at others, and the
    refusal reported is the last pair's; max_entries 16: the same cover is feasible from T = 5."""
    img = GC.cover("bright_me4")
    st4 = {(T, j): GS.plan(img, 0, T, j, 4095, 4)["status"] for T in range(1, 9) for j in range(16)}
    assert set(st4.values()) == {1, 2} and st4[(8, 15)] == 2
    for n in (0, 100):
        _st, info, T, G, _p = GS.embed(img, GC.payload(n, 1), 8, 4095, max_entries=4)
        assert (T, G, info[0]) == (0, -1, 2)
    st16 = {(T, j): GS.plan(img, 0, T, j, 4095, 16)["status"] for T in range(1, 9) for j in range(16)}
    assert set(st16.values()) == {0, 1} and min(T for (T, _j), s in st16.items() if s == 0) == 5


def test_fixed_forms():
    """T=, gate= and both: the rule over what is left free; a refusal reports the fixed values' plan."""
    for name, n, T, gate, want in GC.FIXED:
        img = GC.cover(name)
        mv = CS.top(img.dtype)
        bits = GC.payload(n, 3)
        st, info, t, g, p = GS.embed(img, bits, GC.TMAX, mv, True, 256, T=T, gate=gate)
        assert (t, g) == want, (name, n, T, gate)
        s2, i2, t2, g2 = SC.embed(img.astype(np.int64).tolist(), bits.tolist(), GC.TMAX, mv, img.dtype.itemsize, True, 256,
                                  T or 0, -1 if gate is None else GATES.index(gate))
        assert (t2, g2) == want and tuple(i2) == tuple(info)
        np.testing.assert_array_equal(np.asarray(s2), st)
        if t == 0:
            last = GS.plan(img, n, T or GC.TMAX, 15 if gate is None else GATES.index(gate), mv)
            assert info == (last["status"], n, last["E"], 0, -1, 0)
    img = GC.cover("half_u16")
    for bad in (dict(gate=5), dict(gate=65534), dict(gate=-1), dict(T=0), dict(T=9)):
        with pytest.raises(ValueError):
            GS.choose(img, 0, 8, 4095, **bad)


@pytest.mark.parametrize("name", [c[0] for c in GC.CASES])
@pytest.mark.parametrize("B", [3, 9])
def test_the_gpu_cases_exercise_what_they_claim(name, B):
    """The rule's choice recomputed for every slice of every GPU batch: the table's pairs in the
    first turn, and per case the property it is there for."""
    _n, me, lengths = GC.CASE[name]
    got = []
    for b in range(B):
        img, bits = GC.batch_slice(name, b)
        t, j, _p = GS.choose(img, bits.size, GC.TMAX, CS.top(img.dtype), me)
        got.append((bits.size, t, GATES[j] if t else -1))
    assert tuple(got[:len(lengths)]) == tuple(lengths[:B])
    pairs = {(t, g) for _n2, t, g in got}
    if name.startswith("half"):
        assert len({t for t, _g in pairs if t}) >= 2 and len({g for _t, g in pairs if g >= 0}) >= 2
        if B == 9:
            assert (0, -1) in pairs and any(n == 0 for n, _t, _g in got)
    if name == "half_u16":
        assert any(g == 65535 for _t, g in pairs)
    if name == "long":
        assert got[1][0] == 20000 and got[1][1] > 0 and 0 <= got[1][2] < 65535
    if name.startswith("xwide"):
        assert GC.cover(name).shape[1] // 2 // 64 >= 60   # candidates per lane of one row
    if name == "bright_me4":
        assert pairs == {(0, -1)}


def _hdr(flags, n_user=300, E=0, end=1000, T=4, maxval=4095):
    return [blind.MAGIC, T | (flags << 8) | (maxval << 16), n_user, E, end, 0]


def test_header_rules():
    """Bit 3 marks a gated slice and bits 4-7 hold its ladder index; without bit 3 they are 0; keyed
    and volume headers keep refusing both; the header dict and the rebuilt record carry the gate."""
    H, W = 64, 96
    for j in range(16):
        for crc in (0, 1):
            h = blind.parse_header(_hdr(8 | (j << 4) | crc), H, W, 65535)
            assert h["G"] == GATES[j] and h["flags"] == 8 | (j << 4) | crc
    assert "G" not in blind.parse_header(_hdr(0), H, W, 65535) and "G" not in blind.parse_header(_hdr(1), H, W, 65535)
    for flags in (2, 3):
        with pytest.raises(ValueError, match=r"flags = 0x[23] \(bit 0 alone is defined\)"):
            blind.parse_header(_hdr(flags), H, W, 65535)
    for flags in (0x10, 0x11, 0xF0, 0x80, 4, 5, 6, 0x0A, 0x0C, 0x8A, 0xFE):
        with pytest.raises(ValueError, match="flags"):
            blind.parse_header(_hdr(flags), H, W, 65535)
    for flags in (8, 9, 0x82, 12, 0x88, 0xF8, 0x0A, 0x12):
        with pytest.raises(ValueError, match="flags"):
            blind.parse_header(_hdr(flags), H, W, 65535, keyed=True)
    for flags in (8, 0x82, 12, 13, 0x8C, 0xFC, 0x14):
        with pytest.raises(ValueError, match="flags"):
            blind.parse_header(_hdr(flags), H, W, 65535, volume=True)
    all_flags = [0, 1, 8, 9, 0x48, 0xF9, 2, 0x10, 0xF0, 12]
    hdr = np.array([_hdr(f) + [0, 0] for f in all_flags], dtype=np.uint32)
    good = blind.parse_headers(hdr[:6], H, W, 2)
    assert good["G"].tolist() == [65535, 65535, 0, 0, 4, 65535] and good["flags"].tolist() == all_flags[:6]
    with pytest.raises(ValueError, match=r"slices \[6, 7, 8, 9\]"):
        blind.parse_headers(hdr, H, W, 2)
    # keyed and volume arrays are what they were: blind_volume.py fills its own arrays key by key
    assert "G" not in blind.parse_headers(np.array([_hdr(2) + [0, 0]], dtype=np.uint32), H, W, 2, keyed=True)
    assert "G" not in blind.parse_headers(np.array([_hdr(4) + [0, 0]], dtype=np.uint32), H, W, 2, volume=True)
    rec = np.frombuffer(blind.records_bytes(good, H, W), dtype="<u4").reshape(6, -1)
    assert rec[:, 14].tolist() == [65536, 65536, 1, 1, 5, 65536]
    plain = {k: v for k, v in good.items() if k != "G"}   # headers parsed elsewhere, without a gate
    assert np.frombuffer(blind.records_bytes(plain, H, W), dtype="<u4").reshape(6, -1)[:, 14].tolist() == [65536] * 6
    # a spec-made gated stego parses to the spec's header
    img = GC.cover("half_u16")
    st, info, T, G, _p = GS.embed(img, GC.payload(127, 1), 8, 4095, True)
    h = blind.parse_header(BS.read_words(st, 0, 6), 64, 96, 65535)
    hs = GS.decode(st)[2]
    assert (h["T"], h["G"], h["E"], h["end"], h["n_user"], h["rect"], h["crc"]) == \
        (T, G, hs["E"], hs["end"], hs["n_user"], hs["rect"], hs["crc"]) and (T, G) == (5, 12)
    assert (blind.FLAG_GATED, blind.FLAG_GATE_SHIFT) == (GS.FLAG_GATED, GS.FLAG_J_SHIFT) == (8, 4)


def test_argument_refusals():
    """check_args_gated: tmax, T, gate and the inherited refusals, as ValueError before any GPU work;
    the other blind calls keep refusing gate=."""
    ok = dict(scheme=1, tmax=8, H=64, W=96, maxval=4095)
    assert blind.check_args_gated(**ok) == (0, -1)
    assert blind.check_args_gated(**ok, T=8, gate=65535) == (8, 15)
    assert blind.check_args_gated(**ok, T=1, gate=0) == (1, 0)
    assert blind.check_args_gated(**{**ok, "tmax": 16}, gate=6) == (0, 5)
    for change, text in ((dict(tmax=0), "tmax"), (dict(tmax=17), "tmax"), (dict(tmax=2.5), "tmax"), (dict(tmax="auto"), "tmax"),
                         (dict(tmax=True), "tmax"), (dict(T=0), "1..tmax"), (dict(T=9), "1..tmax"), (dict(T="auto"), "1..tmax"),
                         (dict(T=2.5), "1..tmax"), (dict(T=True), "1..tmax"), (dict(gate=5), "ladder"),
                         (dict(gate=65534), "ladder"), (dict(gate=-1), "ladder"), (dict(gate=None), "ladder"),
                         (dict(gate="on"), "ladder"), (dict(gate=True), "ladder"), (dict(gate=2.5), "ladder"),
                         (dict(scheme=2), "scheme 1"), (dict(scheme=2, tmax=0), "scheme 1"),
                         (dict(roi=(0, 0, 4, 4)), "roi"), (dict(key=b"k" * 32), "key"), (dict(H=65536), "65535"),
                         (dict(W=65536), "65535"), (dict(H=8, W=16), "header bits"), (dict(maxval=0), "maxval"),
                         (dict(max_entries=-1), "max_entries"), (dict(max_entries=65537), "max_entries"),
                         (dict(in_place=True), "out of place"), (dict(tmax=17, gate=5), "tmax"), (dict(T=9, gate=5), "1..tmax")):
        with pytest.raises(ValueError, match=text):
            blind.check_args_gated(**{**ok, **change})
    with pytest.raises(ValueError, match=re.escape(str(GATES))):
        blind.check_args_gated(**ok, gate=5)
    with pytest.raises(ValueError, match="gate"):
        blind.check_args(scheme=1, T=2, gate=4, H=64, W=96, maxval=4095)
    with pytest.raises(ValueError, match="gate"):
        blind.check_args_auto(scheme=1, tmax=8, gate=4, H=64, W=96, maxval=4095)
    import codec_tcc_amd as pkg
    cover = CS.smooth(64, 96)
    for kw in (dict(tmax=0), dict(tmax=17), dict(gate=5), dict(T=5), dict(max_entries=-1), dict(maxval=0)):
        with pytest.raises(ValueError):   # before the GPU is asked for: this runs without one
            pkg.encode_blind_gated(cover, [b"x"], **kw)
    with pytest.raises(ValueError):
        pkg.encode_blind_gated(np.zeros((8, 16), np.uint16), [b"x"])
    assert "encode_blind_gated" in pkg.__all__ and blind.GATES == GATES == _lib.GATES and blind.GATED_TMAX_DEFAULT == 4
    from codec_tcc_amd import pipeline
    from codec_tcc_amd.pee import PeeCodec
    assert callable(pipeline.encode_dicom_pee_gated) and callable(PeeCodec.embed_blind_gated) and \
        callable(PeeCodec.blind_capacity_gated)


def test_loader_lists_the_blind_gate_entries():
    path = os.path.join(build.INC, "codec_tcc_blind_gate.h")
    hdr = open(path).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_BLIND_GATE) == {"codec_pee_blind_gate_workspace_bytes", "codec_pee_blind_plan_gate",
                                                       "codec_pee_blind_embed_gate"}
    assert path in build._common_deps()
    assert os.path.join(build.HERE, "csrc", "codec_blind_gate.hip") in build.SRCS
    assert _lib.KERNEL_TAGS[58] == "k_blind_rows_gate" and "#define CODEC_K_BLIND_ROWS_GATE 58" in hdr
    assert f"#define CODEC_PEE_BLIND_FLAG_GATED {_lib.BLIND_FLAG_GATED}" in hdr
    assert f"#define CODEC_PEE_BLIND_FLAG_GATE_SHIFT {_lib.BLIND_FLAG_GATE_SHIFT}" in hdr
    for name in _lib.EXPORTS_BLIND_GATE:   # the loader binds them: argument counts as declared
        m = re.search(rf"{name}\s*\(([^)]*)\)", hdr, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib._SIGS_BLIND_GATE[name][1]), name
    # the other blind headers keep their entry sets
    for h, n in (("codec_tcc_blind.h", 5), ("codec_tcc_blind_auto.h", 3)):
        text = open(os.path.join(build.INC, h)).read()
        assert len(set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", text, re.M))) == n
