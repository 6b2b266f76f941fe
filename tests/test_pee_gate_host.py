"""Smoothness-gated MED-PEE without a GPU: the specification (tests/pee_gate_spec.py) against
its scalar restatement (tests/pee_gate_scalar.py), the known-answer file and the ungated oracle,
the capacity table against direct counts, the selection rule against brute force, and the
public interface's host-side halves: check_records, the container's scheme byte 3, argument
errors."""
import importlib.util
import json
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import pee_covers as PC
import pee_gate_scalar as GS
import pee_gate_spec as G
from codec_tcc_amd import _lib, container, pee, pipeline, synth
from oracle import pee_cpu as P

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("make_pee_gate_golden",
                                                  os.path.join(HERE, "golden", "make_pee_gate_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _kats():
    with open(os.path.join(HERE, "golden", "pee_gate_kat.json")) as f:
        return json.load(f)["cases"]


def _same_side(a, b):
    for k in ("T", "G", "L", "end", "capacity", "status", "lm_count"):
        assert int(a[k]) == int(b[k]), k
    assert [int(v) for v in a["lm"]] == [int(v) for v in b["lm"]]


@pytest.mark.parametrize("k", _kats(), ids=lambda k: f"{k['kind']}-{k['h']}x{k['w']}-T{k['T']}-G{k['G']}-{k['rule']}")
def test_spec_matches_known_answers(k):
    gen = _gen()
    img = gen.make_image(k["kind"], k["h"], k["w"], k["seed"], k["maxval"], k["clip"])
    bits = gen.payload_bits(k["nbits"], k["seed"])
    stego, side = G.embed(img, bits, k["T"], k["G"], k["maxval"])
    for f in ("L", "end", "capacity", "status", "lm_count"):
        assert int(side[f]) == k[f], f
    assert gen.sha(stego.astype(np.int64).tolist()) == k["stego_sha256"]
    assert gen.sha([int(v) for v in side["lm"]]) == k["lm_sha256"]
    got, back = G.extract(stego, side)
    np.testing.assert_array_equal(back, img)
    np.testing.assert_array_equal(got, bits[:side["L"]])
    n, hs = G.table(img, k["tmax"], k["maxval"])
    assert n.tolist() == k["n"] and hs.tolist() == k["hs"]
    for L, want in k["select"].items():
        assert list(G.select(n, hs, int(L))) == want, L


def test_known_answer_file_is_the_generators():
    gen = _gen()
    kats = _kats()
    assert len(kats) == len(gen.CASES)
    for k, c in zip(kats, gen.CASES):
        assert gen.case_record(c) == k


@pytest.mark.parametrize("dtype,maxval", [("uint16", 4095), ("uint8", None)])
@pytest.mark.parametrize("T,gate", [(1, 0), (2, 3), (3, 24), (2, 65535)])
def test_spec_equals_scalar_restatement(dtype, maxval, T, gate):
    rng = np.random.default_rng(T * 100 + gate)
    for kind in ("ct12", "above", "ends", "ladder"):
        if kind == "ct12":
            img = synth.ct12(17, 22, 3) if dtype == "uint16" else synth.GENERATORS["u8"](17, 22, 3)
        else:
            img = PC.cover(kind, 18, 21, dtype, maxval, T, 5)
        mv = PC.full_scale(img.dtype, maxval)
        cap = G.embed(img, [], T, gate, maxval)[1]["capacity"]
        for nbits in (0, cap // 2, cap, cap + 9):
            bits = rng.integers(0, 2, nbits).astype(np.uint8)
            st, side = G.embed(img, bits, T, gate, maxval)
            st_s, side_s = GS.embed(img.astype(np.int64).tolist(), bits.tolist(), T, gate, mv)
            assert st.astype(np.int64).tolist() == st_s
            _same_side(side, side_s)
            b1, c1 = G.extract(st, side)
            b2, c2 = GS.extract(st_s, side_s)
            assert b1.tolist() == b2 and c1.astype(np.int64).tolist() == c2
            np.testing.assert_array_equal(c1, img)
        n, hs = G.table(img, 6, maxval)
        n_s, hs_s = GS.table(img.astype(np.int64).tolist(), 6, mv)
        assert n.tolist() == n_s and hs.tolist() == hs_s


def test_gate_65535_is_the_ungated_oracle_on_pee_kat():
    """At G = 65535 every candidate is active: the spec is oracle.pee_cpu bit for bit, on the
    ungated scheme's own known-answer inputs."""
    spec = importlib.util.spec_from_file_location("make_pee_golden", os.path.join(HERE, "golden", "make_pee_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "pee_kat.json")) as f:
        kat = json.load(f)
    assert len(kat) == len(gen.CASES)
    for c, k in zip(gen.CASES, kat):
        img, kbits, T, maxval = gen.case_inputs(c)
        for bits in (kbits, kbits[:0], gen.payload_bits(kbits.size + 50, c[3])):
            st0, s0 = P.pee_embed(img, bits, T, maxval, truncate=True)
            st1, s1 = G.embed(img, bits, T, 65535, maxval)
            np.testing.assert_array_equal(st0, st1)
            for f in ("T", "L", "end", "capacity", "status"):
                assert s0[f] == s1[f], f
            if bits is kbits:
                assert (s1["L"], s1["end"], s1["capacity"], s1["status"]) == (k["L"], k["end"], k["capacity"], k["status"])
                assert int(s1["lm"].sum()) == k["lm_ones"]
            np.testing.assert_array_equal(s0["lm"], s1["lm"])
            b0, c0 = P.pee_extract(st0, s0)
            b1, c1 = G.extract(st1, s1)
            np.testing.assert_array_equal(b0, b1)
            np.testing.assert_array_equal(c0, c1)


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("gate", [0, 2, 16, 700])
def test_round_trip_is_exact_on_every_cover_kind(kind, gate):
    for dtype, maxval, T in (("uint16", 4095, 2), ("uint8", None, 3), ("uint16", None, 1)):
        img = PC.cover(kind, 22, 26, dtype, maxval, T, 7)
        cap = G.embed(img, [], T, gate, maxval)[1]["capacity"]
        for nbits in (0, cap // 3, cap, cap + 5):
            bits = G.payload_bits(nbits, nbits)
            st, side = G.embed(img, bits, T, gate, maxval)
            got, back = G.extract(st, side)
            np.testing.assert_array_equal(back, img)
            np.testing.assert_array_equal(got, bits[:min(nbits, cap)])
            assert side["status"] == (1 if nbits > cap else 0)
            # inactive candidates are untouched and flag nothing
            x, a, b, c = P._grids(img)
            inact = G.roughness(a, b, c) > gate
            assert np.array_equal(st[1::2, 1::2][:x.shape[0], :x.shape[1]][inact], x[inact].astype(img.dtype))
            lm = np.zeros(x.size, bool)
            lm[:side["end"] + 1] = side["lm"]
            assert not (lm & inact.ravel()).any()


def test_table_K_is_the_direct_capacity():
    tmax = 7
    for img, maxval in ((synth.ct12(40, 56, 1), 4095), (PC.cover("above", 30, 34, "uint16", 4095, 2, 3), 4095),
                        (PC.cover("ends", 24, 24, "uint8", None, 2, 4), None)):
        n, hs = G.table(img, tmax, maxval)
        K = G.K_table(hs)
        x, a, b, c = P._grids(img)
        d = G.roughness(a, b, c)
        assert int(n.sum()) == x.size
        for j, gate in enumerate(G.GATES):
            assert int(n[:j + 1].sum()) == int((d <= gate).sum())
            for T in range(1, tmax + 1):
                assert int(K[T - 1][j]) == G.embed(img, [], T, gate, maxval)[1]["capacity"], (T, gate)
        # an arbitrary gate: the one-column table
        _n1, hs1 = G.table(img, tmax, maxval, g_fixed=5)
        for T in range(1, tmax + 1):
            assert int(G.K_table(hs1)[T - 1][0]) == G.embed(img, [], T, 5, maxval)[1]["capacity"]
        assert G.gate_class(np.array([0, 1, 4, 5, 6, 7, 8, 9, 128, 129, 65535])).tolist() == \
            [0, 1, 4, 5, 5, 6, 6, 7, 14, 15, 15]


def _brute(n, hs, L, t_fixed=0):
    """The rule from its definition: exact fractions over every pair."""
    tmax = len(hs)
    ts = [t_fixed] if t_fixed else range(1, tmax + 1)
    if L == 0:
        T = t_fixed or 1
        return T, 0, sum(hs[u][0] for u in range(T))
    best = None
    for T in ts:
        for j in range(16):
            K = sum(hs[u][g] for u in range(T) for g in range(j + 1))
            if K >= L and K > 0:
                N = sum(n[:j + 1])
                A = 2 * T * T * (N - K) + sum(hs[u][g] * (u * u + (u + 1) ** 2) for u in range(T) for g in range(j + 1))
                key = (Fraction(A, K), T, j)
                if best is None or key < best[0]:
                    best = (key, K)
    if best is None:
        T = t_fixed or tmax
        return T, 15, sum(hs[u][g] for u in range(T) for g in range(16))
    return best[0][1], best[0][2], best[1]


def test_selection_rule_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(120):
        tmax = int(rng.integers(1, 7))
        hs = rng.integers(0, 4 if trial % 3 else 2, (tmax, 16))
        if trial % 5 == 0:
            hs[:, rng.integers(0, 16, 6)] = 0
        if trial % 7 == 0:   # equal columns and rows: ties in A / K
            hs[:] = hs[0, 0]
        n = hs.sum(axis=0) + rng.integers(0, 3, 16)
        total = int(hs.sum())
        for L in {0, 1, 2, total // 2, total, total + 1}:
            for tf in (0, int(rng.integers(1, tmax + 1))):
                want = _brute(n.tolist(), hs.tolist(), L, tf)
                assert G.select(n, hs, L, tf) == want, (trial, L, tf)
                assert tuple(GS.select(n.tolist(), hs.tolist(), L, tf)) == want, (trial, L, tf)
    # a tie broken by the smaller T, then the smaller j: two classes with the same cost per bit
    hs = np.zeros((2, 16), np.int64)
    hs[0, 0] = hs[0, 1] = 4
    n = hs.sum(axis=0)
    assert G.select(n, hs, 4) == (1, 0, 4)
    # L = 0, and no feasible pair
    assert G.select(n, hs, 0) == (1, 0, 4) and G.select(n, hs, 0, 2) == (2, 0, 4)
    assert G.select(n, hs, 9) == (2, 15, 8) and G.select(n, hs, 9, 1) == (1, 15, 8)
    # the largest table the entries accept: every product below 2^64
    big = np.zeros((16, 16), np.int64)
    big[15, 15] = 1 << 26
    T, j, K = G.select(big.sum(axis=0), big, 1 << 26)
    assert (T, j, K) == (16, 15, 1 << 26)
    A = 2 * 256 * 0 + (1 << 26) * (15 * 15 + 16 * 16)
    assert A * K < 1 << 64


def test_quality_gain_of_the_rule_on_the_reference_images():
    """The issue's table from the spec alone: gate='auto', T='auto' beats T='auto' by >= 2 dB."""
    imgs = np.load(os.path.join(HERE, "golden", "images.npz"))
    for name, maxval in (("pe", 4095), ("torax", 255)):
        img = imgs[name]
        for nbits in (8192, 16384):
            bits = G.payload_bits(nbits, 1)
            T0 = P.select_T(img, nbits, 16, maxval)
            st0, _ = P.pee_embed(img, bits, T0, maxval, truncate=True)
            n, hs = G.table(img, 16, maxval)
            T, j, _K = G.select(n, hs, nbits)
            st1, side = G.embed(img, bits, T, G.GATES[j], maxval)
            assert side["status"] == 0
            gain = G.psnr(st1, img, maxval) - G.psnr(st0, img, maxval)
            assert gain >= 2.0, (name, nbits, gain)


# ---------------------------------------------------------------- records, files, arguments
def _rec(h=16, w=16, **kw):
    base = dict(T=2, maxval=4095, L=5, end=20, status=0)
    base.update(kw)
    return pee.make_record(h, w, **base)


def test_check_records_takes_the_gate_field():
    args = dict(scheme=1, payload_words=1, lm_words=1, bytes=2)
    for gate in (None, 0, 3, 65535):
        r = _rec(gate=gate)
        assert int(r.reserved[1]) == (0 if gate is None else gate + 1)
        pee.check_records([r], 16, 16, **args)
    for bad in (-1, 65537, 1 << 20):
        r = _rec()
        r.reserved[1] = bad
        with pytest.raises(ValueError, match=r"reserved\[1\]"):
            pee.check_records([r], 16, 16, **args)
    # a gated record's other fields are judged as ever
    for kw, field in ((dict(L=30, end=20), "L"), (dict(L=0, end=3), "end"), (dict(end=64), "end"),
                      (dict(status=1, end=10), "end"), (dict(T=0), "T"), (dict(L=-1), "L")):
        with pytest.raises(ValueError, match=field):
            pee.check_records([_rec(gate=8, **kw)], 16, 16, **args)
    r = _rec(gate=8)
    r.tile_end = 5
    with pytest.raises(ValueError, match="tile_end"):
        pee.check_records([r], 16, 16, **args)


def test_gate_argument_errors_need_no_gpu():
    with pytest.raises(ValueError, match="scheme 1"):
        pee.PeeCodec(1, 16, 16, scheme=2, gate=4)
    with pytest.raises(ValueError, match="scheme 1"):
        pee.encode(np.zeros((16, 16), np.uint16), ["a"], scheme=2, gate="auto")
    for bad in (-1, 65536, "best", 2.5, True):
        with pytest.raises(ValueError, match="gate"):
            pee.check_gate_args(bad, 2, 16, 64)
    with pytest.raises(ValueError, match="tmax"):
        pee.check_gate_args("auto", "auto", 17, 64)
    with pytest.raises(ValueError, match="fixed T"):
        pee.check_gate_args("auto", 9, 8, 64)
    with pytest.raises(ValueError, match="2\\^26"):
        pee.check_gate_args(3, 2, 16, (1 << 26) + 1)
    pee.check_gate_args(None, 2, 64, 1 << 30, 2)   # no gate: nothing to check
    pee.check_gate_args(0, 2, 16, 1 << 26)
    pee.check_gate_args("auto", "auto", 16, 64)


def _gated_file(tmp_path, gate=96, crc=False, name="g.stgc"):
    img = synth.ct12(16, 24, 2)
    cap = G.embed(img, [], 2, gate, 4095)[1]["capacity"]
    assert cap >= 2
    bits = G.payload_bits(cap // 2, 3)
    stego, side = G.embed(img, bits, 2, gate, 4095)
    lmb = container.lm_blob(side["lm"])
    hdr = container.create_pee_gate_header("raw", 2, 24, 16, 2, side["L"], side["end"], 4095, side["status"], len(lmb),
                                           gate)
    if crc:
        hdr += container.pee_crc_extension(0x12345678, 0x9ABCDEF0)
    path = str(tmp_path / name)
    container.create_binary_file(path, hdr, container.encode_stego_raw(stego), lmb)
    return path, img, bits, stego, side


def test_container_scheme_byte_3_round_trip_and_refusals(tmp_path):
    path, _img, _bits, stego, side = _gated_file(tmp_path, crc=True)
    raw = open(path, "rb").read()
    assert container.pee_scheme(raw) == 3 and raw[8 + 3] == 3
    md, blob, data = container.parse_pee_gate_bytes(raw)
    assert (md["gate"], md["T"], md["L"], md["end"], md["status"], md["scheme"]) == (96, 2, side["L"], side["end"], 0, 3)
    assert (md["cover_crc32"], md["payload_crc32"]) == (0x12345678, 0x9ABCDEF0)
    np.testing.assert_array_equal(container.lm_from_blob(blob, md["end"]), side["lm"])
    np.testing.assert_array_equal(container.decode_stego_raw(data, 16, 24), stego)
    pf = pipeline.read_pee_bytes(raw)
    assert pf.scheme == 1 and int(pf.records[0][0].reserved[1]) == 97 and pf.md["gate"] == 96
    # an old-style parse of a gated file refuses it (scheme 1's and scheme 2's readers)
    with pytest.raises(ValueError, match="gated"):
        container.parse_pee_bytes(raw)
    with pytest.raises(ValueError):
        container.parse_pee2_bytes(raw)
    # a reader that knows scheme bytes 0 and 2 only sees an unknown one
    assert raw[11] not in (0, container.PEE_SCHEME2)
    # ungated files are no gated ones, and their bytes are what they were
    one = container.create_pee_header("raw", 2, 8, 8, 2, 0, -1, 4095, 0, 0)
    assert one == struct.pack(">BBBBIIiiiiiI", 16, 0, 2, 0, 8, 8, 2, 0, -1, 4095, 0, 0)
    p1 = str(tmp_path / "one.stgc")
    container.create_binary_file(p1, one, b"x" * 128, b"")
    with pytest.raises(ValueError, match="gated"):
        container.parse_pee_gate_bytes(open(p1, "rb").read())
    # a header cut inside the gate field, and inside the checksum extension behind it
    n0 = struct.calcsize(">BBBBIIiiiiiI")
    hdr = raw[8:8 + struct.unpack(">I", raw[4:8])[0]]
    body = raw[8 + len(hdr):]
    for cut, what in ((n0, "truncated"), (n0 + 1, "truncated"), (n0 + 2 + 5, "checksum extension")):
        short = raw[:4] + struct.pack(">I", cut) + hdr[:cut] + body
        with pytest.raises(ValueError, match=what):
            container.parse_pee_gate_bytes(short)
        with pytest.raises(ValueError, match=what):
            pipeline.read_pee_bytes(short)
    with pytest.raises(ValueError, match="gate"):
        container.create_pee_gate_header("raw", 2, 8, 8, 2, 0, -1, 4095, 0, 0, 65536)
    # header fields that contradict each other are refused on the host, as for ungated files
    bad = bytearray(raw)
    bad[8 + 12:8 + 16] = struct.pack(">i", 0)   # T = 0
    with pytest.raises(ValueError, match="T"):
        pipeline.read_pee_bytes(bytes(bad))
    bad = bytearray(raw)
    bad[8 + 16:8 + 20] = struct.pack(">i", side["end"] + 2)   # L > end + 1
    with pytest.raises(ValueError, match="L"):
        pipeline.read_pee_bytes(bytes(bad))


def test_every_gate_entry_is_listed_in_the_loader():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "codec_tcc_gate.h")).read()
    import re
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_GATE) and len(declared) == 5
    assert _lib.GATES == G.GATES == GS.GATES
    assert _lib.KERNEL_TAGS[41] == "k_pee_gate_table"
    assert "#define CODEC_K_PEE_GATE_TABLE 41" in hdr and "tests/pee_gate_spec.py" in hdr
