"""Gated MED-PEE volume payloads without a GPU: the specification (tests/pee_gvol_spec.py) against
its scalar restatement and the known-answer file, the rule's properties, the 128-bit witness,
the open gate against the ungated volume rule, the public interface's argument errors and the
library's lists."""
import json
import os
import re

import numpy as np
import pytest

import pee_gate_spec as G
import pee_gvol_spec as S
import pee_volume_spec as V

HERE = os.path.dirname(os.path.abspath(__file__))


def _kats():
    with open(os.path.join(HERE, "golden", "pee_gvol_kat.json")) as f:
        return json.load(f)


def _kat_id(k):
    return f"{k['source']}-t{k['tmax']}-g{k['g_fixed']}-N{k['N']}"


def _same_plan(a, b):
    for k in ("status", "T", "gate", "total", "requested", "capacity"):
        assert int(a[k]) == int(b[k]), k
    for k in ("n", "t", "g", "off"):
        assert [int(v) for v in a[k]] == [int(v) for v in b[k]], k


@pytest.mark.parametrize("k", _kats(), ids=_kat_id)
def test_spec_matches_known_answers(k):
    """The spec, the scalar restatement and the file agree; per case sum n_b = total, off is
    the prefix of n and every K_b(T_b, j_b) >= n_b."""
    tables = S.source_tables(k["source"], k["tmax"], k["g_fixed"])
    assert len(tables) == k["B"]
    for policy in S.POLICIES:
        want = k[policy]
        got = S.plan(tables, k["N"], policy, k["g_fixed"])
        _same_plan(got, want)
        _same_plan(S.plan_scalar(tables, k["N"], policy, k["g_fixed"]), want)
        n = [int(v) for v in got["n"]]
        assert sum(n) == got["total"] and got["requested"] == k["N"]
        assert [int(v) for v in got["off"]] == [sum(n[:b]) for b in range(len(n) + 1)]
        for b, (nb, hb) in enumerate(tables):
            j = 0 if k["g_fixed"] is not None else G.GATES.index(int(got["g"][b]))
            assert S.K_of(hb, int(got["t"][b]), j) >= n[b], b
            assert 1 <= int(got["t"][b]) <= k["tmax"]
            if n[b] == 0:
                assert int(got["t"][b]) == 1 and int(got["g"][b]) == (k["g_fixed"] if k["g_fixed"] is not None else 0)


def test_known_answer_file_is_the_generators():
    """The committed file lists the generator's cases with the generator's N."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_pee_gvol_golden",
                                                  os.path.join(HERE, "golden", "make_pee_gvol_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    kats = _kats()
    assert len(kats) == len(gen.CASES)
    for k, (source, tmax, g_fixed, rule) in zip(kats, gen.CASES):
        assert (k["source"], k["tmax"], k["g_fixed"], k["rule"]) == (source, tmax, g_fixed, rule)
        assert k["N"] == gen.case_n(S.source_tables(source, tmax, g_fixed), g_fixed, rule)
    # the cases the plan must cover: every BATCHES stack, B = 1, more than one scan round, N = 0,
    # N at the capacity and one bit over it (status 1), the images, the synthetic tables
    srcs = {k["source"] for k in kats}
    assert set(V.BATCHES) | {"pe", "torax", "witness1"} <= srcs and any(k["B"] == 1 for k in kats)
    assert any(k["B"] > 1024 for k in kats) and any(k["N"] == 0 for k in kats)
    assert any(k["rule"] == "cap" and k["even"]["status"] == 0 for k in kats)
    assert any(k["rule"] == "over" and k["even"]["status"] == 1 and k["even"]["total"] == k["N"] - 1 for k in kats)


def test_issue_figures():
    """The choices the rule was prototyped on (the four 256 x 256 quadrants of each image)."""
    want = {("pe", 4096): (1, 1), ("pe", 16384): (2, 6), ("pe", 32768): (5, 65535),
            ("torax", 4096): (1, 0), ("torax", 16384): (1, 6), ("torax", 32768): (4, 16)}
    for (name, N), (T, gate) in want.items():
        p = S.plan(S.source_tables(name, 16), N, "even")
        assert (p["status"], p["T"], p["gate"]) == (0, T, gate), (name, N)


@pytest.mark.parametrize("name", ["5x64x96", "3x33x47", "4x32x64", "1100x8x16"])
@pytest.mark.parametrize("policy", S.POLICIES)
def test_open_gate_fixed_is_the_ungated_volume_rule(name, policy):
    """Gate 65535 fixed: every candidate is active, the one-column capacities are the ungated
    curves, and the plan is pee_volume_spec.plan's."""
    covers, maxval = S.stack(name)
    caps = V.curves(covers, 16, maxval)
    tables = S.source_tables(name, 16, 65535)
    for b, (n, hs) in enumerate(tables):
        assert n[0] == (covers.shape[1] // 2) * (covers.shape[2] // 2) and not any(n[1:])
        assert list(np.cumsum([row[0] for row in hs])) == list(caps[b])
    total = int(caps[:, -1].sum())
    for N in (0, 1, total // 3, total, total + 1):
        want = V.plan(caps, N, policy)
        for got in (S.plan(tables, N, policy, 65535), S.plan_scalar(tables, N, policy, 65535)):
            for key in ("status", "T", "total", "requested", "capacity"):
                assert int(got[key]) == int(want[key]), key
            for key in ("n", "t", "off"):
                assert [int(v) for v in got[key]] == [int(v) for v in want[key]], key
            assert got["gate"] == 65535 and set(int(v) for v in got["g"]) == {65535}


@pytest.mark.parametrize("source,rule", [("witness1", "quarter"), ("witness1", "half"), ("witness2", "third")])
def test_128_bit_witness(source, rule):
    """On the 31-slice 2^26 tables the cross-products pass 2^64, and comparing them modulo 2^64
    picks another (T*, j*) than the exact comparison: the known answers (and the GPU test that
    checks the kernel against them) would fail with a 64-bit comparison."""
    k = next(k for k in _kats() if (k["source"], k["rule"]) == (source, rule))
    tables = S.source_tables(source, 16)
    n, hs = S.sum_tables(tables)
    assert len(tables) == 31 and all(sum(t[0]) == 1 << 26 for t in tables)
    exact = S.select_scalar(n, hs, k["N"])
    wrapped = S.select_scalar(n, hs, k["N"], wrap=2 ** 64)
    assert exact[3] and wrapped[3]
    assert exact[:2] == (k["even"]["T"], G.GATES.index(k["even"]["gate"]))
    assert wrapped[:2] != exact[:2], (exact, wrapped)
    # the chosen pair's products really are beyond 64 bits
    T, j, K, _ok = exact
    A = 2 * T * T * (sum(n[:j + 1]) - K) + sum(hs[u][g] * (u * u + (u + 1) ** 2) for u in range(T) for g in range(j + 1))
    assert A * K >= 2 ** 64
    # and the plan that follows differs too
    assert S.plan_scalar(tables, k["N"], "even", wrap=2 ** 64)["n"] != k["even"]["n"]
    # the per-slice products stay below 2^62 at the bounds
    for nb, hb in tables[:3]:
        assert 2 * 256 * (1 << 26) * (1 << 26) + 481 * (1 << 52) < 2 ** 62 and sum(nb) <= 1 << 26


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("policy", S.POLICIES)
def test_plan_properties_on_random_tables(seed, policy):
    rng = np.random.default_rng(1200 + seed)
    B, tmax = int(rng.integers(1, 12)), int(rng.integers(1, 17))
    top = int(rng.choice([2, 40, 5000]))
    tables = []
    for b in range(B):
        hs = rng.integers(0, top, (tmax, 16))
        if rng.random() < 0.2:
            hs[:] = 0
        n = hs.sum(axis=0) + rng.integers(0, top, 16)
        tables.append(([int(v) for v in n], [[int(v) for v in r] for r in hs]))
    _n, hsum = S.sum_tables(tables)
    cap = S.K_of(hsum, tmax, 15)
    for N in sorted({0, 1, cap // 3, max(0, cap - 1), cap, cap + 7}):
        p = S.plan(tables, N, policy)
        _same_plan(p, S.plan_scalar(tables, N, policy))
        assert p["status"] == (1 if N > cap else 0) and p["total"] == min(N, cap)
        j = G.GATES.index(p["gate"])
        c = [S.K_of(t[1], p["T"], j) for t in tables]
        assert p["capacity"] == sum(c) and int(p["n"].sum()) == p["total"]
        assert all(0 <= int(p["n"][b]) <= c[b] for b in range(B))
        if p["status"]:
            assert (p["T"], p["gate"]) == (tmax, 65535)
        for b, (nb, hb) in enumerate(tables):   # the slice's choice is the per-slice rule's
            tb, jb, kb = G.select(nb, hb, int(p["n"][b]))
            assert (int(p["t"][b]), int(p["g"][b])) == (tb, G.GATES[jb]) and kb >= int(p["n"][b])


def test_argument_errors_need_no_gpu():
    import codec_tcc_amd
    from codec_tcc_amd import pee
    covers = np.zeros((3, 16, 16), np.uint16)
    for bad in ("best", -1, 65536, 1.5, True):
        with pytest.raises(ValueError, match="gate"):
            codec_tcc_amd.encode_volume(covers, b"abc", gate=bad)
    with pytest.raises(ValueError, match="scheme"):
        pee.encode_volume(covers, b"abc", gate="auto", scheme=2)
    with pytest.raises(ValueError, match="tmax"):
        pee.encode_volume(covers, b"abc", gate="auto", tmax=17)
    with pytest.raises(ValueError, match="policy"):
        pee.encode_volume(covers, b"abc", gate=6, policy="spread")
    # a codec already gated: the message keeps naming the ungated codec and now the keyword
    with pytest.raises(ValueError, match=r"ungated.*embed_volume\(\.\.\., gate=\)"):
        pee.check_gvol_args(6, None, 16, 64)
    with pytest.raises(ValueError, match="ungated"):
        pee.check_gvol_args("auto", "auto", 16, 64)
    gated = object.__new__(pee.PeeCodec)   # embed_volume judges its arguments before anything else
    gated.gate, gated.tmax, gated.nc, gated.scheme = 6, 16, 64, 1
    with pytest.raises(ValueError, match="ungated"):
        gated.embed_volume(covers, b"abc", gate="auto")
    with pytest.raises(ValueError, match="2\\^26"):
        pee.check_gvol_args(None, "auto", 16, (1 << 26) + 1)
    pee.check_gvol_args(None, None, 64, 1 << 28)      # ungated: the gate's bounds do not apply
    pee.check_gvol_args(None, "auto", 16, 1 << 26)
    pee.check_gvol_args(None, 0, 1, 1)
    with pytest.raises(ValueError):
        S.plan([([0] * 16, [[0] * 16])], 3, "spread")
    with pytest.raises(ValueError):
        S.plan([([0] * 16, [[0] * 16])], 2 ** 31)


def test_library_lists_the_gvol_entries():
    import ctypes
    from codec_tcc_amd import _lib, build
    hdr = open(os.path.join(build.INC, "codec_tcc_gvol.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS_GVOL) == {"codec_pee_gvol_workspace_bytes", "codec_pee_gvol_plan",
                                                  "codec_pee_gvol_embed", "codec_pee_gvol_extract"}
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_EXT) | set(_lib.EXPORTS_CRC) | set(_lib.EXPORTS_VOL) | \
        set(_lib.EXPORTS_GATE)
    assert not set(_lib.EXPORTS_GVOL) & others
    assert _lib.KERNEL_TAGS[42] == "k_gvol_plan" and "#define CODEC_K_GVOL_PLAN 42" in hdr
    assert ctypes.sizeof(_lib.PeeGvolInfo) == 40 and _lib.PEE_GVOL_INFO_BYTES % 8 == 0
    assert [f[0] for f in _lib.PeeGvolInfo._fields_[:8]] == [f[0] for f in _lib.PeeVolumeInfo._fields_]
    for name, (_res, args) in _lib._SIGS_GVOL.items():   # the binding's arity is the header's
        m = re.search(name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == len(args), name


def test_new_sources_are_in_the_build_digest(tmp_path):
    from codec_tcc_amd import build
    src = os.path.join(build.HERE, "csrc", "codec_gvol.hip")
    inc = os.path.join(build.INC, "codec_tcc_gvol.h")
    assert src in build.SRCS and inc in build._common_deps()
    # the digest covers both: it is the digest of exactly SRCS + _common_deps(), in order
    paths = build.SRCS + build._common_deps()
    assert build.source_digest() == build._digest(paths, build.FLAGS)
    without = [p for p in paths if p not in (src, inc)]
    assert build._digest(without, build.FLAGS) != build.source_digest()
