"""MED-PEE on range-end, extreme-error and out-of-range covers (tests/pee_covers.py): dense
location maps, unsafe candidates at both range ends, errors of +-maxval, pixels above maxval
and every comparison edge of the classification -- none of which the smooth synthetic covers
of the other PEE tests reach.  One batch holds one slice of every kind, so neighbouring slices
differ widely in density.  The CPU oracle (oracle/pee_cpu.py) is the specification: the CPU
tests check it against itself (reversibility), against the scalar restatement
(tests/pee_scalar.py) and that the batches do contain the edges; the GPU tests compare every
launch path with it bit for bit."""
import functools

import numpy as np
import pytest

import pee_covers as PC
import pee_scalar as S
from oracle import pee_cpu as P
from test_pee import PATHS
from test_pee2_auto import spec_auto

KINDS = PC.KINDS
# (dtype, maxval, T) of the fixed-T batches
ROWS = [("uint16", None, 2), ("uint16", 4095, 1), ("uint16", 4095, 16), ("uint16", 4095, 64), ("uint8", None, 2),
        ("uint8", 127, 4)]
FIXED_SHAPES = [(72, 512),     # 2.25 look-back chunks, 9 tiles, W % 8 == 0, ragged last chunk
                (37, 53)]      # odd sizes: the two-pass path
# T="auto": the resident kernel's LIN launch (8 192 items), its cursor launch, and 72 x 512
AUTO_SHAPES = [(1024, 128), (130, 512), (72, 512)]
AUTO_MAXVALS = [4095, None]
AUTO_TMAX = [1, 5, 16]
# the unfused capacity pass + per-slice-T embed alone: tmax beyond the fused kernels' 16, uint8
WIDE = [("uint16", 4095, 64), ("uint8", 127, 16)]
# scheme 2 (four sublattice passes)
MULTI_ROWS = [("uint16", 4095, 16), ("uint16", 4095, 1), ("uint8", 127, 4)]
MULTI_AUTO_ROWS = [("uint16", 4095), ("uint8", 127)]
MULTI_TMAX = 6


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _covers(h, w, dtype, maxval, T):
    """One slice of every kind; computed once, read-only."""
    cov = PC.batch(h, w, dtype, maxval, T, seed=5)
    cov.setflags(write=False)
    return cov


# payload lengths rotate over the slices: 0, 1, capacity // 2, exactly the capacity, capacity + 9
# (truncated: status 1, end = nc - 1, the full-length map).  flat_zero always gets its whole nc
# (= its capacity); the two variants (out of place / in place) give every other kind two
# different lengths, and flat_max and one checker a non-empty payload (their all-ones maps)
_LEN_RULES = ({"flat_zero": "cap", "flat_max": "over", "ends": "half", "checker": "one", "checker_inv": "zero",
               "top_band": "cap", "above": "over", "ladder": "half"},
              {"flat_zero": "cap", "flat_max": "one", "ends": "over", "checker": "zero", "checker_inv": "one",
               "top_band": "half", "above": "cap", "ladder": "over"})


def _length(rule, cap):
    return {"zero": 0, "one": 1, "half": cap // 2, "cap": cap, "over": cap + 9}[rule]


@functools.lru_cache(maxsize=None)
def _fixed_case(h, w, dtype, maxval, T, variant):
    """(covers, payloads, [(stego, side)]) of a fixed-T batch: the oracle's answers, shared by
    every launch path's test."""
    cov = _covers(h, w, dtype, maxval, T)
    pays, exp = [], []
    for i, kind in enumerate(KINDS):
        n = _length(_LEN_RULES[variant][kind], P.capacity(cov[i], T, maxval))
        pays.append(_bits(n, 100 * variant + i))
        exp.append(P.pee_embed(cov[i], pays[i], T, maxval=maxval, truncate=True))
    return cov, tuple(pays), tuple(exp)


def _auto_lengths(curves, variant):
    """Per kind a payload that selects another T: the whole nc (T = 1), nothing, exactly a
    capacity of the curve, one bit more than one, and beyond tmax's capacity (truncated)."""
    tmax = len(curves[0])
    c = dict(zip(KINDS, curves))
    mid, low = tmax // 2, min(1, tmax - 1)
    if variant == 0:
        return [int(c["flat_zero"][0]), 9, int(c["ends"][mid]), 0, 1, int(c["top_band"][-1]),
                int(c["above"][low]) + 1, int(c["ladder"][-1]) + 37]
    return [int(c["flat_zero"][0]), 1, int(c["ends"][-1]) + 37, 1, 0, int(c["top_band"][low]) + 1,
            int(c["above"][-1]), int(c["ladder"][mid])]


@functools.lru_cache(maxsize=None)
def _auto_case(h, w, dtype, maxval, tmax, variant):
    """(covers, payloads, curves, [(T, stego, side)]) of a T="auto" batch."""
    cov = _covers(h, w, dtype, maxval, tmax)
    curves = np.stack([P.capacity_curve(c, tmax, maxval) for c in cov])
    lens = _auto_lengths(curves, variant)
    pays = tuple(_bits(n, 300 + 100 * variant + i) for i, n in enumerate(lens))
    exp = []
    for i in range(len(KINDS)):
        T = P.select_T(cov[i], lens[i], tmax, maxval)
        exp.append((T,) + P.pee_embed(cov[i], pays[i], T, maxval=maxval, truncate=True))
    return cov, pays, curves, tuple(exp)


@functools.lru_cache(maxsize=None)
def _multi_case(h, w, dtype, maxval, T):
    """Scheme 2, fixed T: payloads that stop in pass 0, spill into pass 2, fill all four passes
    exactly, and overflow.  A payload is a prefix of the probe whose truncated embedding gave
    the passes' capacities, so each pass meets the running stego the probe met."""
    cov = _covers(h, w, dtype, maxval, T)
    pays, exp = [], []
    for i in range(len(KINDS)):
        probe = _bits(h * w + 50, 700 + i)
        caps = [ps["L"] for ps in P.pee_embed_multi(cov[i], probe, T, maxval=maxval)[1]["passes"]]
        n = [caps[0] // 2, caps[0] + caps[1] + (caps[2] + 1) // 2, sum(caps), sum(caps) + 50][i % 4]
        if sum(caps) == 0:   # flat_max, the checkers: no pass holds a bit -- four all-ones maps
            n = 50
        pays.append(probe[:n])
        exp.append(P.pee_embed_multi(cov[i], pays[i], T, maxval=maxval))
    return cov, tuple(pays), tuple(exp)


@functools.lru_cache(maxsize=None)
def _multi_auto_case(h, w, dtype, maxval):
    """Scheme 2, T="auto" over 1..MULTI_TMAX: empty, one bit, inside T = 1, just past T = 1,
    between T = 2 and 3, just past T = 4, beyond tmax."""
    cov = _covers(h, w, dtype, maxval, MULTI_TMAX)
    pays, exp = [], []
    for i in range(len(KINDS)):
        probe = _bits(h * w + 50, 800 + i)
        full = {T: P.pee_embed_multi(cov[i], probe, T, maxval=maxval)[1]["L"] for T in (1, 2, 3, 4, MULTI_TMAX)}
        n = [full[MULTI_TMAX] + 60, full[1] // 2, full[1] + 7, 1, (full[2] + full[3]) // 2, full[4] + 9, 0,
             full[MULTI_TMAX] + 60][i]
        pays.append(_bits(n, 900 + i))
        exp.append(spec_auto(cov[i], pays[i], 1, MULTI_TMAX, maxval))
    return cov, tuple(pays), tuple(exp)


def _every_cover_set():
    """(h, w, dtype, maxval, T) of every batch of covers a GPU test below embeds."""
    out = [(h, w) + row for (h, w) in FIXED_SHAPES for row in ROWS]
    out += [(h, w, "uint16", mv, tmax) for (h, w) in AUTO_SHAPES for mv in AUTO_MAXVALS for tmax in AUTO_TMAX]
    out += [(h, w, dt, mv, tmax) for (h, w) in AUTO_SHAPES[1:] for dt, mv, tmax in WIDE]
    out += [(h, w) + row for (h, w) in FIXED_SHAPES for row in MULTI_ROWS]
    out += [(h, w, dt, mv, MULTI_TMAX) for (h, w) in FIXED_SHAPES for dt, mv in MULTI_AUTO_ROWS]
    return sorted(set(out), key=str)


def _cs_id(cs):
    return "-".join(str(v) for v in cs)


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("cs", _every_cover_set(), ids=_cs_id)
def test_oracle_reversible_on_adversarial_covers(cs):
    """pee_embed / pee_extract and the four-pass pee_embed_multi / pee_extract_multi restore
    payload and cover exactly on every kind, at 0 bits, 1 bit, half the capacity, exactly the
    capacity and 9 bits more (truncated); for a T="auto" batch at T = 1 and T = tmax."""
    h, w, dtype, maxval, T = cs
    cov = _covers(*cs)
    for i, kind in enumerate(KINDS):
        for t in sorted({1, T}) if (h, w) in AUTO_SHAPES else [T]:
            cap = P.capacity(cov[i], t, maxval)
            for n in sorted({0, 1, cap // 2, cap, cap + 9}):
                bits = _bits(n, n + i)
                st, side = P.pee_embed(cov[i], bits, t, maxval=maxval, truncate=True)
                assert side["status"] == (1 if n > cap else 0) and side["L"] == min(n, cap), (kind, t, n)
                got, back = P.pee_extract(st, side)
                np.testing.assert_array_equal(got, bits[: side["L"]])
                np.testing.assert_array_equal(back, cov[i])
        if (h, w) in FIXED_SHAPES:
            probe = _bits(h * w + 50, 40 + i)
            total = P.pee_embed_multi(cov[i], probe, T, maxval=maxval)[1]["L"]
            for n in sorted({0, total // 3, total, total + 50}):
                st, side = P.pee_embed_multi(cov[i], probe[:n], T, maxval=maxval)
                assert side["L"] == min(n, total) and side["status"] == (1 if n > total else 0), (kind, n)
                got, back = P.pee_extract_multi(st, side)
                np.testing.assert_array_equal(got, probe[: side["L"]])
                np.testing.assert_array_equal(back, cov[i])


@pytest.mark.parametrize("cs", [c for c in _every_cover_set() if c[0] * c[1] <= 72 * 512], ids=_cs_id)
def test_scalar_restatement_agrees_on_adversarial_covers(cs):
    """tests/pee_scalar.py (one candidate at a time) gives the oracle's stego, `end` and map."""
    h, w, dtype, maxval, T = cs
    cov = _covers(*cs)
    mv = PC.full_scale(dtype, maxval)
    for i, kind in enumerate(KINDS):
        cap = P.capacity(cov[i], T, maxval)
        n = [cap, cap + 9, cap // 2][i % 3]
        bits = _bits(n, 60 + i)
        st, side = P.pee_embed(cov[i], bits, T, maxval=maxval, truncate=True)
        st2, side2 = S.embed(cov[i].tolist(), [int(b) for b in bits], T, mv)
        np.testing.assert_array_equal(np.array(st2, dtype=cov.dtype), st, err_msg=kind)
        assert (side2["end"], side2["L"], side2["capacity"], side2["status"]) == \
            (side["end"], side["L"], side["capacity"], side["status"]), kind
        np.testing.assert_array_equal(np.array(side2["lm"], bool), side["lm"], err_msg=kind)


def _edges(cov, sides, ts, maxval, tmax):
    """What one embedded batch contains, from the oracle alone."""
    mv = PC.full_scale(cov.dtype, maxval)
    d = [PC.describe(cov[i], ts[i], maxval) for i in range(len(KINDS))]
    ia = KINDS.index("above")
    return {
        "all_ones_map": any(s["end"] == x["nc"] - 1 and s["lm"].size == x["nc"] and s["lm"].all()
                            for s, x in zip(sides, d)),
        "capacity_is_nc": any(x["capacity"] == x["nc"] for x in d),
        "both_sides_unsafe": any(x["unsafe_low"] > 0 and x["unsafe_high"] > 0 for x in d),
        "e_plus_maxval": any(x["emax"] == mv for x in d),
        "e_minus_maxval": any(x["emin"] == -mv for x in d),
        "above_left_shifted": d[ia]["left_above"] / d[ia]["nc"],
        "above_capacity": P.capacity(cov[ia], tmax, maxval),
        "top_side_unsafe_shift": d[KINDS.index("top_band")]["unsafe_right_shift"],
    }


def _assert_edges(e, dtype, maxval, what):
    for key in ("all_ones_map", "capacity_is_nc", "both_sides_unsafe", "e_plus_maxval", "e_minus_maxval"):
        assert e[key], (what, key)
    if maxval is not None and maxval < np.iinfo(np.dtype(dtype)).max:   # `above` has room above maxval
        assert e["above_left_shifted"] >= 0.01, (what, e["above_left_shifted"])
        assert e["above_capacity"] > 0, what


def test_covers_reach_every_edge():
    """Every batch the GPU tests embed contains: a slice whose map is all ones through
    end = nc - 1; a slice with capacity == nc; a slice with unsafe candidates on both the 0 side
    and the maxval side; errors equal to +maxval and to -maxval; and, where maxval is below the
    dtype's maximum, an `above` slice with at least 1 % of its candidates left-shifted from
    x - T > maxval (at the T the slice is embedded with) and a non-zero capacity at the largest
    T used.  The multi-chunk 12-bit batches also hold top-side unsafe right shifts in top_band."""
    for (h, w) in FIXED_SHAPES:
        for dtype, maxval, T in ROWS:
            for variant in (0, 1):
                cov, _pays, exp = _fixed_case(h, w, dtype, maxval, T, variant)
                e = _edges(cov, [s for _st, s in exp], [T] * len(KINDS), maxval, T)
                _assert_edges(e, dtype, maxval, (h, w, dtype, maxval, T, variant))
                if maxval == 4095 and T <= 16 and h * w >= 72 * 512:
                    assert e["top_side_unsafe_shift"] > 0
    for (h, w), dtype, maxval, tmax in ([(s, "uint16", mv, t) for s in AUTO_SHAPES for mv in AUTO_MAXVALS
                                         for t in AUTO_TMAX] + [(s,) + row for s in AUTO_SHAPES[1:] for row in WIDE]):
        for variant in (0, 1):
            cov, pays, curves, exp = _auto_case(h, w, dtype, maxval, tmax, variant)
            ts = [T for T, _st, _s in exp]
            e = _edges(cov, [s for _T, _st, s in exp], ts, maxval, tmax)
            _assert_edges(e, dtype, maxval, (h, w, dtype, maxval, tmax, variant))
            # the payloads select different T, one of them beyond tmax's capacity
            assert 1 in ts and tmax in ts and len(set(ts)) >= min(3, tmax), ts
            assert any(s["status"] == 1 and T == tmax for T, _st, s in exp)
            assert any(s["status"] == 0 and s["L"] > 0 for _T, _st, s in exp)
    for (h, w) in FIXED_SHAPES:
        for dtype, maxval, T in MULTI_ROWS:
            cov, pays, exp = _multi_case(h, w, dtype, maxval, T)
            sides = [s for _st, s in exp]
            ls = [[ps["L"] for ps in s["passes"]] for s in sides]
            assert any(s["status"] == 0 and l[0] > 0 and sum(l[1:]) == 0 for s, l in zip(sides, ls))   # stops in pass 0
            assert any(s["status"] == 0 and l[2] > 0 and l[3] == 0 for s, l in zip(sides, ls))        # spills into pass 2
            assert any(s["status"] == 0 and all(ps["status"] == 1 for ps in s["passes"][:3]) and s["L"] > 0
                       for s in sides)                                                                 # fills all four
            assert any(s["status"] == 1 for s in sides)                                                # overflows
        for dtype, maxval in MULTI_AUTO_ROWS:
            cov, pays, exp = _multi_auto_case(h, w, dtype, maxval)
            ts = [T for T, _st, _s in exp]
            assert 1 in ts and any(1 < t < MULTI_TMAX for t in ts), ts
            assert any(T == MULTI_TMAX and s["status"] == 1 for T, _st, s in exp), ts


# ------------------------------------------------------------------------------------ GPU
def _records_and_maps(enc):
    """(records, per-slice location map over candidates 0..end) with one read-back each."""
    recs = enc.records()
    raw = enc.lm.cpu().numpy().view(np.uint8).reshape(len(recs), -1)
    return recs, [np.unpackbits(raw[i], bitorder="little")[: r.end + 1].astype(bool) for i, r in enumerate(recs)]


def _check_scheme1(enc, cov, sides, stegos, ts=None, what=""):
    """stego, end, status, lm_count, lm_bits (and T) against the oracle with truncate=True;
    capacity where the record is not PEE_PARTIAL (else a lower bound that holds the payload)."""
    from codec_tcc_amd import _lib
    recs, maps = _records_and_maps(enc)
    got = enc.stego.cpu().numpy()
    assert len(recs) == len(sides) == len(stegos)   # the whole batch, or its first slices (test_pee_placement.py)
    for i, kind in enumerate(KINDS[: len(sides)]):
        side, r = sides[i], recs[i]
        tag = (what, kind)
        assert (r.status, r.end) == (side["status"], side["end"]), tag
        if ts is not None:
            assert r.T == ts[i], tag
        if r.flags & _lib.PEE_PARTIAL:
            assert side["L"] <= r.capacity <= side["capacity"], tag
        else:
            assert r.capacity == side["capacity"], tag
        bad = np.flatnonzero((got[i] != stegos[i]).ravel())
        assert bad.size == 0, (tag, f"{bad.size} stego pixels differ; first at pixel {int(bad[0])}: "
                               f"got {int(got[i].ravel()[bad[0]])}, oracle {int(stegos[i].ravel()[bad[0]])}, "
                               f"cover {int(cov[i].ravel()[bad[0]])}")
        assert maps[i].size == side["lm"].size, tag
        diff = np.flatnonzero(maps[i] != side["lm"])
        assert diff.size == 0, (tag, f"{diff.size} map bits differ; first at candidate {int(diff[0])}")
        assert r.lm_count == int(side["lm"].sum()), tag


def _check_extract(codec, enc, cov, pays, embedded, inplace, cover=None):
    """codec.extract returns the exact payload prefix and the exact cover.  cover: the caller's
    out buffer of an out-of-place extract (a placed view, test_pee_placement.py)."""
    from codec_tcc_amd import framing
    words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words,
                                cover=enc.stego if inplace else cover)
    assert cover is None or inplace or back.data_ptr() == cover.data_ptr()
    host = words.cpu().numpy()
    assert len(host) == len(pays) == len(embedded)
    for i in range(len(pays)):
        np.testing.assert_array_equal(framing.unpack_bits(host[i], embedded[i]), pays[i][: embedded[i]], err_msg=KINDS[i])
    np.testing.assert_array_equal(back.cpu().numpy(), cov)


@pytest.fixture(params=sorted(PATHS))
def pee_path(request, monkeypatch):
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("dtype,maxval,T", ROWS)
@pytest.mark.parametrize("h,w", FIXED_SHAPES)
def test_gpu_fixed_T_matches_oracle(h, w, dtype, maxval, T, inplace, pee_path):
    """(a) Scheme 1 at a fixed T through every launch path of tests/test_pee.py's PATHS."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    cov, pays, exp = _fixed_case(h, w, dtype, maxval, T, int(inplace))
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T=T, maxval=maxval)
    dev = torch.from_numpy(cov.copy()).cuda()
    enc = codec.embed(dev, list(pays), stego=dev if inplace else None)
    sides = [s for _st, s in exp]
    _check_scheme1(enc, cov, sides, [st for st, _s in exp], what=pee_path)
    _check_extract(codec, enc, cov, pays, [s["L"] for s in sides], inplace)


AUTO_LAUNCHES = (("res", "1", "1", "1", "0"), ("ss", "1", "0", "1", "0"), ("unfused", "0", "1", "1", "0"),
                 ("res_nolin", "1", "1", "0", "0"), ("res512", "1", "1", "1", "512"))


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("tmax", AUTO_TMAX)
@pytest.mark.parametrize("maxval", AUTO_MAXVALS)
@pytest.mark.parametrize("h,w", AUTO_SHAPES)
def test_gpu_auto_matches_oracle(h, w, maxval, tmax, inplace, monkeypatch):
    """(b) T="auto", slice-serial forced: the resident kernel (LIN, cursor and 512-thread
    launches), the two-phase slice-serial kernel and the unfused capacity pass + embed all equal
    the oracle at select_T's T (so they equal each other); the device capacity curve equals
    capacity_curve on every kind."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_SS", "1")
    cov, pays, curves, exp = _auto_case(h, w, "uint16", maxval, tmax, int(inplace))
    ts, stegos, sides = [e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]
    for name, fused, res, lin, nth in AUTO_LAUNCHES:
        monkeypatch.setenv("CODEC_PEE_AUTO_FUSED", fused)
        monkeypatch.setenv("CODEC_PEE_RES", res)
        monkeypatch.setenv("CODEC_PEE_RES_LIN", lin)
        monkeypatch.setenv("CODEC_PEE_RES_THREADS", nth)
        codec = PeeCodec(len(KINDS), h, w, dtype="uint16", T="auto", tmax=tmax, maxval=maxval)
        dev = torch.from_numpy(cov.copy()).cuda()
        if name == "unfused":
            np.testing.assert_array_equal(codec.capacity(dev).cpu().numpy(), curves)
        enc = codec.embed(dev, list(pays), stego=dev if inplace else None)
        assert codec.t_slices.cpu().tolist() == ts, name
        _check_scheme1(enc, cov, sides, stegos, ts=ts, what=name)
        _check_extract(codec, enc, cov, pays, [s["L"] for s in sides], inplace)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("ss", ["default", "slice_serial"])
@pytest.mark.parametrize("dtype,maxval,tmax", WIDE)
@pytest.mark.parametrize("h,w", AUTO_SHAPES[1:])
def test_gpu_auto_unfused_wide(h, w, dtype, maxval, tmax, ss, inplace, monkeypatch):
    """(b) The capacity pass (k_pee_ehist) + per-slice-T embed as two launches where the fused
    kernels do not apply: tmax = 64 and uint8 with maxval 127."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_AUTO_FUSED", "0")
    if ss == "slice_serial":
        monkeypatch.setenv("CODEC_PEE_SS", "1")
    cov, pays, curves, exp = _auto_case(h, w, dtype, maxval, tmax, int(inplace))
    ts, stegos, sides = [e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T="auto", tmax=tmax, maxval=maxval)
    dev = torch.from_numpy(cov.copy()).cuda()
    np.testing.assert_array_equal(codec.capacity(dev).cpu().numpy(), curves)
    enc = codec.embed(dev, list(pays), stego=dev if inplace else None)
    assert codec.t_slices.cpu().tolist() == ts
    _check_scheme1(enc, cov, sides, stegos, ts=ts, what=ss)
    _check_extract(codec, enc, cov, pays, [s["L"] for s in sides], inplace)


def _check_multi(enc, sides, stegos, T=None, ts=None):
    """Scheme 2: stego and every pass's (L, end, status, T, lattice), capacity and map vs the oracle."""
    from codec_tcc_amd import _lib
    got = enc.stego.cpu().numpy()
    prs = enc.pass_records()
    assert len(prs[0]) == len(sides) == len(stegos)
    raw = enc.lm.cpu().numpy().view(np.uint8).reshape(4, len(sides), -1)
    for b, kind in enumerate(KINDS[: len(sides)]):
        np.testing.assert_array_equal(got[b], stegos[b], err_msg=kind)
        Tb = T if ts is None else ts[b]
        for p, ps in enumerate(sides[b]["passes"]):
            r = prs[p][b]
            assert (r.L, r.end, r.status, r.T, r.reserved[0]) == (ps["L"], ps["end"], ps["status"], Tb, p), (kind, p)
            if r.capacity < 0:    # -1: nothing was left for the pass (it skipped the slice)
                assert ps["L"] == 0 and r.end == -1, (kind, p)
            elif r.flags & _lib.PEE_PARTIAL:
                assert ps["L"] <= r.capacity <= ps["capacity"], (kind, p)
            else:
                assert r.capacity == ps["capacity"], (kind, p)
            lm = np.unpackbits(raw[p, b], bitorder="little")[: r.end + 1].astype(bool)
            np.testing.assert_array_equal(lm, ps["lm"], err_msg=f"{kind} pass {p}")
        assert enc.embedded()[b] == sides[b]["L"], kind


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("lat", ["tile", "ss"])
@pytest.mark.parametrize("p0", ["p0_scheme1", "p0_lattice"])
@pytest.mark.parametrize("dtype,maxval,T", MULTI_ROWS)
@pytest.mark.parametrize("h,w", FIXED_SHAPES)
def test_gpu_multipass_matches_oracle(h, w, dtype, maxval, T, p0, lat, inplace, monkeypatch):
    """(c) Scheme 2 at a fixed T: pass 0 through scheme 1's kernels or the lattice kernels, the
    passes as tile launches or the slice-serial kernel, against pee_embed_multi."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    if p0 == "p0_lattice":
        monkeypatch.setenv("CODEC_PEE_MULTI_P0", "0")
    monkeypatch.setenv("CODEC_PEE_LAT_SS", "0" if lat == "tile" else "1")
    cov, pays, exp = _multi_case(h, w, dtype, maxval, T)
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T=T, maxval=maxval, scheme=2)
    dev = torch.from_numpy(cov.copy()).cuda()
    enc = codec.embed(dev, list(pays), stego=dev if inplace else None)
    _check_multi(enc, [s for _st, s in exp], [st for st, _s in exp], T=T)
    work = enc.stego.clone() if inplace else None
    words, back = codec.extract(enc.stego if not inplace else work, enc.meta, enc.lm,
                                payload_words=enc.payload_words, cover=work)
    host = words.cpu().numpy()
    for i, (_st, side) in enumerate(exp):
        np.testing.assert_array_equal(framing.unpack_bits(host[i], side["L"]), pays[i][: side["L"]])
    np.testing.assert_array_equal(back.cpu().numpy(), cov)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,maxval", MULTI_AUTO_ROWS)
@pytest.mark.parametrize("h,w", FIXED_SHAPES)
def test_gpu_multipass_auto_matches_spec(h, w, dtype, maxval):
    """(c) Scheme 2's in-launch T search against spec_auto (tests/test_pee2_auto.py)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing
    from codec_tcc_amd.pee import PeeCodec
    cov, pays, exp = _multi_auto_case(h, w, dtype, maxval)
    codec = PeeCodec(len(KINDS), h, w, dtype=dtype, T="auto", tmax=MULTI_TMAX, maxval=maxval, scheme=2)
    enc = codec.embed(torch.from_numpy(cov.copy()).cuda(), list(pays))
    ts = [e[0] for e in exp]
    assert codec.t_slices.cpu().tolist() == ts
    _check_multi(enc, [e[2] for e in exp], [e[1] for e in exp], ts=ts)
    words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    host = words.cpu().numpy()
    for i, (_T, _st, side) in enumerate(exp):
        np.testing.assert_array_equal(framing.unpack_bits(host[i], side["L"]), pays[i][: side["L"]])
    np.testing.assert_array_equal(back.cpu().numpy(), cov)


@pytest.mark.gpu
def test_gpu_checksummed_call_on_adversarial_batch():
    """(d) embed(..., checksum=True) then decode(verify=True) on the 72 x 512 uint16 batch; one
    altered stego pixel of the flat_max slice (no candidate of it moves, so the restored cover
    carries the alteration) raises IntegrityError."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.checksum import IntegrityError
    from codec_tcc_amd.pee import PeeCodec
    h, w, maxval, T = 72, 512, 4095, 16
    cov = _covers(h, w, "uint16", maxval, T)
    pays = [_bits(P.capacity(c, T, maxval) // (1 + i % 2), 20 + i) for i, c in enumerate(cov)]   # every one fits
    codec = PeeCodec(len(KINDS), h, w, dtype="uint16", T=T, maxval=maxval)
    enc = codec.embed(torch.from_numpy(cov.copy()).cuda(), pays, checksum=True)
    assert enc.cover_crc is not None and enc.payload_crc is not None
    bits, back = codec.decode(enc, verify=True)
    for i in range(len(KINDS)):
        np.testing.assert_array_equal(np.asarray(bits[i]), pays[i])
    np.testing.assert_array_equal(back.cpu().numpy(), cov)
    i = KINDS.index("flat_max")
    enc.stego.view(torch.int16)[i, 40, 301] -= 1
    with pytest.raises(IntegrityError):
        codec.decode(enc, verify=True)
