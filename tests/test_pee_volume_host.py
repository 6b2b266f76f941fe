"""MED-PEE volume payloads without a GPU: the specification (tests/pee_volume_spec.py) against its
scalar restatement and the known-answer file, the rule's properties on random capacity tables,
the oracle driven by the plan, and the public interface's argument errors."""
import json
import os

import numpy as np
import pytest

import pee_volume_spec as V
from oracle import pee_cpu as P

HERE = os.path.dirname(os.path.abspath(__file__))


def _kats():
    with open(os.path.join(HERE, "golden", "pee_volume_kat.json")) as f:
        return json.load(f)


def _random_caps(rng, B, tmax, top):
    caps = np.cumsum(rng.integers(0, top, (B, tmax)), axis=1)
    caps[rng.random(B) < 0.2] = 0
    return caps


def _same_plan(a, b):
    for k in ("status", "T", "total", "capacity"):
        assert int(a[k]) == int(b[k]), k
    for k in ("n", "t", "off"):
        assert [int(v) for v in a[k]] == [int(v) for v in b[k]], k


@pytest.mark.parametrize("k", _kats(), ids=lambda k: f"B{k['B']}-t{k['tmax']}-N{k['N']}")
def test_spec_matches_known_answers(k):
    for policy in V.POLICIES:
        want = k[policy]
        got = V.plan(k["caps"], k["N"], policy)
        _same_plan(got, want)
        _same_plan(V.plan_scalar(k["caps"], k["N"], policy), want)
        pw = want["payload_words"]
        bits = V.stream_bits(k["N"], k["seed"])
        rows = V.scatter(V.pack_stream(bits), got["n"], got["off"], pw)
        if "rows" in want:
            assert [[format(int(w), "016x") for w in r] for r in rows] == want["rows"]
        sw = max(1, (got["total"] + 63) // 64)
        np.testing.assert_array_equal(V.gather(rows, got["n"], sw), V.pack_stream(bits[:got["total"]])[:sw])


def test_known_answer_file_is_the_generators():
    """The committed file is what tests/golden/make_pee_volume_golden.py writes (the capacity
    tables are regenerated from their seeds)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_pee_volume_golden",
                                                  os.path.join(HERE, "golden", "make_pee_volume_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    kats = _kats()
    assert len(kats) == len(gen.CASES)
    for k, (B, tmax, seed, top, rule) in zip(kats, gen.CASES):
        caps = gen.caps_table(B, tmax, seed, top)
        assert caps == k["caps"]
        assert k["N"] == int(rule([sum(r[t] for r in caps) for t in range(tmax)]))


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("policy", V.POLICIES)
def test_plan_properties_on_random_caps(seed, policy):
    rng = np.random.default_rng(900 + seed)
    B, tmax = int(rng.integers(1, 40)), int(rng.integers(1, 20))
    caps = _random_caps(rng, B, tmax, int(rng.choice([3, 50, 2 ** 20])))
    S = caps.sum(axis=0)
    for N in sorted({0, 1, int(S[tmax // 2]), max(0, int(S[tmax // 2]) - 1), int(S[tmax // 2]) + 1, int(S[-1]),
                     int(S[-1]) + 9}):
        if N > V.NMAX:
            continue
        p = V.plan(caps, N, policy)
        _same_plan(p, V.plan_scalar(caps.tolist(), N, policy))
        T, n = p["T"], p["n"]
        fits = np.flatnonzero(S >= N)
        assert p["status"] == (0 if fits.size else 1)
        assert T == (int(fits[0]) + 1 if fits.size else tmax)
        assert p["total"] == (N if fits.size else int(S[-1])) and p["requested"] == N
        assert int(n.sum()) == p["total"] and int(p["off"][-1]) == p["total"]
        assert ((0 <= n) & (n <= caps[:, T - 1])).all()
        for b in range(B):   # T_b minimal, and never above T*
            assert caps[b, p["t"][b] - 1] >= n[b] and p["t"][b] <= T
            assert p["t"][b] == 1 or caps[b, p["t"][b] - 2] < n[b]
        if policy == "fill":   # a prefix: full slices, one partial, then nothing
            rest = np.flatnonzero(n < caps[:, T - 1])
            if rest.size:
                assert (n[rest[0] + 1:] == 0).all()
        if N > 200000:   # the plan alone (the 64-bit products); the cut is size-independent
            continue
        # scatter then gather is the identity on the embedded prefix; row tails and pad bits zero
        bits = V.stream_bits(N, seed)
        pw = V.payload_words(N, max(1, (int(caps.max()) + 63) // 64))
        rows = V.scatter(V.pack_stream(bits), n, p["off"], pw)
        for b in range(B):
            assert not V.unpack_stream(rows[b], 64 * pw)[int(n[b]):].any()
        sw = max(1, (N + 63) // 64) + 1
        back = V.gather(rows, n, sw)
        np.testing.assert_array_equal(V.unpack_stream(back, p["total"]), bits[:p["total"]])
        assert not V.unpack_stream(back, 64 * sw)[p["total"]:].any()
        if N <= 3000:
            words = [int(w) for w in V.pack_stream(bits)]
            srows = V.scatter_scalar(words, n, p["off"], pw)
            assert srows == [[int(w) for w in r] for r in rows]
            assert V.gather_scalar(srows, n, sw) == [int(w) for w in back]


def test_row_pitch_and_record_offsets():
    assert [V.payload_words(N, 24) for N in (0, 1, 64, 65, 1536, 1537, 10 ** 6)] == [1, 1, 1, 2, 24, 24, 24]
    np.testing.assert_array_equal(V.record_offsets([5, -3, 10 ** 6, 0, 64], 2, 100), [0, 5, 5, 105, 105, 169])
    np.testing.assert_array_equal(V.record_offsets([5, 200], 2, 1000), [0, 5, 133])


@pytest.mark.parametrize("name,N", [("5x64x96", 0), ("5x64x96", 1), ("5x64x96", 63), ("5x64x96", 207),
                                    ("5x64x96", 627), ("5x64x96", 3124), ("3x33x47", 1), ("3x33x47", 300),
                                    ("4x32x64", 49), ("4x32x64", 1)])
@pytest.mark.parametrize("policy", V.POLICIES)
def test_oracle_round_trips_under_the_plan(name, N, policy):
    """pee_cpu.pee_embed per slice with the spec's n_b and T_b, then pee_extract and gather:
    the stream and the covers come back exactly; no slice overflows."""
    covers = V.ct12_batch(name)
    caps = V.curves(covers, 16, 4095)
    p = V.plan(caps, N, policy)
    bits = V.stream_bits(N, 3)
    stegos, sides = V.oracle_embed(covers, bits, p, 4095)
    assert all(sd["status"] == 0 for sd in sides)
    pw = V.payload_words(N, max(1, (covers.shape[1] // 2) * (covers.shape[2] // 2) + 63) // 64)
    rows = np.zeros((len(covers), pw), np.uint64)
    for b, (st, sd) in enumerate(zip(stegos, sides)):
        got, back = P.pee_extract(st, sd)
        np.testing.assert_array_equal(back, covers[b])
        rows[b] = V.pack_stream(got, pw)
    stream = V.gather(rows, [sd["L"] for sd in sides], max(1, (N + 63) // 64))
    np.testing.assert_array_equal(V.unpack_stream(stream, p["total"]), bits[:p["total"]])


def test_issue_examples():
    """The figures the volume rule was prototyped on (5 x 64 x 96 with slice 1 saturated)."""
    caps = V.curves(V.ct12_batch("5x64x96"), 16, 4095)
    assert int(caps[:, 15].sum()) == 3115 and not caps[1].any()
    assert list(V.plan(caps, 63, "even")["n"]) == [13, 0, 19, 16, 15]
    p = V.plan(caps, 207, "even")
    assert p["T"] == 2 and list(p["t"]) == [1, 1, 1, 2, 2]
    assert V.plan(caps, 627, "even")["T"] == 3
    p = V.plan(caps, 3124, "even")
    assert (p["status"], p["T"], p["total"]) == (1, 16, 3115)
    caps = V.curves(V.ct12_batch("4x32x64"), 16, 4095)
    p = V.plan(caps, 49, "even")
    assert p["T"] == 2 and list(p["t"]) == [1, 1, 2, 1]
    caps = V.curves(V.ct12_batch("1100x8x16"), 16, 4095)
    assert [V.plan(caps, N)["T"] for N in (1163, 1167, 5000)] == [1, 2, 5]
    assert sorted(set(V.plan(caps, 5000)["t"].tolist())) == [1, 2, 3, 4, 5]


def test_library_lists_the_volume_entries():
    from codec_tcc_amd import _lib, build
    assert set(_lib.EXPORTS_VOL) == {"codec_pee_volume_workspace_bytes", "codec_pee_volume_plan",
                                     "codec_pee_volume_scatter", "codec_pee_volume_gather",
                                     "codec_pee_volume_embed", "codec_pee_volume_extract"}
    assert not set(_lib.EXPORTS_VOL) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_EXT) | set(_lib.EXPORTS_CRC))
    assert os.path.join(build.HERE, "csrc", "codec_vol.hip") in build.SRCS
    assert os.path.join(build.INC, "codec_tcc_vol.h") in build._common_deps()
    assert {38: "k_vol_plan", 39: "k_vol_scatter", 40: "k_vol_gather"}.items() <= _lib.KERNEL_TAGS.items()
    hdr = open(os.path.join(build.INC, "codec_tcc_vol.h")).read()
    for tag, name in ((38, "PLAN"), (39, "SCATTER"), (40, "GATHER")):
        assert f"#define CODEC_K_VOL_{name} {tag}" in hdr
    import ctypes
    assert ctypes.sizeof(_lib.PeeVolumeInfo) == 32


def test_argument_errors_need_no_gpu():
    import codec_tcc_amd
    from codec_tcc_amd import pee
    covers = np.zeros((3, 16, 16), np.uint16)
    with pytest.raises(ValueError, match="policy"):
        codec_tcc_amd.encode_volume(covers, b"abc", policy="proportional")
    with pytest.raises(ValueError, match="scheme"):
        pee.encode_volume(covers, b"abc", scheme=2)
    with pytest.raises(ValueError, match="stack"):
        pee.encode_volume(np.zeros((2, 3, 16, 16), np.uint16), b"abc")
    with pytest.raises(ValueError, match="stack"):
        pee.encode_volume(np.zeros((0, 16, 16), np.uint16), b"abc")
    with pytest.raises(ValueError, match="0/1"):
        pee.encode_volume(covers, np.array([0, 1, 2]))
    pee.check_volume_args((256, 2048, 2048), 2 ** 31 - 1)
    pee.check_volume_args((2047, 2048, 2048), 0, "fill")
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        pee.check_volume_args((2048, 2048, 2048), 8)            # 2^31 candidates
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        pee.check_volume_args((4, 64, 64), 2 ** 31)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        pee.check_volume_args((4, 64, 64), -1)
    with pytest.raises(ValueError, match="scheme"):
        pee.check_volume_args((4, 64, 64), 8, "even", 2)
    with pytest.raises(ValueError, match="stack"):
        pee.check_volume_args((64, 64), 8)
    with pytest.raises(ValueError):
        V.plan([[1, 2]], 3, "spread")
    with pytest.raises(ValueError):
        V.plan([[1, 2]], 2 ** 31)
