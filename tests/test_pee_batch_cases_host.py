"""The conditions tests/test_pee_batch_dispatch.py relies on, checked on the specifications alone (no
GPU, never the library): for every family and every batch size at 256 CUs, no two slices of a
batch can be mistaken for one another, and each batch holds the payloads at which a kernel's
per-slice bookkeeping differs -- an empty one, one whose `end` lies in the slice's second chunk,
one that overflows (blind: is refused)."""
import numpy as np
import pytest

import pee_batch_cases as BC
import pee_gate_spec as G

NCU = 256
SIZES = BC.batches(NCU)
CASES = [(fam, name) for fam, (names, _rows) in BC.FAMILIES.items() for name in names]


def test_batch_sizes():
    assert SIZES == {"below": 255, "fills": 256, "ragged": 265, "two_rounds": 436}
    assert [BC.fills_chip(SIZES[k], NCU) for k in ("below", "fills", "ragged", "two_rounds")] == [False, True, False, True]
    B = SIZES["ragged"]
    assert B % 8 == 1 and B % 32 != 0 and -(-B // 8) == 34           # the last lane holds one slice, the last group is partial
    assert all(np.gcd(p, q) == 1 for p in (5, 7) for q in (8, 32)) and np.gcd(5, 7) == 1
    assert BC.index0(B) + B == 2 ** 31


def test_slice_geometry():
    items = (BC.H // 2) * (BC.W // 8)
    assert BC.W % 8 == 0 and BC.H % 2 == 1 and items == 1089 and -(-items // 1024) == 2
    assert BC.SECOND_CHUNK == 31 * (BC.W // 2) + 4 < BC.NC == 4356     # item 1024 = row pair 31, its second item
    h, w = BC.GRID_SHAPE
    nch = -(-((h // 2) * (w // 8)) // 1024)
    B8 = -(-SIZES["ragged"] // 8)
    assert nch == 9 and 8 * B8 * nch > 2048                            # pee_total_slots in place: past the 2048 workgroups


def check_rows(fam, rows):
    """the conditions on one batch; AssertionError names the one that is broken"""
    seen = {}
    for b, r in enumerate(rows):
        other = seen.setdefault(BC.digest(r), b)
        assert other == b, f"{fam}: slices {other} and {b} cannot be told apart"
    ok = [r for r in rows if r["status"] == 0]
    assert any(r["n"] > 0 and r["end"] >= BC.SECOND_CHUNK for r in ok), f"{fam}: no `end` in the second chunk"
    assert any(r["n"] == 0 for r in ok), f"{fam}: no empty payload"
    assert any(r["status"] != 0 for r in rows), f"{fam}: no overflow / refusal"
    assert any(r["n"] > 0 and 0 <= r["end"] < BC.SECOND_CHUNK for r in ok), f"{fam}: no `end` in the first chunk"


@pytest.mark.parametrize("fam,name", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_batches_meet_their_conditions(fam, name):
    B = SIZES[name]
    rows = BC.FAMILIES[fam][1](B)
    assert len(rows) == B
    check_rows(fam, rows)
    if fam in BC.BLIND_FAMILIES:
        E = [r["info"][2] for r in rows if r["status"] == 0]
        assert 0 in E and max(E) >= 3, (fam, sorted(set(E)))
    if fam in ("blind-auto", "blind-keyed-auto", "auto-uint16", "auto-uint8", "scheme2-auto", "gate-auto"):
        idx = {"auto-uint16": 2, "auto-uint8": 2, "scheme2-auto": 2, "gate-auto": 2}
        make = {"auto-uint16": lambda b: BC.auto("uint16", b), "auto-uint8": lambda b: BC.auto("uint8", b),
                "scheme2-auto": lambda b: BC.scheme2_auto("uint16", b), "gate-auto": BC.gate_auto,
                "blind-auto": BC.blind_auto, "blind-keyed-auto": lambda b: BC.blind_keyed(b, B, True, BC.NONCE_2)}[fam]
        ts = {make(b)[idx.get(fam, 4)] for b in range(B)}
        assert len(ts - {0}) >= 3, (fam, sorted(ts))


def test_a_slice_mix_up_is_noticed():
    """the uniqueness condition fails when two slices are equal"""
    rows = BC.FAMILIES["fixed-uint16"][1](40)
    rows[33] = rows[1]
    with pytest.raises(AssertionError, match="slices 1 and 33"):
        check_rows("fixed-uint16", rows)


def test_gated_covers_are_half_active():
    """as tests/test_pee_gate.py requires of its ct12 covers at G = 24"""
    for b in range(SIZES["ragged"]):
        assert 0.2 <= G.active_fraction(BC.cover("uint16", b), 24) <= 0.8, b
    for q in range(9):
        assert 0.2 <= G.active_fraction(BC.grid_pair(q)[0], 24) <= 0.8, q


def test_per_slice_parameters_meet_every_length():
    """T, G and the rectangle change with period 5, the length with period 7: within 35 slices every
    pair occurs, and the ROI family's rectangles (shifted every five slices) meet every (T, G)"""
    assert {(b % 5, b % 7) for b in range(35)} == {(i, j) for i in range(5) for j in range(7)}
    B = SIZES["fills"]
    kinds = {(b % 5, BC.rect(b // 5 + b)) for b in range(B)}
    assert len(kinds) == 25
    rects = {BC.roi(b)[4] for b in range(B)}
    assert (0, 0, BC.H, BC.W) in rects and (0, 0, 0, 0) in rects and (20, 30, 20, 90) in rects
    full = [b for b in range(B) if BC.roi(b)[4] == (0, 0, BC.H, BC.W)]
    assert all(np.array_equal(BC.roi(b)[5], BC.roi(b)[0]) for b in full)      # a protected slice is never modified


@pytest.mark.parametrize("name", ["fills", "ragged"])
def test_volume_plans(name):
    """the saturated slice gets nothing under either policy, "fill" leaves the stack's tail empty, the
    slices' own T differ, and the stegos are pairwise different"""
    B = SIZES[name]
    for policy in ("even", "fill"):
        cov, bits, p, stegos, sides = BC.volume_plan(B, policy)
        assert p["status"] == 0 and p["T"] == 3 and p["total"] == len(bits) > 0
        assert p["n"][BC.SATURATED] == 0 and len(set(p["t"].tolist())) >= 2
        if policy == "fill":   # a filled slice's `end` is its last expandable candidate: in the second chunk
            assert any(sd["end"] >= BC.SECOND_CHUNK for sd in sides)
            first = int(np.flatnonzero(p["n"] == 0)[1])      # (the saturated slice is the first)
            assert first < B - 8 and not p["n"][first:].any()
        assert len({s.tobytes() for s in stegos}) == B
    cov, bits, p, stegos, sides = BC.gvol_plan(B, "even")
    assert p["status"] == 0 and p["n"][BC.SATURATED] == 0 and len(set(p["g"].tolist())) >= 2
    assert len({s.tobytes() for s in stegos}) == B
