"""The MED-PEE exchange records against an independent statement of the record rule.

codec_pee_pack_records / codec_pee_unpack_records (codec_tcc_amd/csrc/codec_records.hip), their
host restatement (codec_tcc_amd/distributed.py: pack_pee_records / unpack_pee_records on CPU
tensors, map_prefix, record_width_needed, dense_words_needed) and the bit-by-bit statement
tests/pee_record_spec.py are compared word for word over one seeded case matrix, shared by the
CPU and the GPU tests.  Every comparison is exact.

The matrix: lm_words in {1, 4, 255, 256, 257, 600} (the pack kernel scans the map in rounds of
256 words: one round, exactly one, one word into the second, three rounds); per lm_words one
batch with one slice per row of ROWS below.  Map words are random over the whole row, so
garbage lies past every `end`; the meta fields other than end / lm_count hold distinct non-zero
values.  Widths and lm_cols: _widths / _cols.
"""
import ctypes
import functools
import importlib.util
import json
import os
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import pee_record_spec as S
from codec_tcc_amd import _lib
from codec_tcc_amd import distributed as D

HERE = os.path.dirname(os.path.abspath(__file__))
LM_WORDS = (1, 4, 255, 256, 257, 600)
INT_MAX = 2 ** 31 - 1
M64 = (1 << 64) - 1
POISON = 0x5A5A5A5A5A5A5A5A
GUARD = 64   # poisoned words kept behind every output buffer: nothing may be written there

# (name, end, lm_count, bit density); nc = 64 * lm_words, "true" = popcount of the masked prefix
ROWS = (
    ("end-1", lambda nc: -1, "true", 0.5),
    ("end-1_count3", lambda nc: -1, 3, 0.5),                 # recount with a scan loop that never runs
    ("end0_ones", lambda nc: 0, "true", 1.0),
    ("end62", lambda nc: 62, "true", 0.5),
    ("end63", lambda nc: 63, "true", 0.5),
    ("end64", lambda nc: 64 % nc, "true", 0.5),
    ("last_thin", lambda nc: nc - 1, "true", 0.01),
    ("last_ones", lambda nc: nc - 1, "true", 1.0),           # every word all 64 bits
    ("last_half", lambda nc: nc - 1, "true", 0.5),
    ("past_map", lambda nc: nc + 44, "true", 0.5),
    ("end-70", lambda nc: -70, "true", 0.5),
    ("count-1", lambda nc: nc // 2, -1, 0.5),
    ("count1e6", lambda nc: nc // 2, 10 ** 6, 0.001),
    ("understated7", lambda nc: nc - 1, 7, 0.001),           # topped up to nine set bits, see _batch
    # beyond the issue's table: an `end` past the map in the sparse form, the largest `end`, a
    # recount after a scan of every round, a full word in the sparse form, and ten / eleven set
    # bits (lm_count == 2 * 5 and 2 * 5 + 1)
    ("past_map_thin", lambda nc: nc + 44, "true", 0.01),
    ("end_intmax_thin", lambda nc: INT_MAX, "true", 0.01),
    ("overstated3", lambda nc: nc - 1, "true+3", 0.01),
    ("full_word_thin", lambda nc: nc - 1, "true", 0.01),
    ("ten", lambda nc: nc - 6, "true", 0.0),
    ("eleven", lambda nc: nc - 6, "true", 0.0),
)
# rows whose lm_count-th set bit is placed in a given word (an understated count that the scan
# reaches part-way): the last word of round one, the first of round two, the middle of round two
PLACED = (("placed_w255", lambda lw: 255 if lw >= 256 else None, 1),
          ("placed_w256", lambda lw: 256 if lw >= 257 else None, 1),
          ("placed_mid2", lambda lw: 256 + (lw - 256) // 2 if lw >= 257 else None, 2))

Batch = namedtuple("Batch", "lm_words names metas rows bits exact first widths cols need")


def _row_words(bits):
    return [int(w) for w in np.packbits(bits, bitorder="little").view("<u8")]


@functools.lru_cache(maxsize=None)
def _batch(lm_words):
    """The batch of one lm_words: names, metas (16 int32 fields each), map rows (uint64 words),
    the rows' bits, `exact` (the count is not understated: unpack(pack) must return the whole
    prefix), `first` (for an understated row: how many set bits travel), widths, lm_cols."""
    nc = 64 * lm_words
    rng = np.random.default_rng(1000 + lm_words)
    names, ends, counts, maps, first = [], [], [], [], []

    def true_count(bits, end):
        return int(bits[: max(0, min(end + 1, nc))].sum())

    for name, end_of, cnt, density in ROWS:
        end = end_of(nc)
        bits = np.ones(nc, np.uint8) if density >= 1.0 else (rng.random(nc) < density).astype(np.uint8)
        if name == "understated7":       # 0.001 leaves fewer than 7 bits in a small map: top up to >= 9
            bits[:: max(1, nc // 9)][:9] = 1
        if name in ("past_map_thin", "end_intmax_thin"):
            bits[nc - 4:] = 1            # bits of the last word above bit (nc + 44) % 64 = 44
        if name == "full_word_thin":
            w = min(1, lm_words - 1)
            bits[64 * w: 64 * w + 64] = 1
        if name in ("ten", "eleven"):    # exactly 10 / 11 set bits in [0, end], garbage past it
            k = 10 if name == "ten" else 11
            bits[:] = 0
            bits[rng.choice(end + 1, k, replace=False)] = 1
            bits[end + 1:] = 1
        if max(end, -1) + 1 < nc:
            bits[max(end, -1) + 1] = 1   # the first bit past `end` is always garbage
        t = true_count(bits, end)
        f = None
        if cnt == "true":
            cnt = t
        elif cnt == "true+3":
            cnt = t + 3
        elif 0 <= cnt < t:
            f = cnt
        names.append(name), ends.append(end), counts.append(cnt), maps.append(bits), first.append(f)
    for name, word_of, nth in PLACED:
        w = word_of(lm_words)
        if w is None:
            continue
        bits = (rng.random(nc) < 0.01).astype(np.uint8)
        bits[64 * w: 64 * w + 64] = 0
        bits[[64 * w + 3, 64 * w + 40, 64 * w + 63]] = 1
        cnt = int(bits[: 64 * w].sum()) + nth
        assert np.flatnonzero(bits)[cnt - 1] // 64 == w and cnt < int(bits.sum())
        names.append(name), ends.append(nc - 1), counts.append(cnt), maps.append(bits), first.append(cnt)
    metas = []
    for b, (end, cnt) in enumerate(zip(ends, counts)):
        m = [(0x01010101 * (f + 1) + 0x100 * b) & 0x7FFFFFFF for f in range(S.FIELDS)]
        m[S.FLAGS] &= ~S.RECOUNTED
        m[S.END], m[S.LM_COUNT] = end, cnt
        metas.append(m)
    rows = [_row_words(bits) for bits in maps]
    need = S.width_needed(metas, lm_words)
    widths = {1, max(1, need - 1), need, need + 3, lm_words + 5}
    # lm_count exactly 2 * width and 2 * width + 1 for one slice each (ten / eleven at 5; the full
    # word's count c at c // 2)
    for name in ("ten", "eleven", "full_word_thin"):
        widths.add(max(1, counts[names.index(name)] // 2))
    cols = {1, min(S.dense_words_needed(metas), lm_words), lm_words, lm_words + 3}
    exact = [f is None for f in first]
    return Batch(lm_words, names, metas, rows, maps, exact, first, sorted(widths), sorted(cols), need)


@functools.lru_cache(maxsize=None)
def _spec_packed(lm_words, width):
    """spec.pack of the whole batch: uint64 [B, HDR + width]."""
    bt = _batch(lm_words)
    return np.array([S.pack(m, r, width) for m, r in zip(bt.metas, bt.rows)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _spec_unpacked(lm_words, width, cols):
    """spec.unpack of spec.pack's records: (int32 [B, 16] metas, uint64 [B, cols] maps)."""
    rec = _spec_packed(lm_words, width)
    out = [S.unpack([int(w) for w in r], width, cols) for r in rec]
    return np.array([m for m, _ in out], dtype=np.int32), np.array([lm for _, lm in out], dtype=np.uint64)


def _meta_t(metas, dev="cpu"):
    a = np.array(metas, dtype=np.int32).reshape(len(metas), S.FIELDS)
    return torch.from_numpy(a.view(np.uint8).reshape(len(metas), _lib.PEE_META_BYTES).copy()).to(dev)


def _words_t(words, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).view(np.int64).copy()).to(dev)


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _same(got, want, what, names=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, want {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, w = (int(x) for x in bad[0])
        name = f" ({names[b]})" if names else ""
        pytest.fail(f"{what}: {len(bad)} words differ, first at slice {b}{name}, word {w}: "
                    f"got {int(got[b, w]) & M64:#018x}, want {int(want[b, w]) & M64:#018x}")


def _kats():
    with open(os.path.join(HERE, "golden", "pee_records_kat.json")) as f:
        return json.load(f)


def _kat_rows(k):
    return [int(w, 16) for w in k["lm"]]


# ------------------------------------------------------------------ CPU: the matrix and the spec
@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_matrix_holds_the_cases_it_names(lm_words):
    """The properties the matrix is there for, read off the generated batch itself."""
    bt = _batch(lm_words)
    nc = 64 * lm_words
    at = {n: i for i, n in enumerate(bt.names)}
    end = [m[S.END] for m in bt.metas]
    cnt = [m[S.LM_COUNT] for m in bt.metas]
    assert [end[at[n]] for n in ("end-1", "end0_ones", "end62", "end63", "end64", "last_half", "past_map", "end-70")] == \
        [-1, 0, 62, 63, 64 % nc, nc - 1, nc + 44, -70]
    assert cnt[at["end-1"]] == 0 and cnt[at["end-1_count3"]] == 3 and cnt[at["end-70"]] == 0
    assert cnt[at["last_ones"]] == nc and cnt[at["count-1"]] == -1 and cnt[at["count1e6"]] == 10 ** 6
    for n, e, bits in zip(bt.names, end, bt.bits):         # garbage right behind every `end` inside the map
        assert e >= nc - 1 or bits[max(e, -1) + 1] == 1, n
    for m in bt.metas:                                     # distinct non-zero header fields
        other = [v for f, v in enumerate(m) if f not in (S.END, S.LM_COUNT)]
        assert len(set(other)) == len(other) and all(other) and not m[S.FLAGS] & S.RECOUNTED
    u = at["understated7"]
    assert int(bt.bits[u].sum()) >= 9 and bt.first[u] == 7 and not bt.exact[u]
    assert cnt[at["overstated3"]] == int(bt.bits[at["overstated3"]].sum()) + 3
    assert cnt[at["ten"]] == 10 and cnt[at["eleven"]] == 11 and 5 in bt.widths
    assert cnt[at["full_word_thin"]] // 2 in bt.widths and bt.rows[at["full_word_thin"]][min(1, lm_words - 1)] == M64
    assert any(c == 2 * w for c in cnt for w in bt.widths) and any(c == 2 * w + 1 for c in cnt for w in bt.widths)
    assert bt.need == lm_words and {1, max(1, bt.need - 1), bt.need, bt.need + 3, lm_words + 5} <= set(bt.widths)
    assert {1, lm_words, lm_words + 3} <= set(bt.cols)
    placed = [n for n in bt.names if n.startswith("placed")]
    assert placed == [n for n, word_of, _ in PLACED if word_of(lm_words) is not None]
    assert len(placed) == (0 if lm_words < 256 else 1 if lm_words == 256 else 3)
    # both forms occur at every lm_words, and the recount in the sparse one
    forms = {S.is_sparse(c, w) for c in cnt for w in bt.widths}
    assert forms == {True, False}
    assert any(S.is_sparse(cnt[at[n]], max(bt.widths)) for n in ("end-1_count3", "overstated3"))


def test_recounted_flag_is_the_headers():
    src = open(os.path.join(os.path.dirname(HERE), "include", "codec_tcc.h")).read()
    assert int(re.search(r"#define CODEC_PEE_RECORD_RECOUNTED (\d+)", src).group(1)) == S.RECOUNTED == D.RECORD_RECOUNTED
    assert int(re.search(r"#define CODEC_PEE_RECORD_HDR_WORDS (\d+)", src).group(1)) == S.HDR_WORDS == D.PEE_META_WORDS
    assert (S.END, S.LM_COUNT, S.FLAGS) == (D.PEE_END_FIELD, D.PEE_LMCOUNT_FIELD, D.PEE_FLAGS_FIELD)


def test_spec_equals_the_committed_vectors():
    """tests/golden/pee_records_kat.json is what the spec computes today (and what its generator
    writes), so the spec cannot drift silently; the cases the file is there for are in it."""
    kats = _kats()
    spec = importlib.util.spec_from_file_location("make_pee_records_golden",
                                                  os.path.join(HERE, "golden", "make_pee_records_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.build() == kats
    assert 10 <= len(kats) <= 24 and all(k["lm_words"] <= 4 for k in kats)
    for k in kats:
        rec = S.pack(k["meta"], _kat_rows(k), k["width"])
        assert ["%016x" % w for w in rec] == k["record"], k["name"]
        assert len(k["unpack"]) == 2
        for u in k["unpack"]:
            meta, lm = S.unpack(rec, k["width"], u["lm_cols"])
            assert ["%016x" % w for w in lm] == u["lm"], (k["name"], u["lm_cols"])
            assert meta == S.header_fields(rec)
    by = {k["name"]: k for k in kats}
    assert {k["form"] for k in kats} == {"sparse", "dense"}
    assert {by[n]["meta"][S.END] for n in ("recount_end_minus_1", "end_63_dense", "end_64_dense")} == {-1, 63, 64}
    for n in ("recount", "recount_end_minus_1"):
        assert S.header_fields([int(w, 16) for w in by[n]["record"]])[S.FLAGS] & S.RECOUNTED
    for n in ("end_past_map_dense", "end_past_map_sparse"):
        assert by[n]["meta"][S.END] >= 64 * by[n]["lm_words"]
    assert by["boundary_2w"]["meta"][S.LM_COUNT] == 2 * by["boundary_2w"]["width"] and by["boundary_2w"]["form"] == "sparse"
    b1 = by["boundary_2w_plus_1"]
    assert b1["meta"][S.LM_COUNT] == 2 * b1["width"] + 1 and b1["form"] == "dense"
    # an `end` past the map keeps the last word whole, in both forms
    assert by["end_past_map_dense"]["record"][-1] == "f" * 16
    assert by["end_past_map_sparse"]["record"][-1] == "%016x" % (254 | 255 << 32)


def test_host_rule_equals_the_committed_vectors():
    for k in _kats():
        meta, lm = _meta_t([k["meta"]]), _words_t([_kat_rows(k)])
        rec = D.pack_pee_records(meta, lm, k["width"])
        _same(_u64(rec), np.array([[int(w, 16) for w in k["record"]]], dtype=np.uint64), f"pack {k['name']}")
        for u in k["unpack"]:
            _m, got = D.unpack_pee_records(rec, u["lm_cols"])
            _same(_u64(got), np.array([[int(w, 16) for w in u["lm"]]], dtype=np.uint64), f"unpack {k['name']} cols {u['lm_cols']}")


@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_spec_round_trip(lm_words):
    """For width >= the needed one and lm_cols <= lm_words, unpack(pack(.)) is the map prefix of
    every slice whose count is not understated; an understated slice keeps exactly its first
    lm_count set bits and loses every later one."""
    bt = _batch(lm_words)
    for width in (w for w in bt.widths if w >= bt.need):
        for cols in (c for c in bt.cols if c <= lm_words):
            metas, maps = _spec_unpacked(lm_words, width, cols)
            for b, name in enumerate(bt.names):
                pref = S.map_prefix(bt.metas[b][S.END], bt.rows[b], cols)
                got = [int(w) for w in maps[b]]
                if bt.exact[b]:
                    assert got == pref, (name, width, cols)
                    continue
                if not S.is_sparse(bt.first[b], width):    # lm_words 1, width 1: 7 > 2, the dense prefix
                    assert got == [p if w < width else 0 for w, p in enumerate(pref)], (name, width, cols)
                    continue
                kept = S.set_bits(bt.rows[b], bt.metas[b][S.END])[: bt.first[b]]
                assert len(kept) == bt.first[b]
                assert got == S._words(kept, cols), (name, width, cols)
                if cols == lm_words:
                    assert got != pref and all(g & ~p == 0 for g, p in zip(got, pref))
                assert [int(x) for x in metas[b]] == bt.metas[b]       # no recount: the bits were there


def test_understated_row_loses_exactly_the_bits_after_its_seventh():
    for lm_words in LM_WORDS:
        bt = _batch(lm_words)
        b = bt.names.index("understated7")
        allbits = S.set_bits(bt.rows[b], bt.metas[b][S.END])
        width = max(4, bt.need)
        _meta, lm = S.unpack(S.pack(bt.metas[b], bt.rows[b], width), width, lm_words)
        assert len(allbits) >= 9 and S.set_bits(lm, 64 * lm_words) == allbits[:7]


# ------------------------------------------------------------------ the implementations against the spec
def _check_pack(bt, dev):
    """pack_pee_records at every width of the batch, into one flat buffer as PeeRecordExchange
    keeps it: poisoned, packed at `width`, then packed again at the next width's layout without
    re-poisoning (the buffer is reused step to step).  The words behind the records stay
    untouched."""
    meta, lm = _meta_t(bt.metas, dev), _words_t(bt.rows, dev)
    B = len(bt.metas)
    wmax = max(bt.widths)
    flat = torch.empty(B * (S.HDR_WORDS + wmax) + GUARD, dtype=torch.int64, device=dev)
    poison = torch.tensor(POISON, dtype=torch.int64)
    for i, width in enumerate(bt.widths):
        flat.fill_(POISON)
        for w in (width, bt.widths[(i + 1) % len(bt.widths)]):
            n = B * (S.HDR_WORDS + w)
            out = D.pack_pee_records(meta, lm, w, out=flat[:n].view(B, S.HDR_WORDS + w))
            assert out.data_ptr() == flat.data_ptr()
            _same(_u64(out), _spec_packed(bt.lm_words, w), f"pack lm_words {bt.lm_words} width {w}", bt.names)
            assert bool((flat[B * (S.HDR_WORDS + wmax):].cpu() == poison).all()), "a write behind the records"
    # without out=: a fresh buffer
    _same(_u64(D.pack_pee_records(meta, lm, bt.need)), _spec_packed(bt.lm_words, bt.need), "pack (no out=)", bt.names)


def _check_unpack(bt, dev):
    """unpack_pee_records of the spec's records at every width and lm_cols, into a poisoned out=."""
    B = len(bt.metas)
    for width in bt.widths:
        rec = _words_t(_spec_packed(bt.lm_words, width), dev)
        for cols in bt.cols:
            want_meta, want_lm = _spec_unpacked(bt.lm_words, width, cols)
            flat = torch.full((B * cols + GUARD,), POISON, dtype=torch.int64, device=dev)
            meta, lm = D.unpack_pee_records(rec, cols, out=flat[: B * cols].view(B, cols))
            assert lm.data_ptr() == flat.data_ptr()
            _same(_u64(lm), want_lm, f"unpack lm_words {bt.lm_words} width {width} lm_cols {cols}", bt.names)
            _same(meta.cpu().numpy().view(np.int32), want_meta, f"unpack meta width {width}", bt.names)
            assert bool((flat[B * cols:].cpu() == torch.tensor(POISON, dtype=torch.int64)).all()), "a write behind the maps"


def _check_helpers(bt, dev):
    """map_prefix, record_width_needed and dense_words_needed: the batch and every slice alone
    (among them end + 1 a multiple of 64, where map_prefix's shift is by 64, and negative ends
    and counts)."""
    meta, lm = _meta_t(bt.metas, dev), _words_t(bt.rows, dev)
    for cols in sorted({c for c in bt.cols if c <= bt.lm_words} | {max(1, bt.lm_words - 1)}):
        want = np.array([S.map_prefix(m[S.END], r, cols) for m, r in zip(bt.metas, bt.rows)], dtype=np.uint64)
        _same(_u64(D.map_prefix(meta, lm, cols)), want, f"map_prefix lm_words {bt.lm_words} cols {cols}", bt.names)
    assert any((m[S.END] + 1) % 64 == 0 and m[S.END] >= 0 for m in bt.metas)
    for cap in (None, 1, bt.lm_words, bt.lm_words + 7):
        assert int(D.record_width_needed(meta, cap)) == S.width_needed(bt.metas, cap), cap
    assert int(D.dense_words_needed(meta)) == S.dense_words_needed(bt.metas)
    for b, m in enumerate(bt.metas):
        one = meta[b: b + 1]
        assert int(D.record_width_needed(one)) == S.width_needed([m]), bt.names[b]
        assert int(D.record_width_needed(one, bt.lm_words)) == S.width_needed([m], bt.lm_words), bt.names[b]
        assert int(D.dense_words_needed(one)) == S.dense_words_needed([m]), bt.names[b]
    assert int(D.record_width_needed(meta[:0])) == S.width_needed([]) == 1
    assert int(D.dense_words_needed(meta[:0])) == S.dense_words_needed([]) == 1


@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_host_pack_equals_spec(lm_words):
    _check_pack(_batch(lm_words), "cpu")


@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_host_unpack_equals_spec(lm_words):
    _check_unpack(_batch(lm_words), "cpu")


@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_host_helpers_equal_spec(lm_words):
    _check_helpers(_batch(lm_words), "cpu")


# ------------------------------------------------------------------ GPU: the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_gpu_pack_equals_spec(lm_words):
    """k_pee_pack_records word for word: both forms and every slot of them over a poisoned,
    reused buffer; the scan's carry across rounds of 256 words (lm_words 257 and 600: the
    placed_* rows end their count in word 255, 256 and mid round two, last_thin / overstated3
    run every round), the end mask (end62 .. end64, garbage past every end), an `end` past the
    map, the 2 * width boundary from both sides (ten / eleven at width 5), the recount."""
    _check_pack(_batch(lm_words), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_gpu_unpack_equals_spec(lm_words):
    """k_pee_unpack_records on the spec's records: lm_cols below, at and above the width and
    above 256 (the strided loop), width above lm_words."""
    _check_unpack(_batch(lm_words), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("lm_words", LM_WORDS)
def test_gpu_helpers_equal_spec(lm_words):
    _check_helpers(_batch(lm_words), "cuda")


@pytest.mark.gpu
def test_gpu_kernels_equal_the_committed_vectors():
    for k in _kats():
        meta, lm = _meta_t([k["meta"]], "cuda"), _words_t([_kat_rows(k)], "cuda")
        rec = D.pack_pee_records(meta, lm, k["width"])
        _same(_u64(rec), np.array([[int(w, 16) for w in k["record"]]], dtype=np.uint64), f"pack {k['name']}")
        for u in k["unpack"]:
            _m, got = D.unpack_pee_records(rec, u["lm_cols"])
            _same(_u64(got), np.array([[int(w, 16) for w in u["lm"]]], dtype=np.uint64), f"unpack {k['name']} cols {u['lm_cols']}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("lm_words", (4, 257))
def test_gpu_unpack_direct_with_meta_out(lm_words):
    """codec_pee_unpack_records through ctypes: meta_out alone (lm_out = NULL) and both outputs,
    each into poisoned buffers with a guard behind them."""
    lib = _lib.load()
    bt = _batch(lm_words)
    B, width, cols = len(bt.metas), bt.need, lm_words
    rec = _words_t(_spec_packed(lm_words, width), "cuda")
    want_meta, want_lm = _spec_unpacked(lm_words, width, cols)
    poison = torch.tensor(POISON, dtype=torch.int64)
    for with_lm in (False, True):
        mflat = torch.full((B * S.HDR_WORDS + GUARD,), POISON, dtype=torch.int64, device="cuda")
        lflat = torch.full((B * cols + GUARD,), POISON, dtype=torch.int64, device="cuda")
        _lib.check(lib.codec_pee_unpack_records(B, width, rec.data_ptr(), cols, mflat.data_ptr(),
                                                lflat.data_ptr() if with_lm else None, _stream()), "codec_pee_unpack_records")
        torch.cuda.synchronize()
        got_meta = mflat[: B * S.HDR_WORDS].cpu().numpy().view(np.int32).reshape(B, S.FIELDS)
        _same(got_meta, want_meta, f"meta_out (lm_out {'given' if with_lm else 'NULL'})", bt.names)
        assert bool((mflat[B * S.HDR_WORDS:].cpu() == poison).all())
        if with_lm:
            _same(_u64(lflat[: B * cols].view(B, cols)), want_lm, "lm_out beside meta_out", bt.names)
            assert bool((lflat[B * cols:].cpu() == poison).all())
        else:
            assert bool((lflat.cpu() == poison).all())


@pytest.mark.gpu
def test_gpu_zero_rows_touch_nothing():
    """B = 0 / n = 0 return 0 and write nothing."""
    lib = _lib.load()
    bt = _batch(4)
    meta, lm = _meta_t(bt.metas, "cuda"), _words_t(bt.rows, "cuda")
    rec = _words_t(_spec_packed(4, 4), "cuda")
    out = torch.full((len(bt.metas) * (S.HDR_WORDS + 4),), POISON, dtype=torch.int64, device="cuda")
    mout = torch.full_like(out, POISON)
    assert lib.codec_pee_pack_records(0, 4, meta.data_ptr(), lm.data_ptr(), 4, out.data_ptr(), _stream()) == 0
    assert lib.codec_pee_unpack_records(0, 4, rec.data_ptr(), 4, mout.data_ptr(), out.data_ptr(), _stream()) == 0
    assert lib.codec_pee_pack_records(0, 4, None, None, 4, None, _stream()) == 0
    assert lib.codec_pee_unpack_records(0, 4, None, 4, None, None, _stream()) == 0
    torch.cuda.synchronize()
    poison = torch.tensor(POISON, dtype=torch.int64)
    assert bool((out.cpu() == poison).all()) and bool((mout.cpu() == poison).all())
    # the Python wrappers with an empty batch
    e = D.pack_pee_records(meta[:0], lm[:0], 4)
    assert tuple(e.shape) == (0, S.HDR_WORDS + 4)
    m0, l0 = D.unpack_pee_records(e, 4)
    assert tuple(m0.shape) == (0, _lib.PEE_META_BYTES) and tuple(l0.shape) == (0, 4)


@pytest.mark.gpu
def test_gpu_strided_views_pack_like_their_copies():
    bt = _batch(257)
    meta, lm = _meta_t(bt.metas, "cuda"), _words_t(bt.rows, "cuda")
    mv, lv = meta[::2], lm[::2]
    assert not lv.is_contiguous() and not mv.is_contiguous()
    for width in (5, bt.need):
        got = D.pack_pee_records(mv, lv, width)
        _same(_u64(got), _spec_packed(257, width)[::2], f"strided pack width {width}", bt.names[::2])
        _same(_u64(got), _u64(D.pack_pee_records(mv.contiguous(), lv.contiguous(), width)), "strided against its copy")
        rv = D.pack_pee_records(meta, lm, width)[::2]
        _m, l1 = D.unpack_pee_records(rv, 257)
        _same(_u64(l1), _spec_unpacked(257, width, 257)[1][::2], f"strided unpack width {width}", bt.names[::2])


# ------------------------------------------------------------------ GPU: real embed outputs across the round boundary
REAL = dict(H=520, W=504, T=2, cover_maxval=4095, maxval=4096, nbits=20000, kinds=(("top_band", 0), ("ends", 11)))


@functools.lru_cache(maxsize=None)
def _real_covers():
    import pee_covers as C
    r = REAL
    return np.stack([C.cover(kind, r["H"], r["W"], "uint16", r["cover_maxval"], r["T"], seed) for kind, seed in r["kinds"]])


def _real_bits(b):
    return np.random.default_rng(70 + b).integers(0, 2, REAL["nbits"]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _real_oracle():
    """oracle/pee_cpu.py on the real covers: per slice (end, indices of the map's set bits)."""
    from oracle import pee_cpu as P
    r = REAL
    sides = [P.pee_embed(c, _real_bits(b), r["T"], maxval=r["maxval"], truncate=True)[1] for b, c in enumerate(_real_covers())]
    return [(s["end"], np.flatnonzero(s["lm"])) for s in sides]


def _assert_real_covers_span_the_rounds():
    nc = (REAL["H"] // 2) * (REAL["W"] // 2)
    assert (nc + 63) // 64 == 1024
    (end0, idx0), (end1, idx1) = _real_oracle()
    assert max(idx0.size, idx1.size) > 512
    assert end0 == nc - 1 and 128 < idx0.size <= 2 * 1024 and len(set((idx0 // (64 * 256)).tolist())) >= 3
    assert idx1.size > 512 and set((idx1 // (64 * 256)).tolist()) == {0, 1, 2, 3}
    need = max(min((i.size + 1) // 2, (e + 64) // 64) for e, i in ((end0, idx0), (end1, idx1)))
    assert idx0.size <= 2 * need < idx1.size        # at the needed width: slice 0 sparse, slice 1 dense


def test_real_covers_span_the_scan_rounds():
    """The oracle on the covers of the GPU test below: range-end covers built for maxval 4095 and
    embedded at maxval 4096, so that the crest's rim (top_band) and a third of the candidates
    (ends) are overflow-prone.  Slice 0 truncates (end = nc - 1) with some 250 map bits spread
    over three of the four rounds of 256 words -- a sparse record whose scan carries its base
    across rounds; slice 1 has more than 512 map bits in all four rounds and travels dense."""
    _assert_real_covers_span_the_rounds()


@pytest.mark.gpu
def test_gpu_real_covers_across_the_round_boundary():
    """2 x 520 x 504 (lm_words = 1024: four scan rounds) range-end covers embedded by PeeCodec;
    pack at widths {1, need, need + 3} equals the spec, unpack equals spec.map_prefix from the
    needed width on (test_real_covers_span_the_scan_rounds: what the records hold)."""
    from codec_tcc_amd.pee import PeeCodec
    r = REAL
    _assert_real_covers_span_the_rounds()      # before embedding: lm_count > 512, indices in several rounds
    covers = torch.from_numpy(_real_covers()).cuda()
    codec = PeeCodec(2, r["H"], r["W"], dtype="uint16", T=r["T"], maxval=r["maxval"])
    assert codec.lm_words == 1024
    enc = codec.embed(covers, [_real_bits(b) for b in range(2)], check=False)
    torch.cuda.synchronize()
    metas = [[int(x) for x in row] for row in enc.meta.cpu().numpy().view(np.int32)]
    rows = [[int(w) for w in row] for row in _u64(enc.lm)]
    counts = [m[S.LM_COUNT] for m in metas]
    assert [(m[S.END], m[S.LM_COUNT]) for m in metas] == [(e, int(i.size)) for e, i in _real_oracle()]
    assert max(counts) > 512 and metas[0][S.END] == codec.nc - 1
    assert counts == [len(S.set_bits(rw, m[S.END])) for rw, m in zip(rows, metas)]
    need = S.width_needed(metas, codec.lm_words)
    assert int(D.record_width_needed(enc.meta, codec.lm_words)) == need
    assert S.is_sparse(counts[0], need) and not S.is_sparse(counts[1], need)
    cols = S.dense_words_needed(metas)
    want_lm = np.array([S.map_prefix(m[S.END], rw, cols) for m, rw in zip(metas, rows)], dtype=np.uint64)
    for width in (1, need, need + 3):
        rec = D.pack_pee_records(enc.meta, enc.lm, width)
        want = np.array([S.pack(m, rw, width) for m, rw in zip(metas, rows)], dtype=np.uint64)
        _same(_u64(rec), want, f"real pack width {width}")
        meta2, lm2 = D.unpack_pee_records(rec, cols)
        assert torch.equal(meta2, enc.meta)
        if width >= need:
            _same(_u64(lm2), want_lm, f"real unpack width {width}")
        else:
            assert not np.array_equal(_u64(lm2), want_lm)
