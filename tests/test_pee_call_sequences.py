"""Long, mixed call sequences on ONE MED-PEE workspace (include/codec_tcc.h, the rules at
codec_pee_workspace_bytes): the epoch wrap of the self-cleaning look-back, both status-word
buffers under both kernels, state handed between families of calls, shape changes, graph
replays among eager calls, codec_pee_reset in mid-sequence and the gate table of a smaller
shape.  Every call goes through the C ABI on one workspace tensor and every output is compared
bit for bit, on the device, with references computed once on the CPU (oracle/pee_cpu.py,
tests/pee_gate_spec.py); nothing is copied to the host inside a sequence.

A WITNESS proves that a sequence reached the states it claims: after every call the two
status-word buffers, the control words (finished flags, the extract's look-back flag) and the
diagnostic counters are snapshotted from the workspace (offsets from tests/pee_ws_model.py, which
shares no code with the library) and compared with what the model says the library's registry
did -- self-cleaning or not, which epoch, which buffer, which tag.  A sequence that silently took
the zeroing path (buffer 1, tag 0) fails the witness instead of passing by being exact anyway.

What a self-cleaning call at epoch e (buffer par = e & 1, tag = e % 63 + 1) leaves:
  other buffer   every word 0 and every slice's other finished flag 0 -- copy-only chunks and
                 slices with an empty payload included;
  embed          every word of buffer par carries the tag in bits 56-61, and every slice's
                 finished flag of that parity holds tag + 1 in its low byte;
  extract        publishes only the chunks BEFORE the one holding `end` (nothing waits for the
                 others): those words carry the tag, the rest of buffer par and its finished
                 flags stay as they were -- 0 after self-cleaning calls, tag 0 after zeroing ones.

No debug knob is set: the tests see the state ordinary calls leave.  CODEC_PEE_ONEPASS=1 is set
as in the existing self-cleaning tests: it pins the look-back route the sequences are about
against a tuning environment that forces the two-pass path (the default takes the same route).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pee_gate_spec as GS
import pee_ws_model as M
from codec_tcc_amd import _lib, framing, synth
from oracle import pee_cpu as P

MAIN = (3, 130, 512, 2)      # 4160 items: 5 chunks, the last one partial
U8 = (2, 64, 1024, 1)        # 4096 items: 4 full chunks
TAIL = (2, 130, 512, 2)      # the main shape's smaller tail batch
SMALL = (2, 66, 256, 2)      # 1056 items: 2 chunks, another layout
BIG_F, SMALL_F = (7, 256, 256, 2), (1, 8, 8, 2)   # sequence F
T0, GATE, TMAX, TMAX2 = 2, 24, 16, 4
POOL = 5                     # coprime to 2, 63 and 126
CAND = 4 * M.CHUNK           # candidates per look-back chunk (W % 8 == 0)
KINDS = ("full", "chunk0", "empty0", "overflow", "boundary")


def _maxval(shape):
    return 4095 if shape[3] == 2 else 255


def _lm_words(shape):
    return max(1, ((shape[1] // 2) * (shape[2] // 2) + 63) // 64)


def _prm(shape, pw=1, T=T0):
    return _lib.PeeParams(B=shape[0], H=shape[1], W=shape[2], bytes=shape[3], T=T, maxval=_maxval(shape),
                          payload_words=int(pw), lm_words=_lm_words(shape))


def _cover(shape, k, b):
    """ct12 stretched by 21/16 and clipped at 4095 (uint8: its top 8 bits): the bright region, the
    top rows, saturates, so the slices have overflow-prone candidates and their location maps set
    bits.  Odd slices are upside down: their overflow-prone candidates lie in the last chunks."""
    img = synth.ct12(shape[1], shape[2], 1000 + 31 * k + b + 7 * shape[0] + shape[1]).astype(np.uint32)
    img = np.minimum(img * 21 >> 4, 4095).astype(np.uint16)
    if b % 2:
        img = np.ascontiguousarray(img[::-1])
    return img if shape[3] == 2 else (img >> 4).astype(np.uint8)


def _es(cover, T, maxval, G=None):
    """Expandable, safe (and active) candidates in index order: the ones that take payload bits."""
    x, a, b, c = P._grids(cover)
    _e, expand, _r, safe = P.classify(x, P.med(a, b, c), T, maxval)
    es = (expand & safe).ravel()
    return es if G is None else es & (GS.roughness(a, b, c) <= G).ravel()


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, int(n)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pool(shape):
    """POOL batches of (covers, payload bits), one of each kind of KINDS, with scheme 1's oracle
    results at T0.  Every batch has a slice whose `end` lies past chunk 0, so that an extract of
    it publishes a status word (the witness of its buffer and tag)."""
    B, H, W, _by = shape
    mv, nch = _maxval(shape), M.layout(shape).nchunks
    out = []
    for k, kind in enumerate(KINDS):
        covers = np.stack([_cover(shape, k, b) for b in range(B)])
        ess = [_es(c, T0, mv) for c in covers]
        caps = [int(e.sum()) for e in ess]
        if kind == "full":           # every slice filled to its capacity
            lens = list(caps)
        elif kind == "chunk0":       # slice 0 ends inside chunk 0: its later chunks are plain copies
            lens = [max(1, int(ess[0][:CAND].sum()) // 3)] + [caps[b] // 2 + 7 * b for b in range(1, B)]
        elif kind == "empty0":       # slice 0 carries nothing
            lens = [0] + [caps[b] * 3 // 4 - b for b in range(1, B)]
        elif kind == "overflow":     # the last slice is given more than fits: status 1
            lens = [caps[b] // 3 + b for b in range(B - 1)] + [caps[B - 1] + 50]
        else:                        # every slice's payload ends with a chunk's last expandable candidate
            lens = [int(ess[b][:CAND * (1 + b % (nch - 1))].sum()) for b in range(B)]
        bits = [_bits(n, 5000 + 100 * k + b) for b, n in enumerate(lens)]
        s1 = [P.pee_embed(covers[b], bits[b], T0, mv, truncate=True) for b in range(B)]
        out.append({"kind": kind, "covers": covers, "bits": bits, "es": ess, "s1": s1})
    return out


def _cend(end):
    return end // CAND if end >= 0 else -1


# ------------------------------------------------------------------ expected outputs (CPU)
def _record(shape, T, L_given, side, es, lm_count, route="lookback", gate=None):
    """The codec_pee_meta an embed writes, all 16 int32.  capacity / flags: the look-back pass
    stops counting after the chunk holding `end` (CODEC_PEE_PARTIAL unless that is the last
    chunk); the two-pass route and an overflowing slice count the whole slice."""
    _B, H, W, _by = shape
    nc, nch = es.size, M.layout(shape).nchunks
    end, cum = side["end"], np.cumsum(es)
    if side["status"] == 1 or route == "twopass":
        cap, flags = int(cum[-1]), 0
    else:
        ce = max(end, 0) // CAND
        cap, flags = int(cum[min(CAND * (ce + 1), nc) - 1]), 0 if ce == nch - 1 else _lib.PEE_PARTIAL
    return [T, _maxval(shape), L_given, end, nc, (nc + 1023) // 1024, end // 1024 if end >= 0 else -1,
            side["status"], cap, lm_count, H, W, flags, 0, 0 if gate is None else gate + 1, 0]


def _lm_rows(shape, lms):
    rows = np.zeros((len(lms), _lm_words(shape) * 64), np.uint8)
    for b, lm in enumerate(lms):
        rows[b, :lm.size] = lm
    return np.packbits(rows, axis=1, bitorder="little").view(np.int64)


def _raw(recs):
    return np.array([np.frombuffer(bytes(r), dtype=np.int32) for r in recs])


@functools.lru_cache(maxsize=None)
def expect(shape, families=("s1",)):
    """Per pool entry, the inputs and the expected outputs of the families asked for (numpy)."""
    B, H, W, _by = shape
    mv = _maxval(shape)
    entries = pool(shape)
    pw = max((len(b) + 63) // 64 for e in entries for b in e["bits"]) + 1
    out = []
    for e in entries:
        covers, bits = e["covers"], e["bits"]
        words, lens = framing.pack_bits(bits, words=pw)
        d = {"cov": covers, "words": words, "lens": np.array(lens, np.int32), "pw": pw}

        def scheme1(tag, Ts, G=None):
            if G is None:
                res = [P.pee_embed(covers[b], bits[b], Ts[b], mv, truncate=True) for b in range(B)]
            else:
                res = [GS.embed(covers[b], bits[b], Ts[b], G, mv) for b in range(B)]
            ess = [_es(covers[b], Ts[b], mv, G) for b in range(B)]
            d[tag + "_stego"] = np.stack([r[0] for r in res])
            for route in ("lookback", "twopass"):
                d[f"{tag}_meta_{route}"] = np.array(
                    [_record(shape, Ts[b], len(bits[b]), res[b][1], ess[b], int(res[b][1]["lm"].sum()), route, G)
                     for b in range(B)], np.int32)
            d[tag + "_lm"] = _lm_rows(shape, [r[1]["lm"] for r in res])
            d[tag + "_out"] = framing.pack_bits([bits[b][:res[b][1]["L"]] for b in range(B)], words=pw)[0]
            from codec_tcc_amd.pee import make_record
            d[tag + "_rec"] = _raw([make_record(H, W, T=Ts[b], maxval=mv, L=res[b][1]["L"], end=res[b][1]["end"],
                                                status=res[b][1]["status"], gate=G) for b in range(B)])
            nch = M.layout(shape).nchunks
            d[tag + "_xmask"] = np.array([[c < _cend(res[b][1]["end"]) for c in range(nch)] for b in range(B)])
            # chunks past the one holding `end` that hold overflow-prone candidates: the full
            # path publishes a count of them in bits 32-55 (its own at the least, when the
            # finished flag cut its look-back short), a plain copy publishes 0
            unsafe = []
            for b in range(B):
                x, a, bb, c = P._grids(covers[b])
                safe = P.classify(x, P.med(a, bb, c), Ts[b], mv)[3].ravel()
                unsafe.append([int((~safe[CAND * j:CAND * (j + 1)]).sum()) for j in range(nch)])
            d[tag + "_cmask"] = np.array([[j > _cend(res[b][1]["end"]) and res[b][1]["status"] == 0 and unsafe[b][j] > 0
                                           for j in range(nch)] for b in range(B)])

        def scheme2(tag, res, Ts):
            from codec_tcc_amd.pee import make_record
            d[tag + "_stego"] = np.stack([r[0] for r in res])
            recs, lms, masks = [], [], []
            for p in range(4):
                sides = [r[1]["passes"][p] for r in res]
                recs.append(_raw([make_record(H, W, T=Ts[b], maxval=mv, L=s["L"], end=s["end"], status=s["status"],
                                              lattice=p) for b, s in enumerate(sides)]))
                lms.append(_lm_rows(shape, [s["lm"] for s in sides]))
                masks.append(_lm_rows(shape, [np.ones(s["end"] + 1, np.uint8) for s in sides]))
            d[tag + "_rec"], d[tag + "_lm"], d[tag + "_lmmask"] = np.stack(recs), np.stack(lms), np.stack(masks)
            d[tag + "_out"] = framing.pack_bits([bits[b][:res[b][1]["L"]] for b in range(B)], words=pw)[0]

        scheme1("s1", [T0] * B)
        if "cap" in families:
            curves = [P.capacity_curve(c, TMAX, mv) for c in covers]
            d["caps"] = np.array(curves, np.int32)
            d["tsel"] = np.array([P.select_T(covers[b], len(bits[b]), TMAX, mv) for b in range(B)], np.int32)
            scheme1("auto", [int(t) for t in d["tsel"]])
        if "multi" in families:
            scheme2("m2", [P.pee_embed_multi(covers[b], bits[b], T0, maxval=mv) for b in range(B)], [T0] * B)
            res, ts = [], []
            for b in range(B):   # the first T in 1..TMAX2 that places every bit, else TMAX2 (truncated)
                for T in range(1, TMAX2 + 1):
                    st, side = P.pee_embed_multi(covers[b], bits[b], T, maxval=mv)
                    if side["status"] == 0:
                        break
                res.append((st, side))
                ts.append(T)
            scheme2("m2a", res, ts)
            d["m2a_tsel"] = np.array(ts, np.int32)
        if "gate" in families:
            scheme1("g", [T0] * B, GATE)
            tabs = [GS.table(c, TMAX, mv) for c in covers]
            d["gn"] = np.array([t[0] for t in tabs], np.int32)
            d["ghs"] = np.array([t[1] for t in tabs], np.int32)
        out.append(d)
    return out


ALL = ("s1", "cap", "multi", "gate")
# scheme 2's records: the fields its oracle defines (T, L, end, status, lattice)
M2_COLS = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0], np.int32)

# ------------------------------------------------------------------ CPU tests


def _params_for(shape):
    return C.byref(_prm(shape))


@pytest.mark.parametrize("shape", [MAIN, U8, TAIL, SMALL, BIG_F, SMALL_F, (1, 2048, 2048, 2), (5, 37, 53, 1),
                                   (7, 1, 1, 1), (31, 513, 520, 2)])
def test_model_layout_matches_library(shape):
    """The two cross-checks that tie the modelled layout to the library (host entries only), plus
    the diagnostic counters' offset and the gated workspace's size."""
    lib = _lib.load()
    L = M.layout(shape)
    assert L.total == lib.codec_pee_workspace_bytes(_params_for(shape))
    assert L.ctl == lib.codec_pee_extract_flag_offset(_params_for(shape)) - 4
    assert L.extract_flag == lib.codec_pee_extract_flag_offset(_params_for(shape))
    assert L.diag == lib.codec_pee_diag_offset(_params_for(shape))
    if (shape[1] // 2) * (shape[2] // 2) <= GS.NC_MAX:
        assert M.gate_total(shape) == lib.codec_pee_gate_workspace_bytes(_params_for(shape), TMAX)
    # the regions follow one another and the witness's words lie inside theirs
    assert L.cnt < L.off <= L.st < L.ctl < L.ctl_end <= L.diag < L.diag + 16 <= L.hist < L.hist_end <= L.sink < L.total
    assert L.status_word(1, shape[0] - 1, L.nchunks - 1) + 8 == L.ctl
    assert L.fin_flag(1, shape[0] - 1) + 4 <= L.ctl_end


def test_model_registry_rules():
    """The registry as the header states it: first use, epochs, the wrap, shape changes, capture,
    reset, and which calls are self-cleaning."""
    r = M.Registry()
    s = r.call("embed", MAIN)
    assert (s.sc, s.epoch, s.par, s.tag, s.fresh, s.rezero) == (True, 0, 0, 1, True, False)
    s = r.call("extract", MAIN)
    assert (s.sc, s.epoch, s.par, s.tag, s.fresh) == (True, 1, 1, 2, False)
    for kind, kw in [("embed", {"inplace": True}), ("extract", {"inplace": True}), ("gate_embed", {}),
                     ("gate_extract", {}), ("embed", {"aligned": False}), ("capacity", {}), ("multi_extract", {}),
                     ("multi_embed_auto", {}), ("gate_capacity", {})]:
        s = r.call(kind, MAIN, **kw)
        assert not s.sc and s.epoch is None and not s.rezero, kind
        assert s.tag == (0 if s.kernel else None) and s.par == (1 if s.kernel else None), kind
    assert r.call("embed", MAIN, aligned=False).kernel is None       # the two-pass route: no look-back
    assert r.call("multi_embed", MAIN).epoch == 2                    # scheme 2's pass 0 is scheme 1's embed
    assert not r.call("embed", (8,) + MAIN[1:]).sc                   # B > 7: not the flat route
    s = r.call("embed", MAIN)
    assert (s.rezero, s.epoch, s.tag, s.par) == (True, 0, 1, 0)      # a shape change restarts the epochs
    seen = [r.call("extract" if i % 3 else "embed", MAIN) for i in range(1, 2 * M.EPOCHS + 3)]
    assert [x.epoch for x in seen[:4]] == [1, 2, 3, 4] and seen[M.EPOCHS - 2].epoch == 125
    assert (seen[M.EPOCHS - 1].epoch, seen[M.EPOCHS - 1].par, seen[M.EPOCHS - 1].tag) == (0, 0, 1)
    assert (seen[61].epoch, seen[61].tag, seen[62].tag, seen[62].par) == (62, 63, 1, 1)
    assert {(x.par, x.tag) for x in seen} == {(p, t) for p in (0, 1) for t in range(1, 64)}
    # a shape change that moves the counters zeroes them too; one that does not keeps them
    assert r.call("capacity", TAIL).moved_diag and M.layout(TAIL).diag != M.layout(MAIN).diag
    same_diag = (MAIN[0], MAIN[1] + 2, MAIN[2], MAIN[3])
    assert M.layout(same_diag).diag == M.layout(MAIN).diag
    r.call("embed", MAIN)
    s = r.call("embed", same_diag)
    assert s.rezero and not s.moved_diag and s.epoch == 0
    # capture: the captured call zeroes; afterwards the captured shape keeps the fast path, others lose it
    r.call("embed", MAIN)
    assert not r.call("embed", MAIN, capturing=True).sc
    assert r.call("embed", MAIN).sc and not r.call("embed", TAIL).sc and r.call("embed", MAIN).epoch == 0
    r.reset(MAIN)                                                    # keeps the captured shape
    assert r.call("embed", MAIN).epoch == 0 and not r.call("extract", SMALL).sc
    fresh = M.Registry()
    fresh.reset(MAIN)
    s = fresh.call("extract", MAIN)
    assert (s.epoch, s.fresh) == (0, False)


@pytest.mark.parametrize("shape", [MAIN, U8, TAIL, SMALL])
def test_pool_has_every_kind(shape):
    """The pool's batches differ in where `end` falls, by the oracle's `end` and the model's
    chunk count: filled to capacity, inside chunk 0, no payload, overflow, a chunk boundary."""
    nch = M.layout(shape).nchunks
    assert nch >= 2 and len(pool(shape)) == POOL and POOL % 2 and POOL % 3 and POOL % 7
    for e in pool(shape):
        sides = [s for _st, s in e["s1"]]
        ends = [s["end"] for s in sides]
        if nch >= 4:
            assert any(_cend(x) >= 1 for x in ends), e["kind"]      # an extract of it publishes a word
        if e["kind"] == "full":
            assert all(s["status"] == 0 and s["L"] == s["capacity"] > 0 for s in sides)
        elif e["kind"] == "chunk0":
            assert 0 <= ends[0] < CAND and sides[0]["status"] == 0
        elif e["kind"] == "empty0":
            assert ends[0] == -1 and sides[0]["L"] == 0
        elif e["kind"] == "overflow":
            assert sides[-1]["status"] == 1 and ends[-1] == e["es"][-1].size - 1
            assert all(s["status"] == 0 for s in sides[:-1])
        else:
            for b, s in enumerate(sides):   # the chunk holding `end` has no expandable candidate after it
                c = _cend(s["end"])
                assert 0 <= c < nch - 1 and s["status"] == 0, (b, c)
                assert not e["es"][b][s["end"] + 1:CAND * (c + 1)].any() and e["es"][b][CAND * (c + 1):].any()
    assert nch < 4 or len({_cend(s["end"]) for e in pool(shape) for _st, s in e["s1"]}) >= 3


FAMILIES = ("embed", "embed_ip", "extract", "extract_ip", "capacity", "embed_auto", "multi_embed", "multi_extract",
            "multi_embed_auto", "gate_capacity", "gate_embed", "gate_extract", "embed_2p", "extract_2p")


@functools.lru_cache(maxsize=None)
def schedule_b():
    """Sequence B's order: a seeded Euler circuit of the complete directed graph on the families
    (loops included), so every ordered pair of families occurs as two consecutive calls."""
    rng = np.random.default_rng(20)
    nxt = {f: list(rng.permutation(len(FAMILIES))) for f in range(len(FAMILIES))}
    stack, walk = [0], []
    while stack:                       # Hierholzer
        v = stack[-1]
        if nxt[v]:
            stack.append(int(nxt[v].pop()))
        else:
            walk.append(stack.pop())
    return tuple(FAMILIES[v] for v in reversed(walk))


def test_schedule_b_has_every_ordered_pair():
    s = schedule_b()
    assert len(s) == len(FAMILIES) ** 2 + 1 >= 60
    pairs = set(zip(s, s[1:]))
    assert pairs == {(a, b) for a in FAMILIES for b in FAMILIES}
    assert {a for a, b in pairs if b == "capacity"} == set(FAMILIES)   # the capacity pass after every family


def test_gate_table_of_small_shape_overlaps_big_hist():
    """Sequence F's arithmetic: the table of codec_pee_gate_capacity at SMALL_F lies behind
    SMALL_F's own layout, which is inside BIG_F's: on BIG_F's capacity bins."""
    big, lo_hi = M.layout(BIG_F), M.gate_bins(SMALL_F)
    assert lo_hi == (2560, 2560 + 4 * (17 * 16 + 1)) and M.layout(SMALL_F).total == 2560
    assert (big.ctl, big.ctl_end, big.diag, big.hist, big.hist_end) == (1472, 2496, 2496, 2560, 4380)
    assert big.hist <= lo_hi[0] < lo_hi[1] <= big.arrivals < big.total
    # bin w of the table is bin w % 64 of BIG_F's slice w // 64: the first 4 slices wholly, 17 bins of the 5th
    assert (lo_hi[1] - big.hist) // (4 * M.TMAX_MAX) == 4 and (lo_hi[1] - big.hist) // 4 % M.TMAX_MAX == 17
    assert M.gate_total(SMALL_F) <= M.gate_total(BIG_F)


# ------------------------------------------------------------------ the GPU harness
class Rig:
    """One workspace, the model of its registry entry, device copies of the pools and the logs
    (per call: output comparisons, a snapshot of the witness words), read back once at the end."""

    def __init__(self, shapes, slot, families=("s1",), calls=400, extra=()):
        import torch
        self.t, self.lib = torch, _lib.load()
        need = max(M.gate_total(s) for s in tuple(shapes) + tuple(extra))
        # The library keys its registry by workspace pointer and remembers a graph capture across
        # codec_pee_reset, so a workspace at an address an earlier test captured on would lose the
        # self-cleaning path.  This one lies in a block of its own size class, at an offset no
        # other test uses.
        self.block = torch.zeros((2 << 20) + need, dtype=torch.uint8, device="cuda")
        off = (1 << 20) + 4096 * slot
        self.ws = self.block[off:off + need]
        self.reg = M.Registry()
        self.shapes, self.families = shapes, families
        self.dev = {s: [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()
                         if isinstance(v, np.ndarray)} for d in expect(s, families)] for s in shapes}
        self.pw = {s: expect(s, families)[0]["pw"] for s in shapes}
        self.pw.update({s: 1 for s in extra})     # shapes without a pool: table calls only
        self.buf = {s: self._buffers(s) for s in self.pw}
        self.wit_w = max(M.layout(s).ctl_end - M.layout(s).st for s in self.pw) + 16
        self.wit = torch.zeros((calls, self.wit_w), dtype=torch.uint8, device="cuda")
        self.ok = torch.ones((calls, 8), dtype=torch.bool, device="cuda")
        self.names = [None] * calls
        self.calls = []          # (label, shape, model steps, checks, info)
        self.copy_only = 0       # embed chunks seen to have taken the plain-copy path (finish)
        self.m2cols = torch.from_numpy(M2_COLS).cuda()
        self.reset(shapes[0])

    def _buffers(self, s):
        t = self.t
        B, H, W, by = s
        px = t.uint16 if by == 2 else t.uint8
        lmw, pw = _lm_words(s), self.pw[s]
        b = {"stego": t.empty((B, H, W), dtype=px, device="cuda"), "rest": t.empty((B, H, W), dtype=px, device="cuda"),
             "meta": t.empty((4, B, 16), dtype=t.int32, device="cuda"), "lm": t.empty((4, B, lmw), dtype=t.int64, device="cuda"),
             "out": t.empty((B, pw), dtype=t.int64, device="cuda"), "caps": t.empty((B, TMAX), dtype=t.int32, device="cuda"),
             "tsel": t.empty(B, dtype=t.int32, device="cuda"), "gn": t.empty((B, 16), dtype=t.int32, device="cuda"),
             "ghs": t.empty((B, TMAX, 16), dtype=t.int32, device="cuda"),
             "tg": t.full((B,), T0, dtype=t.int32, device="cuda"), "gg": t.full((B,), GATE, dtype=t.int32, device="cuda")}
        for name in ("ua", "ub"):   # views one pixel into their buffers: not vector-aligned (the two-pass route)
            b[name] = t.empty(B * H * W + 1, dtype=px, device="cuda")[1:].view(B, H, W)
        return b

    # ---- plumbing
    def _call(self, fn, prm, *args):
        from codec_tcc_amd.codec import _stream
        a = [x.data_ptr() if hasattr(x, "data_ptr") else x for x in args]
        _lib.check(getattr(self.lib, fn)(C.byref(prm), *a, self.ws.data_ptr(), self.ws.numel(), _stream()), fn)

    def reset(self, shape):
        from codec_tcc_amd.codec import _stream
        _lib.check(self.lib.codec_pee_reset(C.byref(_prm(shape)), self.ws.data_ptr(), self.ws.numel(), _stream()), "reset")
        self.reg.reset(shape)

    def _scrub(self, s, *names):
        """Outputs start from a pattern no result holds, so a call must write all of them."""
        for n in names:
            self.buf[s][n].view(self.t.uint8).fill_(0xA5)

    def _log(self, label, s, steps, checks, **info):
        i = len(self.calls)
        L = M.layout(s)
        n = L.ctl_end - L.st
        self.wit[i, :n].copy_(self.ws[L.st:L.ctl_end])
        self.wit[i, n:n + 16].copy_(self.ws[L.diag:L.diag + 16])
        for j, (name, got, ref, mask) in enumerate(checks):
            if mask is None:
                self.ok[i, j] = (got.contiguous().view(self.t.uint8) == ref.contiguous().view(self.t.uint8)).all()
            elif mask is self.m2cols:
                self.ok[i, j] = (((got - ref) * mask) == 0).all()
            else:
                self.ok[i, j] = (((got ^ ref) & mask) == 0).all()
        self.calls.append((label, s, steps, [c[0] for c in checks], info))

    # ---- the families.  k: the pool entry
    def embed(self, s, k, *, inplace=False, aligned=True, capturing=False, log=True):
        d, b = self.dev[s][k], self.buf[s]
        prm = _prm(s, self.pw[s])
        route = "lookback" if aligned else "twopass"
        if inplace or not aligned:
            src = b["ua"] if not aligned else b["stego"]
            src.copy_(d["cov"])
            dst = src if inplace else b["ub"]
        else:
            src, dst = d["cov"], b["stego"]
        if not inplace:
            dst.view(self.t.uint8 if s[3] == 1 else self.t.int16).fill_(0x5A)
        self._scrub(s, "meta", "lm")
        self._call("codec_pee_embed_ts", prm, src, dst, d["words"], d["lens"], None, b["meta"][0], b["lm"][0])
        step = self.reg.call("embed", s, inplace=inplace, aligned=aligned, capturing=capturing)
        if log:
            self._log("embed" + ("_ip" if inplace else "") + ("" if aligned else "_2p"), s, [step],
                      [("stego", dst, d["s1_stego"], None), ("meta", b["meta"][0], d[f"s1_meta_{route}"], None),
                       ("lm", b["lm"][0], d["s1_lm"], None)], k=k, kernel="E")
        return step

    def extract(self, s, k, *, inplace=False, aligned=True, capturing=False, log=True, tag="s1", fn="codec_pee_extract"):
        d, b = self.dev[s][k], self.buf[s]
        prm = _prm(s, self.pw[s])
        if inplace or not aligned:
            src = b["ua"] if not aligned else b["rest"]
            src.copy_(d[tag + "_stego"])
            dst = src if inplace else b["ub"]
        else:
            src, dst = d[tag + "_stego"], b["rest"]
        if not inplace:
            dst.view(self.t.uint8 if s[3] == 1 else self.t.int16).fill_(0x5A)
        self._scrub(s, "out")
        self._call(fn, prm, src, d[tag + "_rec"], d[tag + "_lm"], dst, b["out"])
        kind = "gate_extract" if tag == "g" else "extract"
        step = self.reg.call(kind, s, inplace=inplace, aligned=aligned, capturing=capturing)
        if log:
            self._log(kind + ("_ip" if inplace else "") + ("" if aligned else "_2p"), s, [step],
                      [("cover", dst, d["cov"], None), ("payload", b["out"], d[tag + "_out"], None)], k=k, kernel="X",
                      xmask=tag + "_xmask")
        return step

    def capacity(self, s, k):
        d, b = self.dev[s][k], self.buf[s]
        self._scrub(s, "caps", "tsel")
        self._call("codec_pee_capacity", _prm(s), d["cov"], TMAX, d["lens"], b["caps"], b["tsel"])
        self._log("capacity", s, [self.reg.call("capacity", s)],
                  [("caps", b["caps"], d["caps"], None), ("t_out", b["tsel"], d["tsel"], None)], k=k)

    def embed_auto(self, s, k):
        d, b = self.dev[s][k], self.buf[s]
        self._scrub(s, "stego", "meta", "lm", "tsel")
        self._call("codec_pee_embed_auto", _prm(s, self.pw[s]), d["cov"], b["stego"], d["words"], d["lens"], TMAX,
                   b["tsel"], b["meta"][0], b["lm"][0])
        steps = [self.reg.call("capacity", s), self.reg.call("embed", s)]
        self._log("embed_auto", s, steps,
                  [("stego", b["stego"], d["auto_stego"], None), ("meta", b["meta"][0], d["auto_meta_lookback"], None),
                   ("lm", b["lm"][0], d["auto_lm"], None), ("t_out", b["tsel"], d["tsel"], None)], k=k, kernel="E")

    def multi_embed(self, s, k, auto=False):
        d, b = self.dev[s][k], self.buf[s]
        tag = "m2a" if auto else "m2"
        self._scrub(s, "stego", "meta", "lm", "tsel")
        if auto:
            self._call("codec_pee_multi_embed_auto", _prm(s, self.pw[s]), d["cov"], b["stego"], d["words"], d["lens"], 1,
                       TMAX2, b["tsel"], b["meta"], b["lm"])
            steps = [self.reg.call("multi_embed_auto", s)]
        else:
            self._call("codec_pee_multi_embed", _prm(s, self.pw[s]), d["cov"], b["stego"], d["words"], d["lens"],
                       b["meta"], b["lm"])
            steps = [self.reg.call("multi_embed", s)]
        checks = [("stego", b["stego"], d[tag + "_stego"], None), ("records", b["meta"], d[tag + "_rec"], self.m2cols),
                  ("lm", b["lm"], d[tag + "_lm"], d[tag + "_lmmask"])]
        if auto:
            checks.append(("t_out", b["tsel"], d["m2a_tsel"], None))
        self._log("multi_embed_auto" if auto else "multi_embed", s, steps, checks, k=k,
                  kernel=None if auto else "E")

    def multi_extract(self, s, k):
        d, b = self.dev[s][k], self.buf[s]
        self._scrub(s, "rest", "out")
        self._call("codec_pee_multi_extract", _prm(s, self.pw[s]), d["m2_stego"], d["m2_rec"], d["m2_lm"], b["rest"],
                   b["out"])
        self._log("multi_extract", s, [self.reg.call("multi_extract", s)],
                  [("cover", b["rest"], d["cov"], None), ("payload", b["out"], d["m2_out"], None)], k=k)

    def gate_capacity(self, s, k, cov=None, refs=None):
        d, b = (self.dev[s][k] if refs is None else refs), self.buf[s]
        self._scrub(s, "gn", "ghs")
        self._call("codec_pee_gate_capacity", _prm(s), d["cov"] if cov is None else cov, TMAX, 0, -1, None, b["gn"],
                   b["ghs"], None, None, None)
        self._log("gate_capacity", s, [self.reg.call("gate_capacity", s)],
                  [("n", b["gn"], d["gn"], None), ("hs", b["ghs"], d["ghs"], None)], k=k)

    def gate_embed(self, s, k):
        d, b = self.dev[s][k], self.buf[s]
        self._scrub(s, "stego", "meta", "lm")
        self._call("codec_pee_gate_embed", _prm(s, self.pw[s]), d["cov"], b["stego"], d["words"], d["lens"], b["tg"],
                   b["gg"], b["meta"][0], b["lm"][0])
        self._log("gate_embed", s, [self.reg.call("gate_embed", s)],
                  [("stego", b["stego"], d["g_stego"], None), ("meta", b["meta"][0], d["g_meta_lookback"], None),
                   ("lm", b["lm"][0], d["g_lm"], None)], k=k, kernel="E")

    def run(self, family, s, k):
        if family in ("embed", "embed_ip", "embed_2p"):
            self.embed(s, k, inplace=family == "embed_ip", aligned=family != "embed_2p")
        elif family in ("extract", "extract_ip", "extract_2p"):
            self.extract(s, k, inplace=family == "extract_ip", aligned=family != "extract_2p")
        elif family == "gate_extract":
            self.extract(s, k, tag="g", fn="codec_pee_gate_extract")
        elif family == "multi_embed_auto":
            self.multi_embed(s, k, auto=True)
        else:
            getattr(self, family)(s, k)

    # ---- read the logs back and judge them
    def finish(self, pure_sc=False):
        """Every output comparison, then the witness of every call against the model.  Returns
        the witnessed (kernel, parity, tag) of the self-cleaning calls, in call order.
        pure_sc: the sequence holds self-cleaning calls only, so what an extract leaves
        unpublished in its own buffer is exactly 0."""
        self.t.cuda.synchronize()
        n = len(self.calls)
        ok, wit = self.ok[:n].cpu().numpy(), self.wit[:n].cpu().numpy()
        seen = []
        for i, (label, s, steps, names, info) in enumerate(self.calls):
            where = f"call {i} ({label}, pool entry {info.get('k')})"
            for j, name in enumerate(names):
                assert ok[i, j], f"{where}: {name} differs from its reference"
            L, B = M.layout(s), s[0]
            nst = L.ctl - L.st
            words = wit[i, :nst].view(np.uint64).reshape(2, B, L.nchunks)
            ctl = wit[i, nst:L.ctl_end - L.st].view(np.uint32)
            fins = np.stack([ctl[32 + 32 * np.arange(B) + M.LINE_FIN[p]] for p in (0, 1)])
            diag = wit[i, L.ctl_end - L.st:L.ctl_end - L.st + 16].view(np.uint32)
            assert not diag.any(), f"{where}: look-back fallback / timeout counters {diag.tolist()}"
            assert ctl[1] == 0, f"{where}: the extract's look-back flag is set"
            tags = (words >> np.uint64(M.TAG_SHIFT)).astype(np.int64) & M.TAG_MASK
            lb = [st for st in steps if st.kernel]
            if pure_sc:
                assert lb and lb[-1].sc, f"{where}: the model says this call is not self-cleaning"
            if not lb or not lb[-1].sc:
                # a zeroing look-back call or none: no word of either buffer carries a live tag
                # unless an earlier self-cleaning call left it (checked when that call was made)
                continue
            st = lb[-1]
            par, tag = st.par, st.tag
            assert not words[1 - par].any() and not fins[1 - par].any(), \
                f"{where}: epoch {st.epoch} left buffer {1 - par} uncleared: words {words[1 - par].tolist()}, " \
                f"flags {fins[1 - par].tolist()}"
            if info["kernel"] == "E":
                assert (tags[par] == tag).all(), f"{where}: epoch {st.epoch}, buffer {par} tags {tags[par].tolist()} != {tag}"
                assert ((fins[par] & 0xFF) == tag + 1).all(), f"{where}: finished flags {fins[par].tolist()}, tag {tag}"
                if label == "embed":
                    cmask = expect(s, self.families)[info["k"]]["s1_cmask"]
                    self.copy_only += int(((((words[par] >> np.uint64(32)) & np.uint64(0xFFFFFF)) == 0) & cmask).sum())
            else:
                mask = expect(s, self.families)[info["k"]][info["xmask"]]
                assert (tags[par][mask] == tag).all(), f"{where}: epoch {st.epoch}, buffer {par} tags {tags[par].tolist()}"
                if pure_sc:
                    assert not words[par][~mask].any() and not fins[par].any(), f"{where}: {words[par].tolist()}"
                else:
                    assert not tags[par][~mask].any(), f"{where}: a foreign tag in buffer {par}: {tags[par].tolist()}"
            # what the workspace itself says, without the model: one buffer carries one live tag,
            # and (buffer, tag) name the epoch.  (An extract whose slices all end in chunk 0
            # publishes nothing: it shows only the cleared other buffer.)
            live = [p for p in (0, 1) if tags[p].any()]
            if info["kernel"] == "X" and not mask.any():
                assert not live, where
                continue
            assert live == [par] and set(tags[par][tags[par] > 0].tolist()) == {tag}, where
            wtag = int(tags[live[0]].max())
            epoch = next(e for e in (wtag - 1, wtag - 1 + M.TAGS) if e % 2 == live[0])
            assert epoch == st.epoch, f"{where}: the workspace shows epoch {epoch}, the model {st.epoch}"
            seen.append((info["kernel"], live[0], wtag, epoch))
        return seen

    def diagnostics(self, s):
        L = M.layout(s)
        return self.ws[L.diag:L.diag + 16].view(self.t.int32).cpu().tolist(), \
            int(self.ws[L.extract_flag:L.extract_flag + 4].view(self.t.int32).item())


@pytest.fixture
def onepass(monkeypatch):
    pytest.importorskip("torch")
    monkeypatch.setenv("CODEC_PEE_ONEPASS", "1")


PATTERN = "EX" "EEXX" "EXX" "EEEX"   # 13 calls: an odd period, so both kernels meet both parities


@pytest.mark.gpu
@pytest.mark.parametrize("shape,grid", [(MAIN, None), (U8, None), (MAIN, 8)],
                         ids=["u16_3x130x512", "u8_2x64x1024", "u16_3x130x512_grid8"])
def test_gpu_seq_a_epoch_wrap(shape, grid, onepass, monkeypatch):
    """Sequence A: 273 self-cleaning calls on one workspace -- more than twice the epoch
    counter's period of 126 -- embeds and extracts in an order of odd period over a pool of 5
    batches, so the same (buffer, tag) never meets the same data twice running.  Every output
    of every call is exact, every call leaves the state the design states, and the witness read
    from the workspace shows both kernels on both buffers, every tag 1..63, the step from tag 63
    to tag 1 and the step from epoch 125 to epoch 0; no chunk ever needed the fallback.
    grid8: the same on a grid of 8 workgroups that walk the 15 slots (CODEC_PEE_1P_WGS, a launch
    shape, not a fault knob).  On the full grid every chunk of these small slices is resident at
    once and none starts after its slice's finished flag went up, so the plain-copy path of the
    chunks past `end` is never taken; here slice 1's chunks 3 and 4 start after a workgroup has
    finished a chunk of slice 0, and the witness counts the plain copies it saw (a status word
    with an empty overflow-count field where the full path publishes a count)."""
    assert len(PATTERN) % 2 == 1
    if grid:
        monkeypatch.setenv("CODEC_PEE_1P_WGS", str(grid))
    rig = Rig([shape], slot=(1 if shape == MAIN else 2) + (7 if grid else 0))
    ne = nx = 0
    for kind in PATTERN * 21:
        if kind == "E":
            rig.embed(shape, ne % POOL)
            ne += 1
        else:
            rig.extract(shape, nx % POOL)
            nx += 1
    assert len(rig.calls) >= 2 * M.EPOCHS + 10
    seen = rig.finish(pure_sc=True)
    assert len(seen) == len(rig.calls)
    assert [e for _k, _p, _t, e in seen] == [i % M.EPOCHS for i in range(len(seen))]
    assert {(k, p) for k, p, _t, _e in seen} == {("E", 0), ("E", 1), ("X", 0), ("X", 1)}
    assert {t for _k, _p, t, _e in seen} == set(range(1, 64))
    steps = {(a[1:3], b[1:3]) for a, b in zip(seen, seen[1:])}
    assert ((0, 63), (1, 1)) in steps                   # tag 63 -> tag 1 (epoch 62 -> 63)
    assert ((1, 63), (0, 1)) in steps                   # epoch 125 -> epoch 0
    assert rig.diagnostics(shape) == ([0, 0, 0, 0], 0)
    print(f"plain-copy chunks witnessed: {rig.copy_only}")
    if grid:
        assert rig.copy_only >= 1


@pytest.mark.gpu
def test_gpu_seq_b_mixed_families(onepass):
    """Sequence B: 197 calls of 14 families on one workspace at the main shape, every ordered
    pair of families as two consecutive calls (schedule_b): scheme 1 out of place, in place and
    through unaligned views (the two-pass route, which writes cnt / off), the capacity pass,
    T = "auto", scheme 2 (pass 0 draws a self-cleaning epoch; passes 1-3 write cnt / off) and its
    T = "auto", the gated table, embed and extract.  Every call equals its oracle, and every
    self-cleaning call leaves the state the model predicts, whatever family ran before it."""
    rig = Rig([MAIN], slot=3, families=ALL)
    for i, fam in enumerate(schedule_b()):
        rig.run(fam, MAIN, i % POOL)
    seen = rig.finish()
    assert len(rig.calls) == len(schedule_b())
    # embed, embed_auto and multi_embed draw one epoch each, and so does extract
    assert len(seen) == sum(f in ("embed", "embed_auto", "multi_embed", "extract") for f in schedule_b())
    assert {(k, p) for k, p, _t, _e in seen} == {("E", 0), ("E", 1), ("X", 0), ("X", 1)}
    assert rig.diagnostics(MAIN) == ([0, 0, 0, 0], 0)


@pytest.mark.gpu
def test_gpu_seq_c_shape_changes(onepass):
    """Sequence C: one workspace sized for (3, 130, 512) serves (3, 130, 512), (2, 130, 512) and
    (2, 66, 256) in turn, every ordered pair of shapes as a change, each change followed by calls
    of four families.  The first self-cleaning call after a change restarts at epoch 0 (buffer 0,
    tag 1) -- the model predicts it, the witness confirms it -- and the diagnostic counters,
    which every one of these changes moves, read 0."""
    rig = Rig([MAIN, TAIL, SMALL], slot=4, families=("s1", "cap"))
    assert len({M.layout(s).diag for s in (MAIN, TAIL, SMALL)}) == 3
    order = [MAIN, TAIL, MAIN, SMALL, TAIL, SMALL, MAIN, TAIL]
    assert {(a, b) for a, b in zip(order, order[1:])} >= {(a, b) for a in order for b in order if a != b}
    firsts = []
    for n, s in enumerate(order):
        first = len(rig.calls)
        for j, fam in enumerate(["embed", "extract", "capacity", "embed_auto", "extract", "embed", "embed"][:5 + n % 3]):
            rig.run(fam, s, (n + j) % POOL)
        firsts.append(first)
    seen = rig.finish()
    for n, first in enumerate(firsts):
        st = rig.calls[first][2][0]
        assert (st.rezero, st.moved_diag) == (n > 0, n > 0), n
        assert (st.epoch, st.par, st.tag) == (0, 0, 1), n
    assert sum(e == 0 for _k, _p, _t, e in seen) == len(order)
    assert rig.diagnostics(TAIL) == ([0, 0, 0, 0], 0)


@pytest.mark.gpu
def test_gpu_seq_d_graph_replays_among_eager_calls(onepass):
    """Sequence D: an embed + extract step captured into a graph on the workspace, then 10 rounds
    of replay, eager embed, eager extract, eager embed, replay, eager extract (and one more eager
    embed in every other round, so that both kernels meet both buffers), all at the captured
    shape.  The header says such eager calls keep the fast path: the witness shows every one of
    them self-cleaning, with epochs that go on across the replays (which zero the state and use
    buffer 1 untagged), and every output of replays and eager calls is exact."""
    from codec_tcc_amd import graphs
    rig = Rig([MAIN], slot=5)
    t = rig.t
    d, b = rig.dev[MAIN][0], rig.buf[MAIN]
    g_stego, g_rest = t.empty_like(b["stego"]), t.empty_like(b["rest"])
    g_meta, g_lm, g_out = t.empty_like(b["meta"][0]), t.empty_like(b["lm"][0]), t.empty_like(b["out"])
    prm = _prm(MAIN, rig.pw[MAIN])

    def step():
        capturing = t.cuda.is_current_stream_capturing()   # what the library asks its stream
        rig._call("codec_pee_embed_ts", prm, d["cov"], g_stego, d["words"], d["lens"], None, g_meta, g_lm)
        rig.reg.call("embed", MAIN, capturing=capturing)
        rig._call("codec_pee_extract", prm, g_stego, g_meta, g_lm, g_rest, g_out)
        rig.reg.call("extract", MAIN, capturing=capturing)

    graph = graphs.capture(step)     # two eager warm-up steps (4 epochs), then the captured one
    assert [s.sc for s in rig.reg.log] == [True] * 4 + [False] * 2 and rig.reg.entry.epoch == 4
    replay_ok = t.ones((20, 5), dtype=t.bool, device="cuda")

    def replay(i):
        for x in (g_stego, g_rest, g_meta, g_lm, g_out):
            x.view(t.uint8).fill_(0xA5)
        graph.replay()
        for j, (got, ref) in enumerate([(g_stego, d["s1_stego"]), (g_meta, d["s1_meta_lookback"]), (g_lm, d["s1_lm"]),
                                        (g_rest, d["cov"]), (g_out, d["s1_out"])]):
            replay_ok[i, j] = (got.view(t.uint8) == ref.contiguous().view(t.uint8)).all()

    for r in range(10):
        replay(2 * r)
        rig.embed(MAIN, (3 * r + 1) % POOL)
        rig.extract(MAIN, (3 * r + 2) % POOL)
        rig.embed(MAIN, (3 * r + 3) % POOL)
        replay(2 * r + 1)
        rig.extract(MAIN, (3 * r + 4) % POOL)
        if r % 2:   # an odd number of eager calls: the next rounds meet the other buffers
            rig.embed(MAIN, (3 * r) % POOL)
    seen = rig.finish()
    assert replay_ok.cpu().numpy().all(), replay_ok.cpu().numpy()
    assert len(seen) == 45 and [e for _k, _p, _t, e in seen] == list(range(4, 49))
    assert {(k, p) for k, p, _t, _e in seen} == {("E", 0), ("E", 1), ("X", 0), ("X", 1)}
    assert rig.diagnostics(MAIN) == ([0, 0, 0, 0], 0)


@pytest.mark.gpu
def test_gpu_seq_e_reset_in_mid_sequence(onepass):
    """Sequence E: codec_pee_reset at an odd epoch away from a wrap (after 7 self-cleaning calls)
    restarts the epochs at 0 -- the model restarts, the witness agrees -- and the next 10 calls
    are exact."""
    rig = Rig([MAIN], slot=6)
    for i in range(7):
        (rig.embed if i % 3 != 1 else rig.extract)(MAIN, i % POOL)
    assert rig.reg.entry.epoch == 7
    rig.reset(MAIN)
    for i in range(10):
        (rig.extract if i % 3 != 1 else rig.embed)(MAIN, (i + 2) % POOL)
    seen = rig.finish(pure_sc=True)
    assert [e for _k, _p, _t, e in seen] == list(range(7)) + list(range(10))
    assert seen[7][:3] == ("X", 0, 1)
    assert rig.diagnostics(MAIN) == ([0, 0, 0, 0], 0)


@pytest.mark.gpu
def test_gpu_seq_f_gate_table_of_a_smaller_shape(onepass):
    """Sequence F: a workspace in use for (7, 256, 256) takes one codec_pee_gate_capacity call at
    (1, 8, 8).  That call's bins lie behind the SMALL shape's layout, i.e. at bytes 2560-3652,
    which are capacity bins of slices 0-4 of the big shape's layout
    (test_gate_table_of_small_shape_overlaps_big_hist), and the call leaves them non-zero.  The
    call enters the workspace registry like every other workspace-taking call, so the next call
    of the big shape sees a shape change and zeroes the workspace first: capacity, embed and
    extract at the big shape stay exact and the counters stay 0.  (Before codec_pee_gate_capacity
    entered the registry, the capacity pass that followed started from the table's bins and
    returned wrong capacities for the slices under them.)"""
    rig = Rig([BIG_F], slot=7, families=("s1", "cap"), extra=[SMALL_F])
    t = rig.t
    rig.capacity(BIG_F, 0)
    rig.embed(BIG_F, 0)
    small = np.stack([_cover(SMALL_F, 0, 0)])
    n, hs = GS.table(small[0], TMAX, _maxval(SMALL_F))
    assert n.sum() == 16 and hs.sum() > 0            # the table call leaves non-zero bins
    refs = {"cov": t.from_numpy(small).cuda(), "gn": t.from_numpy(n[None].astype(np.int32)).cuda(),
            "ghs": t.from_numpy(hs[None].astype(np.int32)).cuda()}
    rig.gate_capacity(SMALL_F, None, refs=refs)
    rig.capacity(BIG_F, 1)
    rig.embed(BIG_F, 1)
    rig.extract(BIG_F, 1)
    rig.capacity(BIG_F, 2)
    seen = rig.finish()
    steps = [c[2][0] for c in rig.calls]
    assert [st.rezero for st in steps] == [False, False, True, True, False, False, False]
    assert [e for _k, _p, _t, e in seen] == [0, 0, 1]
    assert rig.diagnostics(BIG_F) == ([0, 0, 0, 0], 0)
