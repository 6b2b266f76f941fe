"""ROI-protected MED-PEE on the GPU (include/codec_tcc_roi.h), bit-exact against the
specification tests/pee_roi_spec.py: stego, location map, every record field (the three reserved
words included), payload and restored cover -- on the two-pass kernels (odd shapes, the forced
two-pass routes), the look-back single pass in its flat-slot (B <= 7) and grouped forms with its
fallback recount, in place and out of place; every stego against its cover on the rectangle,
directly; the capacity table and the (T, G) selection under a rectangle; codec_roi_bbox; graph
replay; decode() with no configuration."""
import numpy as np
import pytest

import pee_covers as PC
import pee_gate_spec as G
import pee_roi_spec as R
from codec_tcc_amd import _lib, synth

pytestmark = pytest.mark.gpu

NO_GATE = 65535


def _ct12(B, H, W, seed=300):
    return np.stack([synth.ct12(H, W, seed + i) for i in range(B)])


def _end_rect(cover, T, gate, maxval, H, W):
    """A rectangle around the candidate that is `end` when half the (unprotected) capacity is embedded."""
    cap = G.embed(cover, [], T, gate, maxval)[1]["capacity"]
    end = G.embed(cover, G.payload_bits(cap // 2, 1), T, gate, maxval)[1]["end"]
    y, x = 2 * (end // (W // 2)) + 1, 2 * (end % (W // 2)) + 1
    return max(0, y - 3), max(0, x - 6), min(H, y + 4), min(W, x + 7)


def _rects(covers, Ts, Gs, maxval, shift=0):
    """Per slice, in turn: none; central with odd-coordinate edges; vertical edges strictly inside
    an 8-column item (x0 = 11, x1 = 29) from y0 = 1; one covering the unprotected run's `end`.
    A batch of three slices holds three of the four kinds: `shift` = 1 swaps the central one for
    the `end` one, and every three-slice shape runs both assignments in both placements."""
    B, H, W = covers.shape
    out = []
    for b in range(B):
        kind = b % 4
        if B < 4 and shift and kind == 1:
            kind = 3
        if kind == 0:
            out.append((0, 0, 0, 0))
        elif kind == 1:
            out.append(((H // 4) | 1, (W // 4) | 1, (3 * H // 4) | 1, (3 * W // 4) | 1))
        elif kind == 2:
            out.append((1, 11, min(H, (2 * H // 3) | 1), 29))
        else:
            out.append(_end_rect(covers[b], int(Ts[b]), int(Gs[b]), maxval, H, W))
    return out


def _payloads(covers, Ts, Gs, rects, maxval, rule="mixed"):
    """Per slice: half the capacity outside the rectangle; with "mixed" slice 5 carries nothing and
    the last slice 41 bits more than fit (status 1); "near": `end` in the slice's last chunk."""
    out = []
    B = len(covers)
    for b, c in enumerate(covers):
        cap = R.embed(c, [], int(Ts[b]), int(Gs[b]), rects[b], maxval)[1]["capacity"]
        n = cap // 2
        if rule == "mixed" and b == 5:   # (the nine-slice batches: slice 1 has the same kind of rectangle and embeds)
            n = 0
        if rule == "mixed" and b == B - 1:
            n = cap + 41
        if rule == "near":
            n = max(0, cap - 3)
        out.append(G.payload_bits(n, 10 * b + int(Gs[b]) % 97))
    return out


def _codec(B, H, W, dtype, maxval, Ts, Gs):
    """A gated codec with per-slice T and G; every G == 65535: an ungated codec (no gate asked for)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    if all(int(g) == NO_GATE for g in Gs) and len(set(int(t) for t in Ts)) == 1:
        return PeeCodec(B, H, W, dtype=dtype, T=int(Ts[0]), maxval=maxval)
    codec = PeeCodec(B, H, W, dtype=dtype, T=int(Ts[0]), maxval=maxval, gate=int(Gs[0]))
    codec.t_slices.copy_(torch.tensor([int(t) for t in Ts], dtype=torch.int32))
    codec.g_slices.copy_(torch.tensor([int(g) for g in Gs], dtype=torch.int32))
    return codec


def _untouched(stego, covers, rects):
    """Every stego equals its cover on every pixel of its rectangle (not through the spec)."""
    for b, (y0, x0, y1, x1) in enumerate(rects):
        np.testing.assert_array_equal(stego[b, y0:y1, x0:x1], covers[b, y0:y1, x0:x1], err_msg=f"rectangle of slice {b}")


def _check_enc(enc, covers, bits, Ts, Gs, rects, maxval):
    """Every output of a ROI embed against the spec; returns the spec's (stegos, sides)."""
    from codec_tcc_amd.pee import lm_bits
    recs = enc.records()
    stego = enc.stego.cpu().numpy()
    embedded = enc.embedded()
    _untouched(stego, covers, rects)
    assert enc.roi == [R.normalize(r, *covers.shape[1:]) for r in rects]
    out = []
    for b, c in enumerate(covers):
        st, side = R.embed(c, bits[b], int(Ts[b]), int(Gs[b]), rects[b], maxval)
        r = recs[b]
        nc = (c.shape[0] // 2) * (c.shape[1] // 2)
        got = dict(T=r.T, maxval=r.maxval, end=r.end, status=r.status, nc=r.nc, ntiles=r.ntiles, h=r.h, w=r.w,
                   tile_end=r.tile_end, lm_count=r.lm_count, L=r.L, embedded=embedded[b],
                   reserved=tuple(int(v) & 0xFFFFFFFF for v in r.reserved))
        want = dict(T=side["T"], maxval=side["maxval"], end=side["end"], status=side["status"], nc=nc,
                    ntiles=(nc + 1023) // 1024, h=c.shape[0], w=c.shape[1],
                    tile_end=side["end"] // 1024 if side["end"] >= 0 else -1, lm_count=side["lm_count"],
                    L=len(bits[b]), embedded=side["L"], reserved=side["reserved"])
        assert got == want, (b, got, want)
        if r.flags & _lib.PEE_PARTIAL:   # the look-back pass stopped counting at `end`'s chunk
            assert side["L"] <= r.capacity <= side["capacity"], b
        else:
            assert r.capacity == side["capacity"], b
        np.testing.assert_array_equal(stego[b], st, err_msg=f"stego of slice {b}")
        np.testing.assert_array_equal(lm_bits(enc, b), side["lm"], err_msg=f"map of slice {b}")
        out.append((st, side))
    return out


def _round_trip(covers, Ts, Gs, maxval, *, rects=None, inplace=False, rule="mixed", shift=None, bits=None):
    """bits: the slices' payloads, for a caller that brings its own (else `rule`'s)"""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing
    B, H, W = covers.shape
    rects = _rects(covers, Ts, Gs, maxval, shift=int(inplace) if shift is None else shift) if rects is None else rects
    bits = _payloads(covers, Ts, Gs, rects, maxval, rule) if bits is None else bits
    codec = _codec(B, H, W, str(covers.dtype), maxval, Ts, Gs)
    cov = torch.from_numpy(covers).cuda()
    enc = codec.embed(cov, bits, stego=cov if inplace else None, roi=rects)
    ref = _check_enc(enc, covers, bits, Ts, Gs, rects, maxval)
    # decode: gate and rectangle come from the records (codec_pee_roi_extract), in place or out of place
    words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words,
                                cover=enc.stego if inplace else None, roi=True)
    assert not codec.lookback_failed(enc.payload_words)
    host = words.cpu().numpy()
    for b, (_st, side) in enumerate(ref):
        np.testing.assert_array_equal(framing.unpack_bits(host[b], side["L"]), bits[b][:side["L"]], err_msg=f"payload {b}")
        np.testing.assert_array_equal(framing.unpack_bits(host[b], 64 * enc.payload_words)[side["L"]:], 0)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    return codec, enc, ref, rects


SHAPES = [(3, 37, 53, "uint16"), (3, 64, 96, "uint16"), (3, 64, 96, "uint8"), (3, 130, 512, "uint16"),
          (9, 130, 512, "uint16"), (3, 513, 512, "uint16"), (9, 64, 96, "uint16")]


# a three-slice batch holds three of the four rectangle kinds: it runs with the central one and with the `end` one
SHAPE_KINDS = [(*s, k) for s in SHAPES for k in ((0, 1) if s[0] < 4 else (0,))]


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("B,H,W,dtype,shift", SHAPE_KINDS, ids=lambda v: str(v))
def test_gpu_roi_ct12_matches_spec(B, H, W, dtype, shift, inplace):
    """The gate suite's shapes (37x53: the two-pass scalar kernels; the others the look-back pass,
    B = 3 flat slots, B = 9 grouped; 130x512 five chunks with a ragged last one), each slice with
    another rectangle, under a gate (G = 24; uint8: 96)."""
    if dtype == "uint16":
        covers, maxval, gate = _ct12(B, H, W), 4095, 24
    else:
        covers, maxval, gate = np.stack([synth.GENERATORS["u8"](H, W, 40 + i) for i in range(B)]), 255, 96
    _codec_, _enc, ref, rects = _round_trip(covers, [2] * B, [gate] * B, maxval, inplace=inplace, shift=shift)
    # the rectangle over `end` moved `end` (or the test shows nothing)
    b = 3 if B > 3 else (1 if shift else None)
    if b is not None:
        free = G.embed(covers[b], G.payload_bits(G.embed(covers[b], [], 2, gate, maxval)[1]["capacity"] // 2, 1), 2, gate, maxval)
        assert R.protected(H, W, rects[b]).ravel()[free[1]["end"]]


@pytest.mark.parametrize("B,H,W", [(3, 130, 512), (4, 37, 53)])
def test_gpu_roi_without_a_gate(B, H, W):
    """No gate asked for (an ungated codec): G = 65535, reserved[1] = 65536."""
    _round_trip(_ct12(B, H, W, 420), [2] * B, [NO_GATE] * B, 4095)
    _round_trip(_ct12(B, H, W, 430), [3] * B, [NO_GATE] * B, 4095, inplace=True, rule="half")


@pytest.mark.parametrize("B,H,W", [(3, 130, 512), (3, 37, 53)])
def test_gpu_roi_empty_rectangles_are_the_gated_and_the_ungated_call(B, H, W):
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    covers = _ct12(B, H, W, 350)
    none = [(0, 0, 0, 0)] * B
    bits = _payloads(covers, [2] * B, [NO_GATE] * B, none, 4095)
    cov = torch.from_numpy(covers).cuda()
    plain = PeeCodec(B, H, W, T=2, maxval=4095)
    e0 = plain.embed(cov, bits)                                          # codec_pee_embed_ts
    e1 = plain.embed(cov, bits, roi=(0, 0, 0, 0))                        # codec_pee_roi_embed, no gate asked for
    e2 = plain.embed(cov, bits, roi=[(5, 9, 5, 40)] * B)                 # empty rectangles normalise
    gated = PeeCodec(B, H, W, T=2, maxval=4095, gate=24)
    g0, g1 = gated.embed(cov, bits), gated.embed(cov, bits, roi=(0, 0, 0, 0))
    for a, b_, word in ((e0, e1, 65536), (e0, e2, 65536), (g0, g1, None)):
        assert torch.equal(a.stego, b_.stego)
        for b, (r0, r1) in enumerate(zip(a.records(), b_.records())):
            assert (r1.reserved[0], r1.reserved[2]) == (0, 0)
            if word is not None:
                assert r1.reserved[1] == word and r0.reserved[1] == 0
                r1.reserved[1] = 0
            if (r0.flags | r1.flags) & _lib.PEE_PARTIAL:
                r0.capacity = r1.capacity = 0
            assert bytes(r0) == bytes(r1), b
            assert (r0.L, r0.end) == (r1.L, r1.end)
            n = (r0.end + 64) // 64
            assert torch.equal(a.lm[b, :n], b_.lm[b, :n])


@pytest.mark.parametrize("H,W,dtype,maxval", [(64, 96, "uint16", 4095), (64, 64, "uint8", None)], ids=lambda v: str(v))
def test_gpu_roi_adversarial_covers(H, W, dtype, maxval):
    """The pee_covers batch (8 slices: the grouped look-back order) with a rectangle that cuts the
    saturated band (top_band, above) and the range-end fields: the map bits of protected unsafe
    candidates are 0."""
    from codec_tcc_amd.pee import lm_bits
    covers = PC.batch(H, W, dtype, maxval, 2, 3)
    B = len(covers)
    rect = (H // 8 + 1, W // 4 + 1, H // 2 + 3, W // 2 + 8)
    for gate in (NO_GATE, 16):
        _codec_, enc, ref, rects = _round_trip(covers, [2] * B, [gate] * B, maxval, rects=[rect] * B)
        prot = R.protected(H, W, rect).ravel()
        unsafe_inside = 0
        for b in range(B):
            _st, free = G.embed(covers[b], G.payload_bits(10 ** 6, b), 2, gate, maxval)   # every unsafe active candidate
            lm = lm_bits(enc, b)
            assert not lm[prot[:len(lm)]].any(), b
            unsafe_inside += int(free["lm"][prot].sum())
        assert unsafe_inside > 0      # the rectangle does hold unsafe candidates
        _round_trip(covers, [2] * B, [gate] * B, maxval, rects=[rect] * B, inplace=True, rule="half")


@pytest.mark.parametrize("knobs", [{"CODEC_PEE_ONEPASS": "0"}, {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_FUSED": "0"},
                                   {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_EMBED_V": "0", "CODEC_PEE_WAVE_TILES": "0"}],
                         ids=["scan-embed_v-restore", "copy-dcount-recover", "embed-dcount"])
def test_gpu_roi_two_pass_vector_routes(knobs, monkeypatch):
    """The aligned two-pass kernels behind their A/B knobs, as test_gpu_gate_two_pass_vector_routes."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _round_trip(_ct12(4, 128, 512, 340), [2, 1, 3, 2], [24, 24, 12, NO_GATE], 4095)     # 256 | items: the fused restore
    _round_trip(_ct12(4, 130, 96, 343), [2, 1, 3, 2], [24, 24, 12, NO_GATE], 4095)


@pytest.mark.parametrize("slots", ["flat", "lanes"])
def test_gpu_roi_lookback_fallback(slots, monkeypatch):
    """A chunk that never publishes its look-back word: its successors recount it from the pixels
    (EmbedCount / ExtractCount) -- with the rectangle, or the cursor would be the gated one."""
    monkeypatch.setenv("CODEC_DEBUG", "1")
    monkeypatch.setenv("CODEC_PEE_ONEPASS", "1")
    monkeypatch.setenv("CODEC_PEE_DEBUG_SKIP", "2")
    monkeypatch.setenv("CODEC_PEE_LB_SPINS", "256")
    if slots == "lanes":
        monkeypatch.setenv("CODEC_PEE_FLAT_MAXB", "0")
    covers = _ct12(3, 256, 256, 500)          # 4 chunks per slice; `end` in the last one
    rects = [(35, 21, 141, 199)] * 3          # reaches into chunks 0..2 (32 row pairs per chunk): the skipped chunk 1 too
    codec, enc, ref, _r = _round_trip(covers, [2] * 3, [24] * 3, 4095, rects=rects, rule="near")
    assert all(side["end"] >= 3 * 1024 * 4 for _st, side in ref)
    d = codec.diagnostics()
    assert d["embed_fallback_chunks"] >= 1 and d["extract_fallback_chunks"] >= 1
    assert d["embed_unrecovered_chunks"] == 0 == d["extract_unrecovered_chunks"]
    # the gated cursor differs here: the recount honours the rectangle or the results above were not exact
    assert G.embed(covers[0], [], 2, 24, 4095)[1]["capacity"] != ref[0][1]["capacity"]


def test_gpu_roi_table_and_selection_match_spec():
    """The table under rectangles on both routes of both pixel types: W % 8 == 0 (130x512, 64x96,
    16x24) and not (37x53, 16x20), and every batch again as a view one pixel into its buffer (no
    vector alignment: the scalar route whatever W is)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    u8 = [np.stack([synth.GENERATORS["u8"](16, w, 440 + i) for i in range(2)]) for w in (24, 20)]
    for covers, maxval in ((_ct12(4, 130, 512, 360), 4095), (_ct12(4, 37, 53, 363), 4095),
                           (PC.batch(64, 96, "uint16", 4095, 2, 3), 4095), (u8[0], 255), (u8[1], 255)):
        B, H, W = covers.shape
        rects = _rects(covers, [2] * B, [NO_GATE] * B, maxval)
        codec = PeeCodec(B, H, W, dtype=str(covers.dtype), T=2, tmax=16, maxval=maxval)       # no gate: _table_workspace
        cov = torch.from_numpy(covers).cuda()
        flat = torch.empty(B * H * W + 1, dtype=cov.dtype, device="cuda")
        off = flat[1:].view(B, H, W)
        off.copy_(cov)
        n, hs = codec.gate_table(cov, roi=rects)
        n_off, hs_off = codec.gate_table(off, roi=rects)
        assert torch.equal(n, n_off) and torch.equal(hs, hs_off)
        n, hs = n.cpu().numpy(), hs.cpu().numpy()
        for b, c in enumerate(covers):
            sn, sh = R.table(c, 16, rects[b], maxval)
            np.testing.assert_array_equal(n[b], sn, err_msg=f"n of slice {b}")
            np.testing.assert_array_equal(hs[b], sh, err_msg=f"hs of slice {b}")
        for gate in (None, 5):
            caps = codec.capacity(cov, gate=gate, roi=rects).cpu().numpy()
            for b, c in enumerate(covers):
                want = [R.embed(c, [], T, NO_GATE if gate is None else gate, rects[b], maxval)[1]["capacity"] for T in (1, 2, 16)]
                assert [int(caps[b, 0]), int(caps[b, 1]), int(caps[b, 15])] == want, (gate, b)


@pytest.mark.parametrize("T,gate", [("auto", "auto"), (2, "auto"), ("auto", 24), ("auto", None)])
def test_gpu_roi_auto_embeds_the_specs_choice(T, gate):
    """T="auto", gate="auto" and both embed the spec's choice under the rectangles; a rectangle
    that removes enough capacity moves the chosen T up (the payload is picked from the spec's
    capacities so that it does)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    B, H, W = 4, 130, 512
    covers = _ct12(B, H, W, 370)
    rects = [(0, 0, 0, 0), (1, 1, 111, 481), (1, 11, 87, 29), (33, 65, 97, 449)]
    gfix = NO_GATE if gate in (None, "auto") else gate
    # slice 1: more bits than fit at T = 1 beside the rectangle, fewer than fit at T = 1 without it
    lo = R.embed(covers[1], [], 1, gfix, rects[1], 4095)[1]["capacity"]
    hi = G.embed(covers[1], [], 1, gfix, 4095)[1]["capacity"]
    assert lo + 8 < hi
    # (a fixed T = 2 holds under 1 000 bits of these slices, the gate 24 under 2 500 at any T)
    lengths = [500, lo + 8, 0, 200 if T != "auto" else (2000 if gate == 24 else 3000)]
    bits = [G.payload_bits(n, 3 + i) for i, n in enumerate(lengths)]
    codec = PeeCodec(B, H, W, T=T, tmax=16, maxval=4095, gate=gate)
    picks = [R.choose(c, L, 16, rects[b], 4095, T=None if T == "auto" else T, gate=None if gate == "auto" else gfix)
             for b, (c, L) in enumerate(zip(covers, lengths))]
    free = [R.choose(c, L, 16, None, 4095, T=None if T == "auto" else T, gate=None if gate == "auto" else gfix)
            for c, L in zip(covers, lengths)]
    Ts, Gs = [p[0] for p in picks], [p[1] for p in picks]
    if T == "auto" and gate != "auto":
        assert Ts[1] > free[1][0]            # the rectangle moved slice 1's T up
    enc = codec.embed(torch.from_numpy(covers).cuda(), bits, roi=rects)
    ts, gs = codec._roi_slices()
    assert ts.cpu().tolist() == Ts and gs.cpu().tolist() == Gs
    _check_enc(enc, covers, bits, Ts, Gs, rects, 4095)
    got, back = codec.decode(enc)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    for b in range(B):
        np.testing.assert_array_equal(got[b], bits[b])


def _bbox_oracle(img, level, margin):
    H, W = img.shape
    ys, xs = np.nonzero(img > level)
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [max(int(ys.min()) - margin, 0), max(int(xs.min()) - margin, 0), min(int(ys.max()) + 1 + margin, H),
            min(int(xs.max()) + 1 + margin, W)]


@pytest.mark.parametrize("view", ["contiguous", "offset"])
@pytest.mark.parametrize("H,W,dtype", [(37, 53, "uint8"), (37, 53, "uint16"), (130, 512, "uint8"), (130, 512, "uint16")],
                         ids=lambda v: str(v))
def test_gpu_roi_bbox(H, W, dtype, view):
    """codec_roi_bbox against np.nonzero min / max: an empty mask, one pixel in each corner, a full
    mask, margins clamped at every border, level 0 and maxval - 1, a slice whose only set pixel
    is its last element; 16-byte loads (130x512 contiguous) and scalar loads (37x53, offset views)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.roi import roi_bbox
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(H + W)
    imgs = []
    imgs.append(np.zeros((H, W), dtype))                                        # 0: empty
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):               # 1..4: the corners (4: the last element)
        a = np.zeros((H, W), dtype)
        a[y, x] = top
        imgs.append(a)
    imgs.append(np.full((H, W), top, dtype))                                    # 5: full
    a = np.zeros((H, W), dtype)
    a[H // 3: H // 2, W // 5: W // 2] = rng.integers(1, top + 1, (H // 2 - H // 3, W // 2 - W // 5))
    imgs.append(a)                                                              # 6: a blob
    a = rng.integers(0, top, (H, W)).astype(dtype)                              # 7: noise below top, three pixels at top
    a[5, 7] = a[H - 4, W - 9] = a[H // 2, 3] = top
    imgs.append(a)
    a = np.zeros((H, W), dtype)
    a[2, W - 2] = a[H - 3, 1] = 1                                               # 8: near every border (margin clamps)
    imgs.append(a)
    stack = np.stack(imgs)
    B = len(stack)
    if view == "offset":   # one pixel into its buffer: no 16-byte alignment
        flat = torch.zeros(B * H * W + 1, dtype=getattr(torch, dtype), device="cuda")
        dev = flat[1:].view(B, H, W)
        dev.copy_(torch.from_numpy(stack).cuda())
    else:
        dev = torch.from_numpy(stack).cuda()
    for level, margin in ((0, 0), (0, 3), (top - 1, 0), (top - 1, 5), (0, 65535)):
        got = roi_bbox(dev, level=level, margin=margin).cpu().numpy().tolist()
        want = [_bbox_oracle(img, level, margin) for img in stack]
        assert got == want, (level, margin)
    assert roi_bbox(dev[4]).cpu().numpy().tolist() == [[H - 1, W - 1, H, W]]      # a 2-D image; the last element alone
    with pytest.raises(ValueError):
        roi_bbox(dev, level=-1)
    with pytest.raises(ValueError):
        roi_bbox(dev, margin=-1)
    with pytest.raises(ValueError):
        roi_bbox(dev[:, ::2])


def test_gpu_roi_bbox_feeds_embed():
    """roi_bbox's device tensor goes into embed(roi=) as it comes."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    from codec_tcc_amd.roi import roi_bbox
    covers = _ct12(3, 64, 96, 440)
    mask = np.zeros_like(covers)
    mask[0, 20:40, 30:50] = 1
    mask[2, 5:9, 60:90] = 7
    rois = roi_bbox(torch.from_numpy(mask).cuda(), margin=2)
    assert rois.cpu().tolist() == [[18, 28, 42, 52], [0, 0, 0, 0], [3, 58, 11, 92]]
    codec = PeeCodec(3, 64, 96, T=2, maxval=4095)
    bits = [G.payload_bits(100, i) for i in range(3)]
    enc = codec.embed(torch.from_numpy(covers).cuda(), bits, roi=rois)
    _check_enc(enc, covers, bits, [2] * 3, [NO_GATE] * 3, rois.cpu().tolist(), 4095)


def test_gpu_roi_graph_replay():
    """A ROI embed (table + selection + embed) and the ROI extract captured once and replayed on
    refreshed covers equal the eager calls and the spec."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import graphs
    from codec_tcc_amd.pee import PeeCodec
    B, H, W = 3, 130, 512
    codec = PeeCodec(B, H, W, T="auto", maxval=4095, gate="auto")
    rects = [(0, 0, 0, 0), (33, 65, 97, 449), (1, 11, 87, 29)]
    roi = codec.pack_roi(rects)
    cov = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    packed = codec.pack_payloads([G.payload_bits(n, n) for n in (300, 2000, 0)])
    stego, cov2 = torch.empty_like(cov), torch.empty_like(cov)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device="cuda")
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device="cuda")
    pw = packed[0].shape[1]
    outw = torch.empty((B, pw), dtype=torch.int64, device="cuda")

    def step():
        codec.embed(cov, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False, roi=roi)
        codec.extract(stego, meta, lm, payload_words=pw, cover=cov2, payload=outw, roi=True)

    cov.copy_(torch.from_numpy(_ct12(B, H, W, 500)).cuda())
    g = graphs.capture(step)
    for seed in (600, 700):
        host = _ct12(B, H, W, seed)
        cov.copy_(torch.from_numpy(host).cuda())
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (stego, meta, outw, cov2, codec.t_slices, codec.g_slices)]
        enc = codec.embed(torch.from_numpy(host).cuda(), None, packed=packed, roi=roi)
        words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=pw, roi=True)
        for a, b in zip(got, (enc.stego, enc.meta, words, back, codec.t_slices, codec.g_slices)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        np.testing.assert_array_equal(got[3].cpu().numpy(), host)
        _untouched(got[0].cpu().numpy(), host, rects)
        st, _side = R.embed(host[1], G.payload_bits(2000, 2000), int(got[4][1]), int(got[5][1]), rects[1], 4095)
        np.testing.assert_array_equal(got[0][1].cpu().numpy(), st)


def test_gpu_roi_package_level_encode_decode():
    """encode(..., method="pee", roi=) and decode() with no configuration: the rectangle and the
    gate are the records'.  checksum=True composes; "tiles" needs its tile; scheme 2 and volumes refuse."""
    torch = pytest.importorskip("torch")
    import codec_tcc_amd as ct
    from codec_tcc_amd import pee
    from codec_tcc_amd.pee import PeeCodec, PeeEncoded
    covers = _ct12(3, 64, 96, 450)
    rects = [(9, 11, 41, 61), (0, 0, 0, 0), (1, 11, 33, 29)]
    bits = [G.payload_bits(60, i) for i in range(3)]       # these slices hold 71 bits or more at T = 2 beside the rectangles
    enc = ct.encode(covers, bits, method="pee", T=2, maxval=4095, roi=rects)
    assert enc.roi == rects
    _untouched(enc.stego.cpu().numpy(), covers, rects)
    for b in range(3):
        st, side = R.embed(covers[b], bits[b], 2, NO_GATE, rects[b], 4095)
        np.testing.assert_array_equal(enc.stego[b].cpu().numpy(), st)
    bare = PeeEncoded(stego=enc.stego, lm=enc.lm, meta=enc.meta, lengths=enc.lengths, payload_words=enc.payload_words)
    for e in (enc, bare):
        got, back = ct.decode(e)
        np.testing.assert_array_equal(back.cpu().numpy(), covers)
        for b in range(3):
            np.testing.assert_array_equal(got[b], bits[b])
    e1 = pee.encode(covers, bits, T=2, maxval=4095, roi=rects, checksum=True)     # the CRCs are the covers'
    assert e1.cover_crc is not None and torch.equal(e1.stego, enc.stego)
    assert pee.decode(e1, verify="require")[1].cpu().numpy().tolist() == covers.tolist()
    e2 = pee.encode(covers, bits, T=2, maxval=4095, roi=(9, 11, 41, 61), checksum="tiles", tile=16)
    assert e2.tile == (16, 16) and pee.decode(e2, verify="require")[1].cpu().numpy().tolist() == covers.tolist()
    with pytest.raises(ValueError, match="tile"):
        pee.encode(covers, bits, T=2, maxval=4095, roi=rects, checksum="tiles")
    with pytest.raises(ValueError, match="scheme 1"):
        ct.encode(covers, bits, method="pee", T=2, maxval=4095, roi=rects, scheme=2)
    with pytest.raises(ValueError, match="slice 2: x1 = 97"):
        ct.encode(covers, bits, method="pee", T=2, maxval=4095, roi=[(0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 4, 97)])
    codec = PeeCodec(3, 64, 96, T="auto", maxval=4095)
    with pytest.raises(ValueError, match="region of interest"):
        codec.embed_volume(torch.from_numpy(covers).cuda(), b"abc", roi=rects)


@pytest.mark.parametrize("B,H,W", [(5, 130, 512), (40, 64, 96), (3, 37, 53)])
def test_gpu_roi_one_rectangle_for_every_slice(B, H, W):
    """roi=(y0, x0, y1, x1): the same rectangle on every slice (flat and grouped slots, the two-pass
    kernels) -- every record carries it and every slice keeps it untouched."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    covers = _ct12(B, H, W, 460)
    rect = (H // 4 + 1, W // 4, 3 * H // 4, 3 * W // 4 + 1)
    codec = PeeCodec(B, H, W, T=2, maxval=4095, gate=24)
    bits = _payloads(covers, [2] * B, [24] * B, [rect] * B, 4095)
    enc = codec.embed(torch.from_numpy(covers).cuda(), bits, roi=rect)
    assert enc.roi == [rect] * B
    _check_enc(enc, covers, bits, [2] * B, [24] * B, [rect] * B, 4095)
    assert codec.capacity(torch.from_numpy(covers).cuda(), gate=24, roi=rect)[:, 1].cpu().tolist() == \
        [R.embed(c, [], 2, 24, rect, 4095)[1]["capacity"] for c in covers]


@pytest.mark.parametrize("checksum", [False, True])
def test_gpu_roi_file_round_trip(tmp_path, checksum):
    """encode_file_pee(..., roi=) writes scheme byte 4; decode_bin_pee reads it back exactly; the
    other parsers refuse it; a file without roi= is byte for byte what it was."""
    import os
    from codec_tcc_amd import container, pipeline
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images.npz"))
    img, maxval = z["pe"], 4095
    rect = (129, 101, 385, 411)
    bits = G.payload_bits(8192, 5)
    for gate, T in ((None, 2), ("auto", "auto")):
        path = str(tmp_path / f"roi_{gate}.stgc")
        info = pipeline.encode_file_pee(img, bits, path, T=T, maxval=maxval, gate=gate, roi=rect, checksum=checksum)
        raw = open(path, "rb").read()
        assert container.pee_scheme(raw) == 4 and info["scheme"] == 4 and info["roi"] == rect and info["status"] == 0
        if gate is None:
            Tw, Gw = 2, NO_GATE
        else:
            Tw, Gw = R.choose(img, 8192, 16, rect, maxval)
        assert (info["T"], info["gate"]) == (Tw, Gw)
        st, side = R.embed(img, bits, Tw, Gw, rect, maxval)
        np.testing.assert_array_equal(info["stego"], st)
        np.testing.assert_array_equal(info["stego"][129:385, 101:411], img[129:385, 101:411])
        md, _blob, _data = container.parse_pee_roi_bytes(raw)
        assert (md["roi"], md["gate"], md["T"], md["L"], md["end"]) == (rect, Gw, Tw, 8192, side["end"])
        assert ("cover_crc32" in md) == checksum
        got, back = pipeline.decode_bin_pee(path, verify="require" if checksum else True)
        np.testing.assert_array_equal(got, bits)
        np.testing.assert_array_equal(back, img)
        for parse in (container.parse_pee_bytes, container.parse_pee_gate_bytes):
            with pytest.raises(ValueError, match="scheme byte 4"):
                parse(raw)
    p0, p1 = str(tmp_path / "plain.stgc"), str(tmp_path / "empty.stgc")
    pipeline.encode_file_pee(img, bits, p0, T=2, maxval=maxval, checksum=checksum)
    pipeline.encode_file_pee(img, bits, p1, T=2, maxval=maxval, checksum=checksum, roi=(7, 9, 7, 300))   # empty: no ROI
    assert open(p0, "rb").read() == open(p1, "rb").read() and open(p0, "rb").read()[11] == 0
    with pytest.raises(ValueError, match="slice 0: y1 = 513"):
        pipeline.encode_file_pee(img, bits, p1, T=2, maxval=maxval, roi=(0, 0, 513, 8))
