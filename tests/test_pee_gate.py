"""Smoothness-gated MED-PEE on the GPU (include/codec_tcc_gate.h), bit-exact against the
specification tests/pee_gate_spec.py: stego, location map, every record field (reserved[1] = G + 1
included), payload and restored cover -- on the two-pass kernels (odd shapes, unaligned views,
the forced two-pass routes), the look-back single pass in its flat-slot (B <= 7) and grouped
forms with its fallback recount, in place and out of place; the capacity table and the
(T, G) selection; graph replay; the quality gain on the reference's images; files."""
import os

import numpy as np
import pytest

import pee_covers as PC
import pee_gate_spec as G
from codec_tcc_amd import _lib, synth
from oracle import pee_cpu as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def _images():
    if "img" not in _CACHE:
        z = np.load(os.path.join(HERE, "golden", "images.npz"))
        _CACHE["img"] = {"pe": (z["pe"], 4095), "torax": (z["torax"], 255)}
    return _CACHE["img"]


def _ct12(B, H, W, seed=300):
    return np.stack([synth.ct12(H, W, seed + i) for i in range(B)])


def _payloads(covers, Ts, Gs, maxval, rule="mixed"):
    """Per slice: half the gated capacity; with "mixed" slice 1 carries nothing and the last
    slice 41 bits more than fit (status 1)."""
    out = []
    B = len(covers)
    for b, c in enumerate(covers):
        cap = G.embed(c, [], int(Ts[b]), int(Gs[b]), maxval)[1]["capacity"]
        n = cap // 2
        if rule == "mixed" and b == 1 and B > 2:
            n = 0
        if rule == "mixed" and b == B - 1:
            n = cap + 41
        if rule == "near":   # `end` in the slice's last chunk
            n = max(0, cap - 3)
        out.append(G.payload_bits(n, 10 * b + int(Gs[b])))
    return out


def _gated_codec(B, H, W, dtype, maxval, Ts, Gs):
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    codec = PeeCodec(B, H, W, dtype=dtype, T=int(Ts[0]), maxval=maxval, gate=int(Gs[0]))
    codec.t_slices.copy_(torch.tensor([int(t) for t in Ts], dtype=torch.int32))
    codec.g_slices.copy_(torch.tensor([int(g) for g in Gs], dtype=torch.int32))
    return codec


def _check_enc(enc, covers, bits, Ts, Gs, maxval, sides=None):
    """Every output of a gated embed against the spec; returns the spec's (stegos, sides)."""
    from codec_tcc_amd.pee import lm_bits
    recs = enc.records()
    stego = enc.stego.cpu().numpy()
    embedded = enc.embedded()
    out = []
    for b, c in enumerate(covers):
        st, side = G.embed(c, bits[b], int(Ts[b]), int(Gs[b]), maxval)
        r = recs[b]
        nc = (c.shape[0] // 2) * (c.shape[1] // 2)
        got = dict(T=r.T, maxval=r.maxval, end=r.end, status=r.status, nc=r.nc, ntiles=r.ntiles, h=r.h, w=r.w,
                   tile_end=r.tile_end, lm_count=r.lm_count, gate=r.reserved[1], r0=r.reserved[0], r2=r.reserved[2],
                   L=r.L, embedded=embedded[b])
        want = dict(T=side["T"], maxval=side["maxval"], end=side["end"], status=side["status"], nc=nc,
                    ntiles=(nc + 1023) // 1024, h=c.shape[0], w=c.shape[1],
                    tile_end=side["end"] // 1024 if side["end"] >= 0 else -1, lm_count=side["lm_count"],
                    gate=int(Gs[b]) + 1, r0=0, r2=0, L=len(bits[b]), embedded=side["L"])
        assert got == want, (b, got, want)
        if r.flags & _lib.PEE_PARTIAL:   # the look-back pass stopped counting at `end`'s chunk
            assert side["L"] <= r.capacity <= side["capacity"], b
        else:
            assert r.capacity == side["capacity"], b
        np.testing.assert_array_equal(stego[b], st, err_msg=f"stego of slice {b}")
        np.testing.assert_array_equal(lm_bits(enc, b), side["lm"], err_msg=f"map of slice {b}")
        out.append((st, side))
    return out


def _round_trip(covers, Ts, Gs, maxval, *, inplace=False, rule="mixed", decode_codec=None, unaligned=False, bits=None):
    """bits: the slices' payloads, for a caller that brings its own (else `rule`'s)"""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import framing
    B, H, W = covers.shape
    dtype = str(covers.dtype)
    bits = _payloads(covers, Ts, Gs, maxval, rule) if bits is None else bits
    codec = _gated_codec(B, H, W, dtype, maxval, Ts, Gs)
    if unaligned:   # a view one pixel into its buffer: no 16-byte alignment, the scalar kernels
        flat = torch.empty(B * H * W + 1, dtype=getattr(torch, dtype), device="cuda")
        cov = flat[1:].view(B, H, W)
        cov.copy_(torch.from_numpy(covers).cuda())
        flat2 = torch.empty(B * H * W + 1, dtype=getattr(torch, dtype), device="cuda")
        stego = cov if inplace else flat2[1:].view(B, H, W)
    else:
        cov = torch.from_numpy(covers).cuda()
        stego = cov if inplace else None
    enc = codec.embed(cov, bits, stego=stego)
    ref = _check_enc(enc, covers, bits, Ts, Gs, maxval)
    # decode: the gate comes from the records (codec_pee_gate_extract), in place or out of place
    words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words,
                                cover=enc.stego if inplace else None)
    assert not codec.lookback_failed(enc.payload_words)
    host = words.cpu().numpy()
    for b, (_st, side) in enumerate(ref):
        np.testing.assert_array_equal(framing.unpack_bits(host[b], side["L"]), bits[b][:side["L"]], err_msg=f"payload {b}")
        # bits past L are zero in the row
        np.testing.assert_array_equal(framing.unpack_bits(host[b], 64 * enc.payload_words)[side["L"]:], 0)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    return codec, enc, ref


SHAPES = [(3, 37, 53, "uint16"), (3, 64, 96, "uint16"), (3, 64, 96, "uint8"), (3, 130, 512, "uint16"),
          (9, 130, 512, "uint16"), (3, 513, 512, "uint16"), (9, 64, 96, "uint16")]


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("B,H,W,dtype", SHAPES, ids=lambda v: str(v))
def test_gpu_gate_ct12_matches_spec(B, H, W, dtype, inplace):
    """ct12 at G = 24 (uint8: the u8 generator at G = 96): 37x53 runs the two-pass scalar
    kernels, the others the look-back pass -- B = 3 flat slots, B = 9 the grouped order; 130x512
    is five chunks with a ragged last one."""
    if dtype == "uint16":
        covers, maxval, gate = _ct12(B, H, W), 4095, 24
        for c in covers:
            assert 0.2 <= G.active_fraction(c, gate) <= 0.8
    else:
        covers, maxval, gate = np.stack([synth.GENERATORS["u8"](H, W, 40 + i) for i in range(B)]), None, 96
    _round_trip(covers, [2] * B, [gate] * B, maxval, inplace=inplace)


@pytest.mark.parametrize("name,gate", [("pe", 3), ("torax", 8)])
@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
def test_gpu_gate_reference_images_match_spec(name, gate, inplace):
    img, maxval = _images()[name]
    assert 0.2 <= G.active_fraction(img, gate) <= 0.8
    covers = np.stack([img, img[::-1].copy(), img[:, ::-1].copy()])
    _round_trip(covers, [1, 2, 3], [gate] * 3, maxval, inplace=inplace)


@pytest.mark.parametrize("gate", [0, 2, 16])
@pytest.mark.parametrize("H,W,dtype,maxval", [(64, 96, "uint16", 4095), (37, 53, "uint16", 4095), (64, 64, "uint8", None),
                                              (130, 512, "uint16", None)],
                         ids=lambda v: str(v))
def test_gpu_gate_adversarial_covers(H, W, dtype, maxval, gate):
    """The whole pee_covers batch (8 slices: the grouped look-back order): all-inactive slices
    (checker at any small gate), all-active ones (the flat covers) and pixels above maxval."""
    covers = PC.batch(H, W, dtype, maxval, 2, 3)
    fr = [G.active_fraction(c, gate) for c in covers]
    assert min(fr) == 0.0 and max(fr) == 1.0
    _round_trip(covers, [2] * len(covers), [gate] * len(covers), maxval)
    _round_trip(covers, [2] * len(covers), [gate] * len(covers), maxval, inplace=True, rule="half")


def test_gpu_gate_mixed_per_slice_T_and_G():
    covers = _ct12(5, 130, 512, 320)
    Ts, Gs = [1, 2, 3, 5, 16], [24, 0, 65535, 7, 100]
    _round_trip(covers, Ts, Gs, 4095)
    _round_trip(covers[:, :37, :53].copy(), Ts, Gs, 4095)


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
def test_gpu_gate_unaligned_view(inplace):
    _round_trip(_ct12(3, 64, 96, 330), [2, 2, 3], [24, 48, 24], 4095, inplace=inplace, unaligned=True)


@pytest.mark.parametrize("knobs", [{"CODEC_PEE_ONEPASS": "0"}, {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_FUSED": "0"},
                                   {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_EMBED_V": "0", "CODEC_PEE_WAVE_TILES": "0"}],
                         ids=["scan-embed_v-restore", "copy-dcount-recover", "embed-dcount"])
def test_gpu_gate_two_pass_vector_routes(knobs, monkeypatch):
    """The aligned two-pass kernels (k_pee_scan, k_pee_embed_v / k_pee_embed, k_pee_dcount_w /
    k_pee_dcount, k_pee_restore_gs / k_pee_recover) behind their A/B knobs."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _round_trip(_ct12(3, 128, 512, 340), [2, 1, 3], [24, 24, 12], 4095)     # 256 | items: the fused restore
    _round_trip(_ct12(3, 130, 96, 343), [2, 1, 3], [24, 24, 12], 4095)


@pytest.mark.parametrize("slots", ["flat", "lanes"])
def test_gpu_gate_lookback_fallback(slots, monkeypatch):
    """A chunk that never publishes its look-back word: its successors recount it from the
    pixels (EmbedCount / ExtractCount) -- with the gate, or the cursor would be the ungated one."""
    monkeypatch.setenv("CODEC_DEBUG", "1")
    monkeypatch.setenv("CODEC_PEE_ONEPASS", "1")
    monkeypatch.setenv("CODEC_PEE_DEBUG_SKIP", "2")
    monkeypatch.setenv("CODEC_PEE_LB_SPINS", "256")
    if slots == "lanes":
        monkeypatch.setenv("CODEC_PEE_FLAT_MAXB", "0")
    covers = _ct12(3, 256, 256, 500)          # 4 chunks per slice; `end` in the last one
    codec, enc, ref = _round_trip(covers, [2] * 3, [24] * 3, 4095, rule="near")
    assert all(side["end"] >= 3 * 1024 * 4 for _st, side in ref)
    d = codec.diagnostics()
    assert d["embed_fallback_chunks"] >= 1 and d["extract_fallback_chunks"] >= 1
    assert d["embed_unrecovered_chunks"] == 0 == d["extract_unrecovered_chunks"]
    # the ungated cursor differs here: the recount is gated or the results above were not exact
    assert P.capacity(covers[0], 2) != ref[0][1]["capacity"]


@pytest.mark.parametrize("B,H,W", [(3, 130, 512), (9, 64, 96), (3, 37, 53)])
def test_gpu_gate_65535_is_the_ungated_call(B, H, W):
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    covers = _ct12(B, H, W, 350)
    bits = _payloads(covers, [2] * B, [65535] * B, 4095)
    cov = torch.from_numpy(covers).cuda()
    plain = PeeCodec(B, H, W, T=2, maxval=4095)
    gated = PeeCodec(B, H, W, T=2, maxval=4095, gate=65535)
    e0, e1 = plain.embed(cov, bits), gated.embed(cov, bits)
    assert torch.equal(e0.stego, e1.stego)
    for b, (r0, r1) in enumerate(zip(e0.records(), e1.records())):
        assert r1.reserved[1] == 65536 and r0.reserved[1] == 0
        r1.reserved[1] = 0
        if (r0.flags | r1.flags) & _lib.PEE_PARTIAL:   # capacity: a lower bound on the look-back pass
            r0.capacity = r1.capacity = 0
        assert bytes(r0) == bytes(r1), b
        n = (r0.end + 64) // 64
        assert torch.equal(e0.lm[b, :n], e1.lm[b, :n])
    w0, c0 = plain.extract(e0.stego, e0.meta, e0.lm, payload_words=e0.payload_words)
    w1, c1 = gated.extract(e1.stego, e1.meta, e1.lm, payload_words=e1.payload_words)
    assert torch.equal(w0, w1) and torch.equal(c0, c1) and torch.equal(c1, cov)
    # an ungated record through the gated extract, and a gated one decoded by an ungated codec
    w2, c2 = gated.extract(e0.stego, e0.meta, e0.lm, payload_words=e0.payload_words)
    assert torch.equal(w0, w2) and torch.equal(c2, cov)
    half = _payloads(covers, [2] * B, [65535] * B, 4095, "half")   # decode() refuses an overflowed slice
    b3, c3 = plain.decode(gated.embed(cov, half))
    assert torch.equal(c3, cov) and all(np.array_equal(b3[i], half[i]) for i in range(B))


def _table_cases():
    pe, torax = _images()["pe"][0], _images()["torax"][0]
    return [(_ct12(3, 130, 512, 360), 4095), (_ct12(3, 37, 53, 363), 4095), (np.stack([pe, pe[::-1].copy()]), 4095),
            (np.stack([torax, torax[:, ::-1].copy()]), 255), (PC.batch(64, 96, "uint16", 4095, 2, 3), 4095),
            (PC.batch(37, 53, "uint8", None, 2, 5), None)]


@pytest.mark.parametrize("case", range(6))
def test_gpu_gate_table_and_selection_match_spec(case):
    """n, hs, the capacities under a gate, and the chosen (T, G, K) for a range of payloads, a
    fixed T, and a fixed gate -- against the spec's table() / select()."""
    torch = pytest.importorskip("torch")
    import ctypes as C
    from codec_tcc_amd.pee import PeeCodec
    covers, maxval = _table_cases()[case]
    B, H, W = covers.shape
    tmax = 16
    codec = PeeCodec(B, H, W, dtype=str(covers.dtype), T="auto", tmax=tmax, maxval=maxval, gate="auto")
    cov = torch.from_numpy(covers).cuda()
    n, hs = codec.gate_table(cov)
    n, hs = n.cpu().numpy(), hs.cpu().numpy()
    spec = [G.table(c, tmax, maxval) for c in covers]
    for b, (sn, sh) in enumerate(spec):
        np.testing.assert_array_equal(n[b], sn, err_msg=f"n of slice {b}")
        np.testing.assert_array_equal(hs[b], sh, err_msg=f"hs of slice {b}")
    for gate in (0, 5, 24, 65535):
        caps = codec.capacity(cov, gate=gate).cpu().numpy()
        for b, c in enumerate(covers):
            want = [G.embed(c, [], T, gate, maxval)[1]["capacity"] for T in (1, 2, tmax)]
            assert [int(caps[b, 0]), int(caps[b, 1]), int(caps[b, tmax - 1])] == want, (gate, b)
    np.testing.assert_array_equal(codec.capacity(cov).cpu().numpy(), codec.capacity(cov, gate=65535).cpu().numpy())
    lib = _lib.load()
    out = torch.empty((3, B), dtype=torch.int32, device="cuda")
    P0 = codec._params(1)

    def choose(lengths, t_fixed, g_fixed):
        lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        _lib.check(lib.codec_pee_gate_capacity(C.byref(P0), cov.data_ptr(), tmax, t_fixed, g_fixed, lens.data_ptr(), None,
                                               None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                               codec.workspace.data_ptr(), codec.workspace.numel(), None),
                   "codec_pee_gate_capacity")
        return out.cpu().numpy().T.tolist()
    totals = [int(sh.sum()) for _sn, sh in spec]
    for frac in (0.0, 0.01, 0.25, 0.7, 1.0, 1.5):
        lengths = [int(t * frac) + (1 if frac > 1 else 0) for t in totals]
        for tf in (0, 3):
            got = choose(lengths, tf, -1)
            for b, (sn, sh) in enumerate(spec):
                T, j, K = G.select(sn, sh, lengths[b], tf)
                assert got[b] == [T, G.GATES[j], K], (frac, tf, b)
        got = choose(lengths, 0, 7)
        for b, c in enumerate(covers):
            T, K = G.select_T(G.table(c, tmax, maxval, g_fixed=7)[1], lengths[b])
            assert got[b] == [T, 7, K], (frac, b)


@pytest.mark.parametrize("T,gate", [("auto", "auto"), (2, "auto"), ("auto", 24)])
def test_gpu_gate_auto_embeds_the_specs_choice(T, gate):
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    covers = _ct12(4, 130, 512, 370)
    covers[3] = PC.cover("top_band", 130, 512, "uint16", 4095, 2, 9)
    B = 4
    codec = PeeCodec(B, 130, 512, T=T, tmax=16, maxval=4095, gate=gate)
    tables = [G.table(c, 16 if T == "auto" else T, 4095) for c in covers]
    lengths = [500, 0, 4000, 10 ** 6]
    bits = [G.payload_bits(n, 3 + i) for i, n in enumerate(lengths)]
    if gate == "auto":
        picks = [G.select(n, hs, L, 0 if T == "auto" else T) for (n, hs), L in zip(tables, lengths)]
        Ts, Gs = [p[0] for p in picks], [G.GATES[p[1]] for p in picks]
    else:
        Ts = [G.select_T(G.table(c, 16, 4095, g_fixed=gate)[1], L)[0] for c, L in zip(covers, lengths)]
        Gs = [gate] * B
    enc = codec.embed(torch.from_numpy(covers).cuda(), bits)
    assert codec.t_slices.cpu().tolist() == Ts and codec.g_slices.cpu().tolist() == Gs
    _check_enc(enc, covers, bits, Ts, Gs, 4095)
    assert enc.config["gate"] == gate
    with pytest.raises(ValueError, match="capacity"):
        codec.decode(enc)            # slice 3 overflowed
    # payloads every setting holds (T = 2 alone carries under 1 000 bits of these slices)
    fit = [bits[0][:300], bits[1], bits[2][:400], bits[3][:100]]
    enc2 = codec.embed(torch.from_numpy(covers).cuda(), fit, checksum=True)
    got, back = codec.decode(enc2, verify="require")
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    for b in range(B):
        np.testing.assert_array_equal(got[b], fit[b])
    with pytest.raises(ValueError, match="ungated"):
        codec.embed_volume(torch.from_numpy(covers).cuda(), b"abc")


def test_gpu_gate_graph_replay():
    """gate_embed_auto + gate_extract captured once and replayed on refreshed covers equal the
    eager calls (and so the spec, by the tests above)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import graphs
    from codec_tcc_amd.pee import PeeCodec
    B, H, W = 3, 130, 512
    codec = PeeCodec(B, H, W, T="auto", maxval=4095, gate="auto")
    cov = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    packed = codec.pack_payloads([G.payload_bits(n, n) for n in (300, 2000, 0)])
    stego, cov2 = torch.empty_like(cov), torch.empty_like(cov)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device="cuda")
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device="cuda")
    pw = packed[0].shape[1]
    outw = torch.empty((B, pw), dtype=torch.int64, device="cuda")

    def step():
        codec.embed(cov, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False)
        codec.extract(stego, meta, lm, payload_words=pw, cover=cov2, payload=outw)

    cov.copy_(torch.from_numpy(_ct12(B, H, W, 500)).cuda())
    g = graphs.capture(step)
    for seed in (600, 700):
        host = _ct12(B, H, W, seed)
        cov.copy_(torch.from_numpy(host).cuda())
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (stego, meta, outw, cov2, codec.t_slices, codec.g_slices)]
        enc = codec.embed(torch.from_numpy(host).cuda(), None, packed=packed)
        words, back = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=pw)
        for a, b in zip(got, (enc.stego, enc.meta, words, back, codec.t_slices, codec.g_slices)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        np.testing.assert_array_equal(got[3].cpu().numpy(), host)
        st, _side = G.embed(host[0], G.payload_bits(300, 300), int(got[4][0]), int(got[5][0]), 4095)
        np.testing.assert_array_equal(got[0][0].cpu().numpy(), st)


@pytest.mark.parametrize("name", ["pe", "torax"])
def test_gpu_gate_quality_gain(name):
    """gate='auto', T='auto' against T='auto' at 8 192 and 16 384 bits: at least 2.0 dB of PSNR
    (quality.quality at the image's full scale).  The spec gives 2.8 / 3.8 dB on pe and
    5.9 / 3.7 dB on torax."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import quality
    from codec_tcc_amd.pee import PeeCodec
    img, maxval = _images()[name]
    cov = torch.from_numpy(np.stack([img, img])).cuda()
    bits = [G.payload_bits(8192, 1), G.payload_bits(16384, 2)]
    plain = PeeCodec(2, 512, 512, dtype=str(img.dtype), T="auto", maxval=maxval)
    gated = PeeCodec(2, 512, 512, dtype=str(img.dtype), T="auto", maxval=maxval, gate="auto")
    e0, e1 = plain.embed(cov, bits), gated.embed(cov, bits)
    assert all(r.status == 0 for r in e0.records() + e1.records())
    q0, q1 = quality.quality(cov, e0.stego, maxval), quality.quality(cov, e1.stego, maxval)
    for b in range(2):
        gain = q1[b]["psnr"] - q0[b]["psnr"]
        print(f"{name} {len(bits[b])} bits: T={e0.records()[b].T} {q0[b]['psnr']:.2f} dB -> "
              f"(T, G)=({e1.records()[b].T}, {e1.records()[b].reserved[1] - 1}) {q1[b]['psnr']:.2f} dB, gain {gain:.2f}")
        assert gain >= 2.0, (name, len(bits[b]), gain)
    got, back = gated.decode(e1)
    assert torch.equal(back, cov) and np.array_equal(got[1], bits[1])


@pytest.mark.parametrize("checksum", [False, True])
def test_gpu_gate_file_round_trip(tmp_path, checksum):
    from codec_tcc_amd import container, pipeline
    img, maxval = _images()["pe"]
    bits = G.payload_bits(8192, 5)
    path = str(tmp_path / "gated.stgc")
    info = pipeline.encode_file_pee(img, bits, path, T="auto", maxval=maxval, gate="auto", checksum=checksum)
    raw = open(path, "rb").read()
    assert container.pee_scheme(raw) == 3 and info["scheme"] == 3 and info["status"] == 0
    n, hs = G.table(img, 16, maxval)
    T, j, _K = G.select(n, hs, 8192)
    assert (info["T"], info["gate"]) == (T, G.GATES[j])
    st, side = G.embed(img, bits, T, G.GATES[j], maxval)
    np.testing.assert_array_equal(info["stego"], st)
    md, _blob, _data = container.parse_pee_gate_bytes(raw)
    assert (md["gate"], md["T"], md["L"], md["end"]) == (G.GATES[j], T, 8192, side["end"]) and ("cover_crc32" in md) == checksum
    got, back = pipeline.decode_bin_pee(path, verify="require" if checksum else True)
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back, img)
    with pytest.raises(ValueError, match="gated"):
        container.parse_pee_bytes(raw)
    # an ungated file of the same image and payload is byte for byte what it was: scheme byte 0
    p0 = str(tmp_path / "plain.stgc")
    pipeline.encode_file_pee(img, bits, p0, T="auto", maxval=maxval)
    assert container.pee_scheme(open(p0, "rb").read()) == 1 and open(p0, "rb").read()[11] == 0
