"""Gated MED-PEE volume payloads on the GPU (include/codec_tcc_gvol.h,
codec_tcc_amd/csrc/codec_gvol.hip): the plan kernel on uploaded tables against
tests/pee_gvol_spec.py for every known-answer case, and embed_volume(gate=...) / decode_volume
end to end against tests/pee_gate_spec.py driven by that plan."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pee_gate_spec as G
import pee_gvol_spec as S
import pee_volume_spec as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INFO_FIELDS = ("status", "T", "total", "requested", "capacity", "policy", "gate")


def _torch():
    return pytest.importorskip("torch")


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _same(a, b):
    """Bitwise equality of two contiguous device tensors of any dtype."""
    torch = _torch()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _kats():
    with open(os.path.join(HERE, "golden", "pee_gvol_kat.json")) as f:
        return json.load(f)


def _shape_of(source):
    """(H, W, nbytes, maxval) the plan entry is told for a known-answer source; the witness
    tables stand for 31 slices of 2^26 candidates."""
    if source.startswith("witness"):
        return 16384, 16384, 2, 4095
    covers, maxval = S.stack(source.split(":")[0])
    return covers.shape[1], covers.shape[2], covers.dtype.itemsize, maxval


def _upload_tables(tables):
    torch = _torch()
    n = np.array([t[0] for t in tables], dtype=np.uint32)
    hs = np.array([t[1] for t in tables], dtype=np.uint32)
    return torch.from_numpy(n.view(np.int32)).cuda(), torch.from_numpy(hs.view(np.int32)).cuda()


def _plan_gpu(tables, N, policy, g_fixed, H, W, nbytes=2, maxval=4095):
    """codec_pee_gvol_plan on uploaded tables -> (the spec's dict, the raw info record)."""
    torch = _torch()
    from codec_tcc_amd import _lib, pee
    B, tmax = len(tables), len(tables[0][1])
    nc = (H // 2) * (W // 2)
    Pm = _lib.PeeParams(B=B, H=H, W=W, bytes=nbytes, T=1, maxval=maxval, payload_words=max(1, (min(N, nc) + 63) // 64),
                        lm_words=max(1, (nc + 63) // 64))
    d_n, d_hs = _upload_tables(tables)
    out = torch.full((4 * B + 1 + 10,), -7, dtype=torch.int32, device="cuda")
    p0 = out.data_ptr()
    _lib.check(_lib.load().codec_pee_gvol_plan(
        C.byref(Pm), d_n.data_ptr(), d_hs.data_ptr(), tmax, N, _lib.VOL_POLICIES[policy], -1 if g_fixed is None else g_fixed,
        p0, p0 + 4 * B, p0 + 4 * (3 * B + 1), p0 + 8 * B, p0 + 4 * (4 * B + 1), _stream()), "codec_pee_gvol_plan")
    host = out.cpu().numpy()
    return pee._plan_dict(host[:4 * B + 1], host[4 * B + 1:], B, gated=True), host[4 * B + 1:]


def _assert_plan(got, want):
    for k in INFO_FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("n", "t", "g", "off"):
        np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k)


@pytest.mark.parametrize("k", _kats(), ids=lambda k: f"{k['source']}-t{k['tmax']}-g{k['g_fixed']}-N{k['N']}")
def test_plan_kernel_matches_spec(k):
    """k_gvol_plan alone: n, t, g, off and every info field, on every known-answer case -- B = 1,
    1100 slices (the scan's carry across rounds of 1024), the 31-slice 2^26 tables (the
    128-bit comparison: tests/test_pee_gvol_host.py shows a 64-bit one picks another pair)."""
    tables = S.source_tables(k["source"], k["tmax"], k["g_fixed"])
    H, W, nbytes, maxval = _shape_of(k["source"])
    for policy in S.POLICIES:
        got, info = _plan_gpu(tables, k["N"], policy, k["g_fixed"], H, W, nbytes, maxval)
        want = dict(k[policy], policy=policy)
        _assert_plan(got, want)
        assert list(info) == [want["status"], want["T"], want["total"], want["requested"], want["capacity"],
                              V.POLICIES.index(policy), k["B"], k["tmax"], want["gate"], 0]
    _assert_plan(got, dict(S.plan(tables, k["N"], policy, k["g_fixed"]), policy=policy))


def test_plan_kernel_clamps_what_the_buffers_hold():
    """Table values past (H/2)(W/2) count as (H/2)(W/2) and a slice's share never passes it:
    every n_b fits its payload row and the offsets stay a prefix sum, whatever was uploaded."""
    rng = np.random.default_rng(5)
    B, tmax, H, W = 70, 16, 16, 16
    nc = 64
    tables = [([int(v) for v in rng.integers(0, 2 ** 32, 16, dtype=np.uint64)],
               [[int(v) for v in r] for r in rng.integers(0, 2 ** 32, (tmax, 16), dtype=np.uint64)]) for _ in range(B)]
    for policy in S.POLICIES:
        for g_fixed in (None, 9):
            got, _info = _plan_gpu(tables, 3000, policy, g_fixed, H, W)
            n = got["n"].astype(np.int64)
            assert ((0 <= n) & (n <= nc)).all() and int(n.sum()) == got["total"] <= 3000
            np.testing.assert_array_equal(got["off"], np.concatenate([[0], np.cumsum(n)]))
            assert ((1 <= got["t"]) & (got["t"] <= tmax)).all()
            assert set(got["g"].tolist()) <= (set(G.GATES) if g_fixed is None else {9})


# ---------------------------------------------------------------- end to end
def _check_gvol(codec, vol, covers, bits, policy, maxval, gate, tmax=16):
    """vol against the gated spec driven by the plan spec: plan, info, per-slice T / G / L /
    end / status, stego and maps; the exact round trip; each slice decoded on its own."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec, lm_bits
    g_fixed = None if gate == "auto" else int(gate)
    p = S.plan(S.tables_of(covers, tmax, maxval, g_fixed), len(bits), policy, g_fixed)
    _assert_plan(vol.plan_host(), p)
    assert vol.embedded_bits == p["total"] and vol.total_bits == len(bits)
    assert vol.enc.lengths == [int(v) for v in p["n"]]
    assert vol.gate == gate and vol.enc.config["gate"] == gate
    stegos, sides = S.oracle_embed(covers, bits, p, maxval)
    recs = vol.enc.records()
    for b, (r, sd) in enumerate(zip(recs, sides)):
        assert (r.T, r.L, r.end, r.status, r.reserved[1]) == (int(p["t"][b]), sd["L"], sd["end"], 0, int(p["g"][b]) + 1), b
        assert sd["status"] == 0 and r.lm_count == sd["lm_count"]
        np.testing.assert_array_equal(lm_bits(vol.enc, b), sd["lm"])
    np.testing.assert_array_equal(vol.enc.stego.cpu().numpy(), stegos)
    got, back = codec.decode_volume(vol)
    np.testing.assert_array_equal(got, bits[:p["total"]])
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    # the records are ordinary gated records: the per-slice code decodes every slice on its own
    B, H, W = covers.shape
    alone = PeeCodec(B, H, W, dtype=str(covers.dtype), T=2, maxval=maxval, gate=0)
    per, back = alone.decode(vol.enc)
    np.testing.assert_array_equal(np.concatenate(per), bits[:p["total"]])
    assert torch.equal(back.cpu(), torch.from_numpy(covers))
    return p


STACKS = {"5x64x96": 627, "3x33x47": 150, "pe": 16384, "torax": 16384}


@pytest.mark.parametrize("policy", S.POLICIES)
@pytest.mark.parametrize("gate", ["auto", 6])
@pytest.mark.parametrize("name", list(STACKS))
def test_gated_volume_matches_spec(name, gate, policy):
    """5 x 64 x 96 ct12 with a saturated slice (the look-back path), 3 x 33 x 47 (odd sizes: the
    two-pass path), the pe (uint16) and torax (uint8) quadrant stacks."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec
    covers, maxval = S.stack(name)
    B, H, W = covers.shape
    N = STACKS[name] if gate == "auto" or name in S.IMAGES else STACKS[name] // 10   # gate 6 holds 128 / 17 bits
    bits = V.stream_bits(N, 21)
    codec = PeeCodec(B, H, W, dtype=str(covers.dtype), T=3, tmax=16, maxval=maxval)
    vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, policy=policy, gate=gate)
    p = _check_gvol(codec, vol, covers, bits, policy, maxval, gate)
    assert p["status"] == 0 and p["total"] == N
    if name in S.IMAGES and gate == "auto":
        assert (p["T"], p["gate"]) == {"pe": (2, 6), "torax": (1, 6)}[name]


@pytest.mark.parametrize("policy", S.POLICIES)
def test_gated_volume_edges(policy):
    """N = 0; N at the stack's capacity at (tmax, the open gate); N above it (status 1, the
    capacity embedded, every slice reversible, the prefix returned); in place; a fixed gate's
    overflow."""
    torch = _torch()
    import codec_tcc_amd
    from codec_tcc_amd.pee import PeeCodec
    covers, maxval = S.stack("5x64x96")
    dev = torch.from_numpy(covers).cuda()
    codec = PeeCodec(5, 64, 96, dtype="uint16", tmax=16, maxval=maxval)
    cap = int(V.curves(covers, 16, maxval)[:, -1].sum())
    assert cap == 3115
    for N in (0, cap):
        bits = V.stream_bits(N, 22)
        p = _check_gvol(codec, codec.embed_volume(dev, bits, policy=policy, gate="auto"), covers, bits, policy, maxval, "auto")
        assert (p["status"], p["total"]) == (0, N)
    bits = V.stream_bits(cap + 9, 23)
    vol = codec.embed_volume(dev, bits, policy=policy, gate="auto", checksum=True)
    p = _check_gvol(codec, vol, covers, bits, policy, maxval, "auto")
    assert (p["status"], p["T"], p["gate"], p["total"]) == (1, 16, 65535, cap)
    assert vol.embedded_bits == cap and vol.total_bits == cap + 9
    got, _ = codec.decode_volume(vol, verify="require")
    np.testing.assert_array_equal(got, bits[:cap])
    with pytest.raises(ValueError, match="capacity"):
        codec_tcc_amd.encode_volume(dev, bits, maxval=maxval, gate="auto")
    # a fixed gate overflows at its own capacity
    cap6 = sum(S.K_of(t[1], 16, 0) for t in S.source_tables("5x64x96", 16, 6))
    bits = V.stream_bits(cap6 + 1, 24)
    p = _check_gvol(codec, codec.embed_volume(dev, bits, policy=policy, gate=6), covers, bits, policy, maxval, 6)
    assert (p["status"], p["total"]) == (1, cap6)
    # in place: the table pass reads the covers before the embed overwrites them
    bits = V.stream_bits(627, 25)
    work = dev.clone()
    vol = codec.embed_volume(work, bits, policy=policy, stego=work, gate="auto")
    assert vol.enc.stego.data_ptr() == work.data_ptr()
    _check_gvol(codec, vol, covers, bits, policy, maxval, "auto")


def test_gated_volume_checksums_and_package_calls():
    torch = _torch()
    import codec_tcc_amd
    from codec_tcc_amd import IntegrityError
    covers, maxval = S.stack("5x64x96")
    bits = V.stream_bits(627, 26)
    dev = torch.from_numpy(covers).cuda()
    vol = codec_tcc_amd.encode_volume(dev, bits, maxval=maxval, checksum=True, gate="auto")
    assert vol.payload_crc is not None and vol.enc.cover_crc is not None and vol.gate == "auto"
    assert any(r.reserved[1] != 0 for r in vol.enc.records())
    got, back = codec_tcc_amd.decode_volume(vol, verify="require")
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    # one flipped stego pixel (a context pixel of slice 3): its cover checksum fails
    vol.enc.stego.view(torch.int16)[3, 10, 10] ^= 4
    with pytest.raises(IntegrityError, match="cover"):
        codec_tcc_amd.decode_volume(vol)
    novol = codec_tcc_amd.encode_volume(dev, bits[:100], maxval=maxval, gate=6)   # gate 6 holds 128 bits here
    assert {r.reserved[1] for r in novol.enc.records()} == {7} and novol.plan_host()["gate"] == 6
    with pytest.raises(IntegrityError, match="require"):
        codec_tcc_amd.decode_volume(novol, verify="require")
    got, _ = codec_tcc_amd.decode_volume(novol)
    np.testing.assert_array_equal(got, bits[:100])
    # a codec built with gate= still refuses volumes
    gated = codec_tcc_amd.PeeCodec(5, 64, 96, dtype="uint16", maxval=maxval, gate=6)
    for kw in ({}, {"gate": "auto"}):
        with pytest.raises(ValueError, match="ungated"):
            gated.embed_volume(dev, bits, **kw)


@pytest.mark.parametrize("name", ["5x64x96", "3x33x47", "pe"])
def test_ungated_volume_is_unchanged(name):
    """embed_volume without gate= is what it was: pee_volume_spec's plan, the oracle's stego,
    ungated records, the 3 B + 1 plan and the 8-word info record."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec
    covers, maxval = S.stack(name)
    B, H, W = covers.shape
    N = STACKS[name]
    bits = V.stream_bits(N, 27)
    codec = PeeCodec(B, H, W, dtype=str(covers.dtype), tmax=16, maxval=maxval)
    lm, side = codec.volume_buffers()
    assert side.numel() == B * 16 + 3 * B + 1 + 8 and codec.volume_buffers(gate=True)[1].numel() == side.numel() + B + 2
    for policy in V.POLICIES:
        vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, policy=policy)
        p = V.plan(V.curves(covers, 16, maxval), N, policy)
        got = vol.plan_host()
        assert "g" not in got and vol.gate is None and "gate" not in vol.enc.config
        assert vol.plan.numel() == 3 * B + 1 and vol.info.numel() == 8
        for key in ("status", "T", "total", "requested", "capacity"):
            assert got[key] == p[key]
        for key in ("n", "t", "off"):
            np.testing.assert_array_equal(got[key], p[key])
        stegos, _sides = V.oracle_embed(covers, bits, p, maxval)
        np.testing.assert_array_equal(vol.enc.stego.cpu().numpy(), stegos)
        assert all(r.reserved[1] == 0 for r in vol.enc.records())
        out, back = codec.decode_volume(vol)
        np.testing.assert_array_equal(out, bits)
        np.testing.assert_array_equal(back.cpu().numpy(), covers)


@pytest.mark.parametrize("gate", ["auto", 6])
def test_convenience_entries_equal_separate_calls(gate):
    """codec_pee_gvol_embed / _extract against gate_capacity -> gvol_plan -> volume_scatter ->
    gate_embed and gate_extract -> volume_gather called one by one: bit for bit."""
    torch = _torch()
    from codec_tcc_amd import _lib
    from codec_tcc_amd.pee import PeeCodec
    lib = _lib.load()
    covers, maxval = S.stack("5x64x96")
    B, H, W = covers.shape
    N, g_fixed = (400, -1) if gate == "auto" else (100, gate)   # gate 6 holds 128 bits here
    bits = V.stream_bits(N, 28)
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=maxval)
    dev = torch.from_numpy(covers).cuda()
    vol = codec.embed_volume(dev, bits, gate=gate)
    pw = vol.enc.payload_words
    Pm = codec._params(pw)
    n_t, hs_t = codec.gate_table(dev, 16, None if gate == "auto" else gate)
    plan = torch.full((4 * B + 1 + 10,), -1, dtype=torch.int32, device="cuda")
    p0 = plan.data_ptr()
    _lib.check(lib.codec_pee_gvol_plan(C.byref(Pm), n_t.data_ptr(), hs_t.data_ptr(), 16, N, 0, g_fixed, p0, p0 + 4 * B,
                                       p0 + 4 * (3 * B + 1), p0 + 8 * B, p0 + 4 * (4 * B + 1), _stream()),
               "codec_pee_gvol_plan")
    words, nbits = codec.pack_volume(bits)
    rows = torch.empty((B, pw), dtype=torch.int64, device="cuda")
    _lib.check(lib.codec_pee_volume_scatter(C.byref(Pm), words.data_ptr(), nbits, p0, p0 + 8 * B, rows.data_ptr(),
                                            _stream()), "codec_pee_volume_scatter")
    stego = torch.empty_like(dev)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device="cuda")
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device="cuda")
    _lib.check(lib.codec_pee_gate_embed(C.byref(Pm), dev.data_ptr(), stego.data_ptr(), rows.data_ptr(), p0, p0 + 4 * B,
                                        p0 + 4 * (3 * B + 1), meta.data_ptr(), lm.data_ptr(), codec.workspace.data_ptr(),
                                        codec.workspace.numel(), _stream()), "codec_pee_gate_embed")
    assert torch.equal(plan[:4 * B + 1], vol.plan) and torch.equal(plan[4 * B + 1:], vol.info)
    assert _same(stego, vol.enc.stego) and _same(meta, vol.enc.meta)
    ends = [r.end for r in vol.enc.records()]
    for b in range(B):   # the map is defined over candidates 0..end
        w = (ends[b] + 1 + 63) // 64
        mine = np.unpackbits(lm[b, :w].cpu().numpy().view(np.uint8), bitorder="little")[:ends[b] + 1]
        ref = np.unpackbits(vol.enc.lm[b, :w].cpu().numpy().view(np.uint8), bitorder="little")[:ends[b] + 1]
        np.testing.assert_array_equal(mine, ref)
    out_rows, cover = codec.extract(stego, meta, lm, payload_words=pw, gated=True)
    sw = (N + 63) // 64
    out = torch.full((sw + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.codec_pee_volume_workspace_bytes(C.byref(Pm), 1)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.codec_pee_volume_gather(C.byref(Pm), meta.data_ptr(), out_rows.data_ptr(), out.data_ptr(), sw,
                                           out.data_ptr() + 8 * sw, ws.data_ptr(), ws.numel(), _stream()),
               "codec_pee_volume_gather")
    host = out.cpu().numpy()
    got, back = codec.decode_volume(vol)
    assert int(host[sw:].view(np.int32)[0]) == N
    np.testing.assert_array_equal(V.unpack_stream(host[:sw], N), got)
    np.testing.assert_array_equal(got, bits)
    assert _same(cover, back)


def _ct12(B, H, W, seed):
    from codec_tcc_amd import synth
    return np.stack([synth.ct12(H, W, seed + i) for i in range(B)])


def test_gated_volume_graph_replay():
    """embed_volume(gate="auto") on preallocated buffers and the decode entry captured as one
    graph, replayed on refreshed covers whose tables lead to another (T*, G*): equal to eager."""
    torch = _torch()
    from codec_tcc_amd import _lib, graphs
    from codec_tcc_amd.pee import PeeCodec
    lib = _lib.load()
    B, H, W, N = 3, 130, 512, 4000
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095)
    bits = V.stream_bits(N, 29)
    packed = codec.pack_volume(bits)
    cov = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    stego, cov2 = torch.empty_like(cov), torch.empty_like(cov)
    buffers = codec.volume_buffers(gate=True)
    sw = (N + 63) // 64
    out = torch.empty(sw + 1, dtype=torch.int64, device="cuda")
    made = []

    def step():
        vol = codec.embed_volume(cov, None, stego=stego, check=False, buffers=buffers, packed=packed, gate="auto")
        made.append(vol)
        gws = codec._gvol_workspace(vol.enc.payload_words, 1)
        _lib.check(lib.codec_pee_gvol_extract(
            C.byref(codec._params(vol.enc.payload_words)), stego.data_ptr(), vol.enc.meta.data_ptr(), vol.enc.lm.data_ptr(),
            cov2.data_ptr(), out.data_ptr(), sw, out.data_ptr() + 8 * sw, codec.workspace.data_ptr(),
            codec.workspace.numel(), gws.data_ptr(), gws.numel(), _stream()), "codec_pee_gvol_extract")

    first = _ct12(B, H, W, 500)
    cov.copy_(torch.from_numpy(first).cuda())
    g = graphs.capture(step)
    vol = made[-1]
    p0 = S.plan(S.tables_of(first, 16, 4095), N, "even")
    picks = []
    for host in ((_ct12(B, H, W, 600) >> 3 << 3).astype(np.uint16), _ct12(B, H, W, 700)):
        cov.copy_(torch.from_numpy(host).cuda())
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (stego, buffers[1], out, cov2)]
        eager = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095).embed_volume(
            torch.from_numpy(host).cuda(), bits, gate="auto")
        assert _same(got[0], eager.enc.stego)
        nm = B * 16
        assert torch.equal(got[1][nm:], torch.cat([eager.plan, eager.info]))
        assert torch.equal(got[1][:nm].view(torch.uint8).view(B, 64), eager.enc.meta)
        np.testing.assert_array_equal(got[3].cpu().numpy(), host)
        h = got[2].cpu().numpy()
        assert int(h[sw:].view(np.int32)[0]) == N
        np.testing.assert_array_equal(V.unpack_stream(h[:sw], N), bits)
        bits_back, back = codec.decode_volume(vol)
        np.testing.assert_array_equal(bits_back, bits)
        np.testing.assert_array_equal(back.cpu().numpy(), host)
        p = S.plan(S.tables_of(host, 16, 4095), N, "even")
        _assert_plan(vol.plan_host(), p)
        picks.append((p["T"], p["gate"]))
    assert picks[0] != (p0["T"], p0["gate"])   # the replay chose anew, from the refreshed covers


@pytest.mark.parametrize("name", ["pe", "torax"])
def test_gated_volume_quality_gain(name):
    """The quadrant stacks, policy even, 4 096 and 16 384 bits: the stack PSNR of the gated
    volume is at least 2.0 dB above the ungated volume's (the spec gives 5.15 / 5.49 dB on pe and
    6.57 / 3.24 dB on torax, and the GPU is bit-exact with it: a floor, not a measurement)."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec
    covers, maxval = S.stack(name)
    B, H, W = covers.shape
    dev = torch.from_numpy(covers).cuda()
    codec = PeeCodec(B, H, W, dtype=str(covers.dtype), tmax=16, maxval=maxval)
    for N in (4096, 16384):
        bits = V.stream_bits(N, 1)
        v0 = codec.embed_volume(dev, bits, policy="even")
        v1 = codec.embed_volume(dev, bits, policy="even", gate="auto")
        assert v0.embedded_bits == v1.embedded_bits == N
        q0 = G.psnr(v0.enc.stego.cpu().numpy(), covers, maxval)
        q1 = G.psnr(v1.enc.stego.cpu().numpy(), covers, maxval)
        info = v1.plan_host()
        print(f"{name} {N} bits: ungated {q0:.2f} dB -> gated (T*, G*) = ({info['T']}, {info['gate']}) {q1:.2f} dB, "
              f"gain {q1 - q0:.2f}")
        assert q1 - q0 >= 2.0, (name, N, q1 - q0)
        got, back = codec.decode_volume(v1)
        np.testing.assert_array_equal(got, bits)
        assert torch.equal(back, dev)
