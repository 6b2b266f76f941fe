"""MED-PEE volume payloads on the GPU (include/codec_tcc_vol.h, codec_tcc_amd/csrc/codec_vol.hip):
the plan, the cut and the reassembly against tests/pee_volume_spec.py, and embed_volume /
decode_volume end to end against the oracle driven by that spec."""
import ctypes as C

import numpy as np
import pytest

import pee_volume_spec as V
from oracle import pee_cpu as P

pytestmark = pytest.mark.gpu


def _torch():
    return pytest.importorskip("torch")


def _params(B, H, W, pw, nbytes=2, maxval=4095):
    from codec_tcc_amd import _lib
    nc = (H // 2) * (W // 2)
    return _lib.PeeParams(B=B, H=H, W=W, bytes=nbytes, T=1, maxval=maxval, payload_words=pw,
                          lm_words=max(1, (nc + 63) // 64))


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _same(a, b):
    """Bitwise equality of two contiguous device tensors of any dtype."""
    torch = _torch()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _plan_gpu(caps, N, policy, H, W):
    """codec_pee_volume_plan on a capacity table -> the spec's dict (one read-back)."""
    torch = _torch()
    from codec_tcc_amd import _lib, pee
    B, tmax = caps.shape
    nc = (H // 2) * (W // 2)
    Pm = _params(B, H, W, max(1, (min(N, nc) + 63) // 64))
    dev = torch.from_numpy(np.ascontiguousarray(caps, dtype=np.int32)).cuda()
    out = torch.full((3 * B + 1 + 8,), -7, dtype=torch.int32, device="cuda")
    p0 = out.data_ptr()
    _lib.check(_lib.load().codec_pee_volume_plan(C.byref(Pm), dev.data_ptr(), tmax, N, _lib.VOL_POLICIES[policy], p0,
                                                 p0 + 4 * B, p0 + 8 * B, p0 + 4 * (3 * B + 1), _stream()),
               "codec_pee_volume_plan")
    host = out.cpu().numpy()
    return pee._plan_dict(host[:3 * B + 1], host[3 * B + 1:], B)


def _assert_plan(got, want):
    for k in ("status", "T", "total", "requested", "capacity", "policy"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("n", "t", "off"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _synthetic_caps(B, tmax, seed):
    """Non-decreasing in T, uneven across slices (non-monotone in b), with all-zero slices."""
    rng = np.random.default_rng(seed)
    caps = np.cumsum(rng.integers(0, 7, (B, tmax)), axis=1)
    caps[rng.random(B) < 0.15] = 0
    if B >= 5:
        caps[1] = 0
        caps[B - 2] = caps.max(axis=0)
    return caps


@pytest.mark.parametrize("tmax", [1, 16, 64])
@pytest.mark.parametrize("B", [1, 5, 64, 65, 1024, 1025, 1100])
def test_plan_matches_spec(B, tmax):
    caps = _synthetic_caps(B, tmax, 31 * B + tmax)
    S = caps.sum(axis=0)
    mid = tmax // 2
    H = W = 64   # 1024 candidates: above every entry of the table (<= 6 * 64)
    for N in sorted({0, 1, max(0, int(S[mid]) - 1), int(S[mid]), int(S[mid]) + 1, int(S[-1]), int(S[-1]) + 9}):
        for policy in V.POLICIES:
            _assert_plan(_plan_gpu(caps, N, policy, H, W), V.plan(caps, N, policy))


@pytest.mark.parametrize("policy", V.POLICIES)
def test_plan_64_bit_products(policy):
    """2048 slices of capacity near 2^20 and N near 2^31 - 1: N * P_b passes 2^61."""
    B, H, W = 2048, 2048, 2046
    nc = (H // 2) * (W // 2)
    assert B * nc <= 2 ** 31 - 1
    rng = np.random.default_rng(77)
    top = rng.integers(nc - 5000, nc + 1, B)
    caps = np.stack([top // 2, top], axis=1)
    S = caps.sum(axis=0)
    for N in (int(S[1]) - 12345, int(S[1]), int(S[0]) + 1, 2 ** 31 - 1):
        want = V.plan(caps, N, policy)
        _assert_plan(_plan_gpu(caps, N, policy, H, W), want)
    assert want["status"] == 1 and want["total"] == int(S[1])


def _lengths(B, seed, small=False):
    rng = np.random.default_rng(seed)
    if small:
        n = rng.integers(0, 14, B)
    else:
        n = rng.choice([0, 0, 1, 5, 63, 64, 65, 128, 129, 192, 193, 250], B)
        n[rng.integers(0, B, max(1, B // 8))] = rng.integers(0, 64, max(1, B // 8))
        if B >= 12:
            n[3:9] = 0   # a run of empty slices
    return n.astype(np.int64)


@pytest.mark.parametrize("B,small", [(1, False), (7, False), (65, False), (300, False), (1100, True)])
def test_scatter_and_gather_match_spec(B, small):
    """The cut and its inverse on random bit counts (runs of zeros, below 64, multiples of 64,
    64k + 1; 1100 slices of <= 13 bits, so that twenty and more share one stream word): every
    row word and every stream word, tails and pad words included; decode-side bounds on L."""
    torch = _torch()
    from codec_tcc_amd import _lib
    lib = _lib.load()
    n = _lengths(B, 50 + B, small)
    off = np.concatenate([[0], np.cumsum(n)])
    N = int(off[-1])
    pw = max(1, (int(n.max()) + 63) // 64)
    H = W = 64
    Pm = _params(B, H, W, pw)
    bits = V.stream_bits(N, B)
    stream = V.pack_stream(bits)
    d_stream = torch.from_numpy(stream.view(np.int64)).cuda()
    d_n = torch.from_numpy(n.astype(np.int32)).cuda()
    d_off = torch.from_numpy(off.astype(np.int32)).cuda()
    rows = torch.full((B, pw), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.codec_pee_volume_scatter(C.byref(Pm), d_stream.data_ptr(), N, d_n.data_ptr(), d_off.data_ptr(),
                                            rows.data_ptr(), _stream()), "codec_pee_volume_scatter")
    want_rows = V.scatter(stream, n, off, pw)
    np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint64), want_rows)

    # the inverse, from records: L = n, but for a negative L (counts as 0) and an L past the row
    L = n.copy()
    if B >= 7:
        L[2], L[5] = -9, 10 ** 6
    meta = np.zeros((B, _lib.PEE_META_BYTES // 4), np.int32)
    meta[:, 2] = L
    d_meta = torch.from_numpy(meta).cuda()
    # junk above the rows' bits must not reach the stream: fill every row's tail with ones
    junk = want_rows.copy()
    for b in range(B):
        tail = np.ones(64 * pw, np.uint8)
        tail[:int(n[b])] = V.unpack_stream(want_rows[b], int(n[b]))
        junk[b] = V.pack_stream(tail, pw)
    d_rows = torch.from_numpy(junk.view(np.int64)).cuda()
    want_off = V.record_offsets(L, pw, (H // 2) * (W // 2))
    eff = np.diff(want_off)
    sw = (int(want_off[-1]) + 63) // 64 + 2   # two pad words
    out = torch.full((sw + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.codec_pee_volume_workspace_bytes(C.byref(Pm), 1)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.codec_pee_volume_gather(C.byref(Pm), d_meta.data_ptr(), d_rows.data_ptr(), out.data_ptr(), sw,
                                           out.data_ptr() + 8 * sw, ws.data_ptr(), ws.numel(), _stream()),
               "codec_pee_volume_gather")
    host = out.cpu().numpy()
    assert int(host[sw:].view(np.int32)[0]) == int(want_off[-1])
    np.testing.assert_array_equal(host[:sw].view(np.uint64), V.gather(junk, eff, sw))
    if B < 7:
        np.testing.assert_array_equal(V.unpack_stream(host[:sw], N), bits)
    # a stream buffer shorter than the total is cut, not overrun
    if want_off[-1] > 64:
        short = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        _lib.check(lib.codec_pee_volume_gather(C.byref(Pm), d_meta.data_ptr(), d_rows.data_ptr(), short.data_ptr(), 1,
                                               short.data_ptr() + 16, ws.data_ptr(), ws.numel(), _stream()),
                   "codec_pee_volume_gather")
        h = short.cpu().numpy()
        assert h[1] == -1 and h[0].view(np.uint64) == V.gather(junk, eff, 1)[0]


def _check_volume(codec, vol, covers, bits, policy, maxval, tmax=16):
    """vol against the oracle driven by the spec: plan, info, per-slice T / L / end / status,
    stego and maps; then the exact round trip."""
    from codec_tcc_amd.pee import lm_bits
    p = V.plan(V.curves(covers, tmax, maxval), len(bits), policy)
    _assert_plan(vol.plan_host(), p)
    assert vol.embedded_bits == p["total"] and vol.total_bits == len(bits)
    assert vol.enc.lengths == [int(v) for v in p["n"]]
    stegos, sides = V.oracle_embed(covers, bits, p, maxval)
    recs = vol.enc.records()
    for b, (r, sd) in enumerate(zip(recs, sides)):
        assert (r.T, r.L, r.end, r.status) == (int(p["t"][b]), sd["L"], sd["end"], 0), b
        np.testing.assert_array_equal(lm_bits(vol.enc, b), sd["lm"])
    np.testing.assert_array_equal(vol.enc.stego.cpu().numpy(), stegos)
    got, back = codec.decode_volume(vol)
    np.testing.assert_array_equal(got, bits[:p["total"]])
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    return p


@pytest.mark.parametrize("policy", V.POLICIES)
@pytest.mark.parametrize("N", [0, 1, 63, 207, 627])
def test_volume_5x64x96(N, policy):
    """One saturated slice; the look-back launch path."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec
    covers = V.ct12_batch("5x64x96")
    bits = V.stream_bits(N, 11)
    codec = PeeCodec(5, 64, 96, dtype="uint16", T=3, tmax=16, maxval=4095)
    vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, policy=policy)
    p = _check_volume(codec, vol, covers, bits, policy, 4095)
    if policy == "even" and N == 63:
        assert list(p["n"]) == [13, 0, 19, 16, 15]
    if policy == "even" and N == 207:
        assert p["T"] == 2 and list(p["t"]) == [1, 1, 1, 2, 2]
    if N == 627:
        assert p["T"] == 3


@pytest.mark.parametrize("policy", V.POLICIES)
@pytest.mark.parametrize("name,N,env", [("3x33x47", 300, {}), ("3x33x47", 1, {}),
                                        ("4x32x64", 49, {"CODEC_PEE_SS": "1"}), ("4x32x64", 1, {"CODEC_PEE_SS": "1"}),
                                        ("1100x8x16", 1163, {}), ("1100x8x16", 1167, {}), ("1100x8x16", 5000, {})])
def test_volume_other_shapes(name, N, env, policy, monkeypatch):
    """3 x 33 x 47: the two-pass path (odd width); 4 x 32 x 64 slice-serial; 1100 x 8 x 16: more
    slices than one scan round, N = 1163 / 1167 / 5000 giving T* = 1 / 2 / 5."""
    torch = _torch()
    from codec_tcc_amd.pee import PeeCodec
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    covers = V.ct12_batch(name)
    B, H, W = covers.shape
    bits = V.stream_bits(N, 12)
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095)
    vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, policy=policy)
    p = _check_volume(codec, vol, covers, bits, policy, 4095)
    if name == "1100x8x16":
        assert p["T"] == {1163: 1, 1167: 2, 5000: 5}[N]
        if N == 5000 and policy == "even":
            assert sorted(set(p["t"].tolist())) == [1, 2, 3, 4, 5]
    if name == "4x32x64" and N == 49 and policy == "even":
        assert p["T"] == 2 and list(p["t"]) == [1, 1, 2, 1]


@pytest.mark.parametrize("policy", V.POLICIES)
def test_volume_uint8_and_in_place(policy):
    torch = _torch()
    from codec_tcc_amd import synth
    from codec_tcc_amd.pee import PeeCodec
    covers = np.stack([synth.GENERATORS["u8"](40, 24, 60 + i) for i in range(3)])
    caps = V.curves(covers, 8)
    N = int(caps[:, 2].sum()) + 5
    bits = V.stream_bits(N, 13)
    codec = PeeCodec(3, 40, 24, dtype="uint8", tmax=8)
    vol = codec.embed_volume(torch.from_numpy(covers).cuda(), bits, policy=policy)
    _check_volume(codec, vol, covers, bits, policy, None, tmax=8)
    # in place: the capacity pass reads the covers before the embed overwrites them
    covers = V.ct12_batch("5x64x96")
    bits = V.stream_bits(627, 14)
    codec = PeeCodec(5, 64, 96, dtype="uint16", tmax=16, maxval=4095)
    dev = torch.from_numpy(covers).cuda()
    vol = codec.embed_volume(dev, bits, policy=policy, stego=dev)
    assert vol.enc.stego.data_ptr() == dev.data_ptr()
    _check_volume(codec, vol, covers, bits, policy, 4095)


def test_volume_overflow():
    """N = 3124 > S(16) = 3115: status 1, the first 3115 bits embedded, every slice reversible;
    encode_volume raises."""
    torch = _torch()
    import codec_tcc_amd
    from codec_tcc_amd.pee import PeeCodec
    covers = V.ct12_batch("5x64x96")
    bits = V.stream_bits(3124, 15)
    codec = PeeCodec(5, 64, 96, dtype="uint16", tmax=16, maxval=4095)
    dev = torch.from_numpy(covers).cuda()
    for policy in V.POLICIES:
        vol = codec.embed_volume(dev, bits, policy=policy, checksum=True)
        p = _check_volume(codec, vol, covers, bits, policy, 4095)
        assert (p["status"], p["T"], p["total"]) == (1, 16, 3115)
        assert vol.embedded_bits == 3115 and vol.total_bits == 3124
        got, _ = codec.decode_volume(vol, verify="require")
        np.testing.assert_array_equal(got, bits[:3115])
    with pytest.raises(ValueError, match="capacity"):
        codec_tcc_amd.encode_volume(dev, bits, maxval=4095)


def test_volume_checksums():
    torch = _torch()
    import codec_tcc_amd
    from codec_tcc_amd import IntegrityError
    covers = V.ct12_batch("5x64x96")
    bits = V.stream_bits(627, 16)
    dev = torch.from_numpy(covers).cuda()
    vol = codec_tcc_amd.encode_volume(dev, bits, maxval=4095, checksum=True)
    assert vol.payload_crc is not None and vol.enc.cover_crc is not None
    got, back = codec_tcc_amd.decode_volume(vol, verify="require")
    np.testing.assert_array_equal(got, bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    # every slice stays decodable by the per-slice code
    per, back = codec_tcc_amd.pee.decode(vol.enc)
    np.testing.assert_array_equal(np.concatenate(per), bits)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    # one flipped stego pixel (a context pixel of slice 3): its cover checksum fails
    keep = vol.enc.stego.clone()
    vol.enc.stego.view(torch.int16)[3, 10, 10] ^= 4
    with pytest.raises(IntegrityError, match="cover"):
        codec_tcc_amd.decode_volume(vol)
    vol.enc.stego.copy_(keep)
    # one flipped stream bit: the LSB of an expanded candidate carries a payload bit and nothing
    # else, so the covers still restore and only the payload checksum fails
    p = V.plan(V.curves(covers, 16, 4095), 627, "even")
    _st, sides = V.oracle_embed(covers, bits, p, 4095)
    x, a, b, c = P._grids(covers[0])
    e = (x - P.med(a, b, c)).ravel()
    T0 = int(p["t"][0])
    k = int(np.flatnonzero((e >= -T0) & (e < T0) & ~np.pad(sides[0]["lm"], (0, e.size - sides[0]["lm"].size)))[0])
    assert k <= sides[0]["end"]
    wc = covers.shape[2] // 2
    vol.enc.stego.view(torch.int16)[0, 2 * (k // wc) + 1, 2 * (k % wc) + 1] ^= 1
    with pytest.raises(IntegrityError, match="payload"):
        codec_tcc_amd.decode_volume(vol)
    got, back = codec_tcc_amd.decode_volume(vol, verify=False)
    assert int((got != bits).sum()) == 1
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    vol.enc.stego.copy_(keep)
    novol = codec_tcc_amd.encode_volume(dev, bits, maxval=4095)
    with pytest.raises(IntegrityError, match="require"):
        codec_tcc_amd.decode_volume(novol, verify="require")


@pytest.mark.parametrize("policy", V.POLICIES)
def test_convenience_entries_equal_separate_calls(policy):
    """codec_pee_volume_embed / _extract against capacity -> plan -> scatter -> embed_ts and
    extract -> gather called one by one: bit for bit."""
    torch = _torch()
    from codec_tcc_amd import _lib
    from codec_tcc_amd.pee import PeeCodec
    lib = _lib.load()
    covers = V.ct12_batch("5x64x96")
    B, H, W = covers.shape
    N = 627
    bits = V.stream_bits(N, 17)
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095)
    dev = torch.from_numpy(covers).cuda()
    vol = codec.embed_volume(dev, bits, policy=policy)
    pw = vol.enc.payload_words
    Pm = codec._params(pw)
    caps = codec.capacity(dev)
    plan = torch.full((3 * B + 1 + 8,), -1, dtype=torch.int32, device="cuda")
    p0 = plan.data_ptr()
    _lib.check(lib.codec_pee_volume_plan(C.byref(Pm), caps.data_ptr(), 16, N, _lib.VOL_POLICIES[policy], p0, p0 + 4 * B,
                                         p0 + 8 * B, p0 + 4 * (3 * B + 1), _stream()), "codec_pee_volume_plan")
    words, nbits = codec.pack_volume(bits)
    rows = torch.empty((B, pw), dtype=torch.int64, device="cuda")
    _lib.check(lib.codec_pee_volume_scatter(C.byref(Pm), words.data_ptr(), nbits, p0, p0 + 8 * B, rows.data_ptr(),
                                            _stream()), "codec_pee_volume_scatter")
    stego = torch.empty_like(dev)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device="cuda")
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device="cuda")
    _lib.check(lib.codec_pee_embed_ts(C.byref(Pm), dev.data_ptr(), stego.data_ptr(), rows.data_ptr(), p0, p0 + 4 * B,
                                      meta.data_ptr(), lm.data_ptr(), codec.workspace.data_ptr(),
                                      codec.workspace.numel(), _stream()), "codec_pee_embed_ts")
    assert torch.equal(plan[:3 * B + 1], vol.plan) and torch.equal(plan[3 * B + 1:], vol.info)
    assert _same(stego, vol.enc.stego) and _same(meta, vol.enc.meta)
    ends = [r.end for r in vol.enc.records()]
    for b in range(B):   # the map is defined over candidates 0..end
        w = (ends[b] + 1 + 63) // 64
        got = np.unpackbits(lm[b, :w].cpu().numpy().view(np.uint8), bitorder="little")[:ends[b] + 1]
        ref = np.unpackbits(vol.enc.lm[b, :w].cpu().numpy().view(np.uint8), bitorder="little")[:ends[b] + 1]
        np.testing.assert_array_equal(got, ref)
    # decode side
    out_rows, cover = codec.extract(stego, meta, lm, payload_words=pw)
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


def test_volume_embed_graph_replay():
    """embed_volume's launches on preallocated buffers captured as a graph (a linear chain, as
    tests/test_pee.py's capture test), replayed twice on refreshed covers: equal to eager."""
    torch = _torch()
    from codec_tcc_amd import graphs, synth
    from codec_tcc_amd.pee import PeeCodec
    B, H, W, N = 3, 256, 264, 4000
    codec = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095)
    bits = V.stream_bits(N, 18)
    packed = codec.pack_volume(bits)
    cov = torch.empty((B, H, W), dtype=torch.uint16, device="cuda")
    stego = torch.empty_like(cov)
    buffers = codec.volume_buffers()
    made = []

    def step():
        made.append(codec.embed_volume(cov, None, stego=stego, check=False, buffers=buffers, packed=packed))

    cov.copy_(torch.from_numpy(np.stack([synth.ct12(H, W, 500 + i) for i in range(B)])).cuda())
    g = graphs.capture(step)
    vol = made[-1]
    for seed in (600, 700):
        host = np.stack([synth.ct12(H, W, seed + i) for i in range(B)])
        cov.copy_(torch.from_numpy(host).cuda())
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (stego, buffers[1])]
        eager = PeeCodec(B, H, W, dtype="uint16", tmax=16, maxval=4095).embed_volume(torch.from_numpy(host).cuda(), bits)
        assert _same(got[0], eager.enc.stego)
        nm = B * 16
        assert torch.equal(got[1][nm:], torch.cat([eager.plan, eager.info]))
        assert torch.equal(got[1][:nm].view(torch.uint8).view(B, 64), eager.enc.meta)
        out, back = codec.decode_volume(vol)
        np.testing.assert_array_equal(out, bits)
        np.testing.assert_array_equal(back.cpu().numpy(), host)
        p = V.plan(V.curves(host, 16, 4095), N, "even")
        np.testing.assert_array_equal(got[1][nm:nm + B].cpu().numpy(), p["n"])
