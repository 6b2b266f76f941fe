"""Blind MED-PEE on the GPU where its loops run more than once (csrc/codec_blind.hip), bit-exact
against tests/pee_blind_spec.py on the SHAPE_CASES of tests/pee_blind_cases.py:

  tall     hc = 550: k_blind_plan's scan over three chunks of 256 rows, cap0 / uns0 carried, i* in
           every chunk
  wide     W > 1024: the VEC row pass's second and ragged third lane iteration, 515 candidates per
           row on the scalar route; info words 6 and 7 straight from codec_pee_blind_plan
  many     E > 256 entries and a map of more than 256 words: k_blind_pack's carry, entries >= 16384,
           k_blind_scatter's second block; max_entries as the boundary at E; the decoder's entry
           rules (padding, duplicates, entries beyond `end` or >= nc) against the spec's
  long     n_side + n_user > 16384: k_blind_splice and k_blind_restore beyond their first block, a
           map of more than 768 words
  narrow   wc = 1, W = 8, dozens of reserved rows, slices the header fills or does not fit

Every case: stego and info are the spec's, decode_blind returns bits and cover, the spec decodes
the GPU's stego, the covers are untouched.  The spec at these shapes is pinned to the scalar
restatement by tests/test_pee_blind_host.py."""
import ctypes as C

import numpy as np
import pytest

import pee_blind_cases as CS
import pee_blind_spec as BS

pytestmark = pytest.mark.gpu

_spec = {}


def _codec(B, H, W, dtype, T, maxval):
    from codec_tcc_amd.pee import PeeCodec
    return PeeCodec(B, H, W, dtype=dtype, T=T, maxval=maxval)


def _reference(name):
    """(cover, T, maxval, max_entries, checksum, [(bits, stego, info, plan) per length]), once per case."""
    if name not in _spec:
        img, T, mv, me, checksum, lengths, _cap = CS.shape_case(name)
        rows = []
        for q, n in enumerate(lengths):
            bits = CS.payload(n, q + 1)
            st, info, p = BS.embed(img, bits, T, mv, checksum, me)
            st.setflags(write=False)
            rows.append((bits, st, info, p))
        _spec[name] = (img, T, mv, me, checksum, rows)
    return _spec[name]


def _names(group):
    return [c[0] for c in CS.SHAPE_CASES if c[1] == group]


def _parity(codec, covers, bits, T, mv, checksum, max_entries, want=None):
    """embed_blind on the stack against the spec slice by slice (stego, info), decode_blind (bits,
    cover), the spec's decode of the GPU's stego, the covers left alone.  Every slice must embed."""
    import torch
    B = covers.shape[0]
    cov = torch.from_numpy(covers).cuda()
    stego, info = codec.embed_blind(cov, bits, checksum=checksum, max_entries=max_entries)
    got_st, got_info = stego.cpu().numpy(), info.cpu().numpy()
    assert got_info.shape == (B, 6)
    for b in range(B):
        st, winfo = want[b] if want is not None else BS.embed(covers[b], bits[b], T, mv, checksum, max_entries)[:2]
        assert winfo[0] == 0, (b, winfo)
        assert tuple(int(v) for v in got_info[b]) == tuple(winfo), (b, got_info[b], winfo)
        np.testing.assert_array_equal(got_st[b], st, err_msg=f"stego of slice {b}")
    out, back = codec.decode_blind(stego)
    np.testing.assert_array_equal(back.cpu().numpy(), covers)
    for b in range(B):
        np.testing.assert_array_equal(out[b], bits[b], err_msg=f"bits of slice {b}")
        sb, sc, hdr = BS.decode(got_st[b])   # the spec reads what the GPU wrote
        np.testing.assert_array_equal(sb, bits[b])
        np.testing.assert_array_equal(sc, covers[b])
        assert hdr["flags"] == int(checksum) and hdr["crc"] == (BS.cover_crc(covers[b]) if checksum else 0)
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)
    return cov, stego


def _run(name):
    """The case's cover in every slice, one slice per payload length of the case."""
    img, T, mv, me, checksum, rows = _reference(name)
    B = len(rows)
    covers = np.stack([img] * B)
    codec = _codec(B, img.shape[0], img.shape[1], str(img.dtype), T, mv)
    cov, stego = _parity(codec, covers, [r[0] for r in rows], T, mv, checksum, me, want=[(r[1], r[2]) for r in rows])
    return codec, cov, stego


def _capacity(codec, cov, max_entries):
    return codec.blind_capacity(cov, max_entries=max_entries).cpu().tolist()


@pytest.mark.parametrize("name", _names("tall"))
def test_gpu_blind_tall(name):
    """hc = 550, B = 3 with (cap, 55 % of it, 0) bits: i* lies in the plan's chunk 2, 1 and 0 and E
    grows with the chunk, so cap0 and uns0 are carried twice and first-fit rows lie behind both
    chunk edges; 1100 x 24 takes the VEC row pass, 1101 x 22 the scalar one."""
    img, T, mv, _me, _ck, rows = _reference(name)
    plans = [r[3] for r in rows]
    assert img.shape[0] // 2 == 550
    assert [p["i_star"] // 256 for p in plans] == [2, 1, 0]
    assert plans[0]["E"] > plans[1]["E"] > plans[2]["E"] > 0
    if name == "tall_vec_u16":
        assert rows[0][0].size == 2906 and [(p["i_star"], p["E"]) for p in plans] == [(541, 5), (331, 3), (92, 1)]
    codec, cov, _stego = _run(name)
    for me in (256, 4, 2):
        assert _capacity(codec, cov, me) == [BS.capacity(img, T, mv, me)] * 3, me


@pytest.mark.parametrize("name", _names("wide"))
def test_gpu_blind_wide(name):
    """W = 1032 (VEC: 129 items per row, 516 per full wave -- two full lane iterations and a ragged
    third of 4; the second wave has 2 rows) and 13 x 1030 (scalar: 515 candidates per row), with
    unsafe pixels past column 800.  i* and the capacity are read from codec_pee_blind_plan itself."""
    import torch
    from codec_tcc_amd import _lib, blind
    from codec_tcc_amd.codec import _stream
    img, T, mv, me, _ck, rows = _reference(name)
    H, W = img.shape
    if W % 8 == 0:
        assert 4 * (W // 8) == 2 * 256 + 4 and H // 2 == 4 + 2   # items of a full wave; rows of the second wave
    else:
        assert W // 2 == 515
    assert (rows[0][3]["i_star"], rows[0][3]["E"]) == (4, 4)
    if name == "wide_vec_u16":
        assert rows[0][0].size == 1914
    if name == "wide_scalar_u16":
        assert rows[0][0].size == 1932
    codec, cov, _stego = _run(name)
    B = len(rows)
    pw = blind.row_words(0, me)
    ws = blind._workspace(codec, pw, me)
    info = torch.full((B, _lib.BLIND_INFO_WORDS), -7, dtype=torch.int32, device=cov.device)
    lens = torch.tensor([r[0].size for r in rows], dtype=torch.int32, device=cov.device)
    _lib.check(_lib.load().codec_pee_blind_plan(C.byref(codec._params(pw)), cov.data_ptr(), lens.data_ptr(), me,
                                                info.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_plan")
    got = info.cpu().tolist()
    for b, (bits, _st, _info, p) in enumerate(rows):
        q = BS.plan(img, bits.size, T, mv, me)
        assert q["i_star"] == p["i_star"]
        assert got[b][:5] == [0, bits.size, q["E"], q["n_side"], -1], (b, got[b])   # `end` is the embed's to fill
        assert got[b][5:] == [q["rect"][0], q["i_star"], q["capacity"]], (b, got[b])


def _entry_words(stego, E):
    return [int(v) for v in BS.read_words(stego, BS.HDR_WORDS, E)]


@pytest.mark.parametrize("name", _names("many"))
def test_gpu_blind_many_entries(name):
    """300 planted pixels, max_entries = 65536, B = 3 with (cap, cap // 2, 0) bits so that E
    differs per slice.  uint16: E = 271 entries from a map of 275 words, 15 of them >= 16384 --
    k_blind_pack's second chunk behind a non-zero carry, entry slots >= 256 in pack and scatter.
    max_entries is the boundary at E, and the valid-prefix rule cuts blind_capacity at 256."""
    import torch
    img, T, mv, me, checksum, rows = _reference(name)
    bits0, st0, info0, p0 = rows[0]
    E = info0[2]
    assert len({r[2][2] for r in rows}) == 3
    if name == "many_u16":
        assert (bits0.size, E, info0[3], p0["r"], info0[4]) == (1937, 271, 8864, 17, 17543)
        assert E > 256 and (info0[4] + 64) >> 6 > 256
        ent = _entry_words(st0, E)
        assert ent == sorted(ent) and sum(v >= 16384 for v in ent) >= 1 and ent[-1] != BS.NO_ENTRY
    codec, cov, _stego = _run(name)
    assert _capacity(codec, cov, 65536) == [bits0.size] * 3
    assert _capacity(codec, cov, 256) == [BS.capacity(img, T, mv, 256)] * 3
    if name == "many_u16":
        assert BS.capacity(img, T, mv, 256) == 1786 and BS.capacity(img, T, mv, 65536) == 1937
    # max_entries = E embeds, E - 1 is status 2 and the cover goes through
    one = _codec(1, img.shape[0], img.shape[1], str(img.dtype), T, mv)
    _parity(one, img[None].copy(), [bits0], T, mv, checksum, E)
    c1 = torch.from_numpy(img[None].copy()).cuda()
    assert BS.embed(img, bits0, T, mv, checksum, E - 1)[1] == (2, bits0.size, E, 0, -1, 0)
    with pytest.raises(ValueError, match=r"max_entries in slices \[0\]"):
        one.embed_blind(c1, [bits0], checksum=checksum, max_entries=E - 1)
    stego, info = one.embed_blind(c1, [bits0], checksum=checksum, max_entries=E - 1, check=False)
    assert tuple(info.cpu().tolist()[0]) == (2, bits0.size, E, 0, -1, 0)
    np.testing.assert_array_equal(stego.cpu().numpy()[0], img)


def _with_entries(stego, entries):
    """A copy of the slice with its entry words rewritten (side words 6 ..: LSBs, backwards)."""
    out = stego.copy()
    H, W = out.shape
    idx = H * W - 1 - np.arange(32 * BS.HDR_WORDS, 32 * (BS.HDR_WORDS + len(entries)))
    flat = out.ravel()
    flat[idx] = (flat[idx] & ~np.asarray(1, out.dtype)) | BS.words_to_bits(entries).astype(out.dtype)
    return out


def _entry_variant(kind, ent, end, nc):
    """The rewritten entry list; slots >= 256 are touched wherever one entry changes."""
    ent = list(ent)
    if kind == "reversed":
        return ent[::-1]
    if kind == "duplicate":     # entry 259 over its neighbour's slot: entry 260 is lost
        ent[260] = ent[259]
    elif kind == "past_end":
        ent[0] = end + 1
    elif kind == "nc":
        ent[len(ent) - 1] = nc
    elif kind == "padding":     # a real entry turned into padding, in the middle of the list
        ent[258] = BS.NO_ENTRY
    return ent


@pytest.mark.parametrize("kind", ["reversed", "duplicate", "past_end", "nc", "padding"])
def test_gpu_blind_entry_rules(kind):
    """The decoder's entry rules against the spec's: entries are a set (order and duplicates do not
    matter), padding, entries beyond `end` and entries >= nc are ignored.  The spec's stego of the
    many-entry slice with its entry words rewritten decodes, with verify=False, to the spec's
    bits and cover -- the true ones for the reversed list, others where an entry is lost; under
    the header's CRC those raise IntegrityError naming the slice."""
    import torch
    from codec_tcc_amd import IntegrityError
    img, T, mv, _me, checksum, rows = _reference("many_u16")
    bits0, st0, info0, p = rows[0]
    E, end = info0[2], info0[4]
    H, W = img.shape
    nc = (H // 2) * (W // 2)
    assert checksum and E > 260 and end + 1 < (H // 2 - p["r"]) * (W // 2)
    ent = _entry_words(st0, E)
    new = _entry_variant(kind, ent, end, nc)
    assert len(new) == E and new != ent
    lost = set(ent) - set(new)
    assert len(lost) == (0 if kind == "reversed" else 1)
    bad = _with_entries(st0, new)
    assert _entry_words(bad, E) == new and [int(v) for v in BS.read_words(bad, 0, 6)] == [int(v) for v in BS.read_words(st0, 0, 6)]
    want_bits, want_cover, _hdr = BS.decode(bad, verify=False)
    if lost:
        assert not np.array_equal(want_cover, img)
    else:
        np.testing.assert_array_equal(want_cover, img)
        np.testing.assert_array_equal(want_bits, bits0)
    stack = np.stack([rows[1][1], bad, rows[2][1]])   # the rewritten slice between two good ones
    codec = _codec(3, H, W, str(img.dtype), T, mv)
    dev = torch.from_numpy(stack).cuda()
    out, back = codec.decode_blind(dev, verify=False)
    np.testing.assert_array_equal(out[1], want_bits)
    np.testing.assert_array_equal(back.cpu().numpy()[1], want_cover)
    for b, r in ((0, rows[1]), (2, rows[2])):
        np.testing.assert_array_equal(out[b], r[0])
        np.testing.assert_array_equal(back.cpu().numpy()[b], img)
    if lost:
        with pytest.raises(ValueError):
            BS.decode(bad)
        with pytest.raises(IntegrityError) as ei:
            codec.decode_blind(dev)
        assert ei.value.bad_cover == [1]
    else:
        out, back = codec.decode_blind(dev)
        np.testing.assert_array_equal(out[1], bits0)
        np.testing.assert_array_equal(back.cpu().numpy()[1], img)


@pytest.mark.parametrize("name", _names("long"))
def test_gpu_blind_long_payload(name):
    """512 x 512, B = 2 with (cap, 20000) bits: more than 16384 payload-row bits in both slices, so
    displaced and user bits cross into k_blind_splice's and k_blind_restore's second block, and
    at capacity a map of more than 768 words (four chunks of k_blind_pack)."""
    _img, _T, _mv, _me, _ck, rows = _reference(name)
    assert [r[0].size for r in rows][1] == 20000 and rows[0][0].size > 20000
    for bits, _st, info, _p in rows:
        assert info[0] == 0 and info[3] + bits.size > 16384
    assert (rows[0][2][4] + 64) >> 6 > 768
    if name == "long_u16":
        assert [(r[0].size, r[2][2], r[2][4]) for r in rows] == [(41843, 19, 65279), (20000, 18, 29466)]
    _run(name)


@pytest.mark.parametrize("name", _names("narrow"))
def test_gpu_blind_narrow(name):
    """Flat mid-grey slices at T = 2 with wc = 1 (600 x 2, r = 48), W = 3 (r = 32), W = 8 (one vector
    item per row; the header fits and nothing else), W = 9, and slices too small for a header's
    worth of candidates (14 x 14, 28 x 14, 2 x 96 with hc = 1: capacity -1).  PeeCodec refuses none
    of these shapes, so each runs: blind_capacity is the spec's, capacity bits embed and round-trip,
    one more is status 1 and the cover goes through."""
    import torch
    img, T, mv, me, checksum, rows = _reference(name)
    cap = CS.shape_case(name)[6]
    H, W = img.shape
    assert cap == CS.SHAPE_CAPACITY[name] == BS.capacity(img, T, mv, me)
    if name == "narrow_600x2":
        assert rows[0][3]["r"] == 48 and W // 2 == 1
    if name == "narrow_601x3":
        assert rows[0][3]["r"] == 32
    codec = _codec(1, H, W, str(img.dtype), T, mv)
    covers = img[None].copy()
    cov = torch.from_numpy(covers).cuda()
    assert _capacity(codec, cov, me) == [cap]
    if cap >= 0:
        assert rows[0][0].size == cap
        _parity(codec, covers, [rows[0][0]], T, mv, checksum, me, want=[(rows[0][1], rows[0][2])])
    over, st, info, _p = rows[-1]
    assert over.size == cap + 1 and info == (1, cap + 1, 0, 0, -1, 0)
    np.testing.assert_array_equal(st, img)
    with pytest.raises(ValueError, match=r"capacity in slices \[0\]"):
        codec.embed_blind(cov, [over], checksum=checksum, max_entries=me)
    stego, ginfo = codec.embed_blind(cov, [over], checksum=checksum, max_entries=me, check=False)
    assert tuple(ginfo.cpu().tolist()[0]) == info
    np.testing.assert_array_equal(stego.cpu().numpy()[0], img)
    np.testing.assert_array_equal(cov.cpu().numpy(), covers)
