"""MED-PEE side records that are NOT what our own embed just wrote: records built from the
oracle's side dicts, from file headers, and records whose fields disagree.

Host half (no GPU): pee.check_records accepts every record the oracle writes and rejects
every single-field mutant; pipeline.read_pee_bytes turns any truncated or inconsistent file
into ValueError before a launch.  GPU half: files written by the oracle decode to the
oracle's bits and cover (every other file test decodes what the GPU encoded), and every
extract kernel follows the oracle on a record whose L is understated or whose `end` lies
beyond its lattice (include/codec_tcc.h, record contract).

None of the GPU tests aims at a fault: each is built so that a kernel without the bound would
fail an assertion while writing only into memory the test allocated (the arithmetic is in
the docstrings).
"""
import os
import re
import struct
import zlib

import numpy as np
import pytest

from codec_tcc_amd import container, framing, pipeline, synth
from codec_tcc_amd.pee import _check_multi_args, check_records, lattice_geometry, make_record
from oracle import pee_cpu as P

from test_pee import _kat_inputs, _kats, _multi_kat_inputs, _multi_kats

SHAPES = [(3, 2), (2, 9), (9, 2), (8, 8), (9, 7), (16, 16), (33, 41)]
KINDS = {"u8": (np.uint8, 255), "ct12": (np.uint16, 4095), "u16": (np.uint16, 65535)}
RULES = ["zero", "half", "cap", "over", "cap0_left"]


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def _image(kind, h, w, seed):
    """A cover with a useful capacity at small T: a ramp plus noise of a few grey levels
    (synth.ct12's noise leaves ~5 % of the candidates expandable at T = 2)."""
    dtype, mv = KINDS[kind]
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (mv // 3 + 3 * y + 2 * x) % (mv - 40) + 20
    if kind == "u16":   # full range: some candidates expand, many shift, a few overflow
        img = np.where(rng.random((h, w)) < 0.15, rng.integers(0, 65536, (h, w)), base + rng.integers(0, 4, (h, w)))
    else:
        img = base + rng.integers(0, 4, (h, w))
    return np.clip(img, 0, mv).astype(dtype)


def _lm_words(h, w):
    return max(1, ((h // 2) * (w // 2) + 63) // 64)


def _records(side, h, w, scheme):
    """[pass][slice] records of one slice from an oracle side dict."""
    passes = side["passes"] if scheme == 2 else [side]
    return [[make_record(h, w, T=ps["T"], maxval=ps["maxval"], L=ps["L"], end=ps["end"], status=ps["status"],
                         lattice=p)] for p, ps in enumerate(passes)]


def _check(recs, h, w, scheme, nbytes, total, *, payload_words=None, lm_words=None, lengths="sum"):
    pw = max(1, (total + 63) // 64) if payload_words is None else payload_words
    check_records(recs, h, w, scheme=scheme, payload_words=pw, lm_words=_lm_words(h, w) if lm_words is None else lm_words,
                  bytes=nbytes, lengths=([total] if lengths == "sum" else lengths) if scheme == 2 else None)


def _embed_oracle(img, bits, T, mv, scheme):
    if scheme == 2:
        return P.pee_embed_multi(img, bits, T, maxval=mv)
    return P.pee_embed(img, bits, T, maxval=mv, truncate=True)


def _capacity(img, T, mv, scheme):
    if scheme == 2:
        return P.pee_embed_multi(img, _bits(img.size, 1), T, maxval=mv)[1]["L"]
    return P.capacity(img, T, mv)


def _payload(rule, img, T, mv, scheme, seed):
    cap = _capacity(img, T, mv, scheme)
    n = {"zero": 0, "half": cap // 2, "cap": cap, "over": cap + 9, "cap0_left": 5}[rule]
    return _bits(n, seed)


# ------------------------------------------------------------------ CPU: no false rejects
def test_check_records_accepts_every_oracle_record():
    """Records built from the oracle's side dicts -- every known-answer input of both schemes and
    a seeded sweep of small shapes, three pixel types and five payload rules (`cap0_left`: a
    saturated cover, capacity 0, bits left over: L = 0, end = nc - 1, status 1) -- all pass.
    Nothing is skipped: the number checked equals the number generated."""
    generated = checked = 0
    for k in _kats():
        img, bits, mv = _kat_inputs(k)
        generated += 1
        _st, side = P.pee_embed(img, bits, k["T"], maxval=mv, truncate=True)
        _check(_records(side, *img.shape, 1), *img.shape, 1, img.dtype.itemsize, side["L"])
        checked += 1
    for k in _multi_kats():
        img, bits, mv = _multi_kat_inputs(k)
        generated += 1
        _st, side = P.pee_embed_multi(img, bits, k["T"], maxval=mv)
        _check(_records(side, *img.shape, 2), *img.shape, 2, img.dtype.itemsize, side["L"])
        checked += 1
    seen_cap0 = 0
    for si, (h, w) in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            dtype, mv = KINDS[kind]
            for ri, rule in enumerate(RULES):
                for scheme in (1, 2):
                    generated += 1
                    seed = 1000 * si + 100 * ki + 10 * ri + scheme
                    T = 1 + seed % 3
                    img = np.full((h, w), mv, dtype) if rule == "cap0_left" else _image(kind, h, w, seed)
                    bits = _payload(rule, img, T, mv, scheme, seed)
                    _st, side = _embed_oracle(img, bits, T, mv, scheme)
                    if rule == "cap0_left":
                        assert side["L"] == 0 and side["status"] == 1
                        seen_cap0 += 1
                    _check(_records(side, h, w, scheme), h, w, scheme, img.dtype.itemsize, side["L"])
                    checked += 1
    assert generated == checked == len(_kats()) + len(_multi_kats()) + len(SHAPES) * len(KINDS) * len(RULES) * 2
    assert seen_cap0 == len(SHAPES) * len(KINDS) * 2


# ------------------------------------------------------------------ CPU: mutation table
def _mutant(recs, p, field, value, fix_tile=True):
    """A copy of the record set with one field of pass p changed (`end`: tile_end follows, so
    that the rejection is `end`'s own)."""
    out = [[type(r).from_buffer_copy(bytes(r)) for r in pr] for pr in recs]
    r = out[p][0]
    if field == "reserved0":
        r.reserved[0] = value
    else:
        setattr(r, field, value)
    if field == "end" and fix_tile:
        r.tile_end = value // 1024 if value >= 0 else -1
    return out


def test_check_records_rejects_every_single_field_mutant():
    """One field at a time set to each forbidden value, from valid scheme-1 and scheme-2 record
    sets at 16 x 16 (lm_words = 1: 64 map bits; nc = 64, 49, 56, 56) and 33 x 41 (nc_0 = 320):
    every mutant raises ValueError naming the field.  Among them `end = nc_p` for lattices 1..3,
    which the map's 64 bits do not catch (49, 56 < 64)."""
    h = w = 16
    mv, T = 4095, 2
    img = _image("ct12", h, w, 5)
    ncs = [hc * wc for _y, _x, hc, wc in (lattice_geometry(p, h, w) for p in range(4))]
    assert ncs == [64, 49, 56, 56] and _lm_words(h, w) == 1
    mutants = []   # (label, records, kwargs of _check)

    def add(label, recs, scheme, total, **kw):
        mutants.append((label, recs, scheme, total, kw))

    # scheme 1, a pass that stopped half way (status 0) and one that filled up (status 1)
    cap = P.capacity(img, T, mv)
    assert cap >= 8
    _st, half = P.pee_embed(img, _bits(cap // 2, 1), T, maxval=mv, truncate=True)
    _st, over = P.pee_embed(img, _bits(cap + 9, 2), T, maxval=mv, truncate=True)
    r_half, r_over = _records(half, h, w, 1), _records(over, h, w, 1)
    _check(r_half, h, w, 1, 2, half["L"])
    _check(r_over, h, w, 1, 2, over["L"])
    assert half["status"] == 0 and 0 <= half["end"] < 63 and over["status"] == 1 and over["end"] == 63
    nc = 64
    for field, values in (("T", [0, -1, 65]), ("maxval", [0, -1, 65536]), ("h", [h + 1, 0]), ("w", [w - 1, w + 2]),
                          ("nc", [nc + 1, nc - 1]), ("ntiles", [0, 2]), ("status", [3, -1]),
                          ("L", [half["end"] + 2, -1, 0, 2 ** 31 - 1]), ("end", [nc, -1, -2, half["L"] - 2, 2 ** 31 - 1]),
                          ("tile_end", [-1, 1])):
        for v in values:
            add(f"s1.{field}={v}", _mutant(r_half, 0, field, v), 1, half["L"])
    for field, values in (("end", [nc - 2, nc, -1]), ("L", [nc + 1, -1]), ("tile_end", [-1, 1])):
        for v in values:
            add(f"s1.full.{field}={v}", _mutant(r_over, 0, field, v), 1, over["L"])
    add("s1.maxval>u8", _mutant(r_half, 0, "maxval", 256), 1, half["L"], nbytes=1)

    # scheme 2: for every lattice p a valid set whose last embedding pass is p (status 0 there)
    caps = [ps["capacity"] for ps in P.pee_embed_multi(img, _bits(h * w, 3), T, maxval=mv)[1]["passes"]]
    assert min(caps) >= 4
    for p in range(4):
        n = sum(caps[:p]) + caps[p] // 2
        _st, side = P.pee_embed_multi(img, _bits(n, 10 + p), T, maxval=mv)
        recs = _records(side, h, w, 2)
        _check(recs, h, w, 2, 2, side["L"])
        ps = side["passes"][p]
        assert ps["status"] == 0 and 1 <= ps["L"] <= ps["end"] + 1 <= ncs[p]
        add(f"s2.p{p}.end=nc", _mutant(recs, p, "end", ncs[p]), 2, side["L"])
        add(f"s2.p{p}.end=63+1", _mutant(recs, p, "end", 64), 2, side["L"])
        add(f"s2.p{p}.L=end+2", _mutant(recs, p, "L", ps["end"] + 2), 2, side["L"], lengths=None)
        add(f"s2.p{p}.tile_end+1", _mutant(recs, p, "tile_end", 1), 2, side["L"])
        add(f"s2.p{p}.tile_end-1", _mutant(recs, p, "tile_end", -1), 2, side["L"])
        add(f"s2.p{p}.reserved0", _mutant(recs, p, "reserved0", (p + 1) % 4), 2, side["L"])
        add(f"s2.p{p}.T=0", _mutant(recs, p, "T", 0), 2, side["L"])
        add(f"s2.p{p}.nc", _mutant(recs, p, "nc", ncs[p] + 1), 2, side["L"])
        add(f"s2.p{p}.sum+1", recs, 2, side["L"], lengths=[side["L"] + 1])
        add(f"s2.p{p}.sum-1", recs, 2, side["L"], lengths=[side["L"] - 1])
        if p < 3:   # a later pass embeds although pass p did not fill up
            late = _mutant(_mutant(recs, p + 1, "L", 1), p + 1, "end", 0)
            add(f"s2.p{p}.late_bits", late, 2, side["L"], lengths=None)
        if p > 0:   # an earlier pass claims it stopped early
            add(f"s2.p{p}.early_status", _mutant(recs, p - 1, "status", 0), 2, side["L"])
    # all four passes filled up: `end` must be each lattice's last candidate
    _st, full = P.pee_embed_multi(img, _bits(h * w, 4), T, maxval=mv)
    r_full = _records(full, h, w, 2)
    _check(r_full, h, w, 2, 2, full["L"])
    for p in range(4):
        add(f"s2.full.p{p}.end=nc", _mutant(r_full, p, "end", ncs[p]), 2, full["L"])
        add(f"s2.full.p{p}.end=nc-2", _mutant(r_full, p, "end", ncs[p] - 2), 2, full["L"])

    # the buffers' sizes (33 x 41: nc_0 = 320, 5 map words)
    big = _image("ct12", 33, 41, 6)
    capb = P.capacity(big, T, mv)
    assert capb > 130
    _st, sb = P.pee_embed(big, _bits(capb - 1, 7), T, maxval=mv, truncate=True)
    rb = _records(sb, 33, 41, 1)
    _check(rb, 33, 41, 1, 2, sb["L"])
    assert sb["L"] > 128 and sb["end"] >= 128
    for label, kw in (("payload_words", dict(payload_words=(sb["L"] + 63) // 64 - 1)), ("payload_words=0", dict(payload_words=0)),
                      ("lm_words", dict(lm_words=sb["end"] // 64)), ("lm_words=0", dict(lm_words=0)), ("bytes", dict(nbytes=3))):
        mutants.append((f"args.{label}", rb, 1, sb["L"], dict(kw, hw=(33, 41))))

    rejected = 0
    for label, recs, scheme, total, kw in mutants:
        kw = dict(kw)
        hh, ww = kw.pop("hw", (h, w))
        nbytes = kw.pop("nbytes", 2)
        with pytest.raises(ValueError):
            _check(recs, hh, ww, scheme, nbytes, total, **kw)
            pytest.fail(f"mutant {label} was accepted")
        rejected += 1
    assert rejected == len(mutants) and len(mutants) > 90


def test_check_records_names_slice_pass_and_field():
    h = w = 16
    img = _image("ct12", h, w, 5)
    _st, side = P.pee_embed_multi(img, _bits(h * w, 4), 2, maxval=4095)
    recs = _records(side, h, w, 2)
    two = [[pr[0], _mutant(recs, 1, "end", 49)[p][0]] for p, pr in enumerate(recs)]   # slice 1 is the mutant
    with pytest.raises(ValueError, match=r"slice 1, pass 1: end = 49"):
        check_records(two, h, w, scheme=2, payload_words=4, lm_words=1, bytes=2)
    flat = [pr[0] for pr in recs]   # PeeEncoded.records()' flat pass-major list is taken too
    check_records(flat, h, w, scheme=2, payload_words=4, lm_words=1, bytes=2, lengths=[side["L"]])


# ------------------------------------------------------------------ CPU: files the oracle wrote
def _oracle_file(img, bits, T, mv, scheme):
    """(file bytes, stego, side, header format, header values) of a version-16 file written from
    the oracle's embedding alone (raw stego codec)."""
    h, w = img.shape
    st, side = _embed_oracle(img, bits, T, mv, scheme)
    if scheme == 1:
        blobs = [container.lm_blob(side["lm"]) if side["end"] >= 0 else b""]
        hdr = container.create_pee_header("raw", img.dtype.itemsize, w, h, T, side["L"], side["end"], mv, side["status"],
                                          len(blobs[0]))
        fmt = container._PEE_FMT
    else:
        blobs = [container.lm_blob(ps["lm"]) if ps["end"] >= 0 else b"" for ps in side["passes"]]
        hdr = container.create_pee2_header("raw", img.dtype.itemsize, w, h, T, mv, side["L"], side["status"],
                                           [(ps["L"], ps["end"], ps["status"], len(b)) for ps, b in zip(side["passes"], blobs)])
        fmt = container._PEE2_FMT + container._PEE2_PASS[1:] * 4
    body = b"".join(blobs) + container.encode_stego_raw(st)
    return _frame(hdr, body), st, side, fmt, list(struct.unpack(fmt, hdr)), body


def _frame(hdr, body):
    return container.MAGIC + struct.pack(">I", len(hdr)) + hdr + body


FILES = [(1, "ct12", 16, 16), (2, "u8", 9, 7)]


def _file_case(scheme, kind, h, w):
    _dtype, mv = KINDS[kind]
    img = _image(kind, h, w, 21)
    img[1::2, 1::4] = mv            # saturated candidates: a location map with set bits
    bits = _bits(_capacity(img, 2, mv, scheme) // 2 + 1, 22)
    return (img, bits, mv) + _oracle_file(img, bits, 2, mv, scheme)


def _host_half(raw):
    """'rejected' for ValueError, 'accepted' for records that pass check_records; any other
    exception propagates and fails the test."""
    try:
        pf = pipeline.read_pee_bytes(raw)
    except ValueError:
        return "rejected"
    h, w = pf.stego.shape
    check_records(pf.records, h, w, scheme=pf.scheme, payload_words=pf.payload_words, lm_words=pf.lm_words,
                  bytes=pf.stego.dtype.itemsize, lengths=[pf.md["L"]] if pf.scheme == 2 else None)
    assert pf.lm.shape == (len(pf.records), 1, 64 * pf.lm_words) and pf.payload_words * 64 >= pf.md["L"]
    return "accepted"


@pytest.mark.parametrize("scheme,kind,h,w", FILES)
def test_oracle_file_host_half_and_prefixes(scheme, kind, h, w):
    """The host half reads the oracle's file back (records, map bits, stego); every proper
    prefix of the file raises ValueError and nothing else."""
    img, bits, mv, raw, st, side, _fmt, _vals, _body = _file_case(scheme, kind, h, w)
    pf = pipeline.read_pee_bytes(raw)
    np.testing.assert_array_equal(pf.stego, st)
    passes = side["passes"] if scheme == 2 else [side]
    assert any(ps["lm"].any() for ps in passes)
    for p, ps in enumerate(passes):
        r = pf.records[p][0]
        assert (r.L, r.end, r.status, r.T, r.maxval) == (ps["L"], ps["end"], ps["status"], 2, mv)
        np.testing.assert_array_equal(pf.lm[p, 0, : ps["end"] + 1], ps["lm"])
        assert not pf.lm[p, 0, ps["end"] + 1:].any()
    assert pf.payload_words == max(1, (side["L"] + 63) // 64)
    for n in range(len(raw)):
        with pytest.raises(ValueError):
            pipeline.read_pee_bytes(raw[:n])


@pytest.mark.parametrize("scheme,kind,h,w", FILES)
def test_oracle_file_header_field_mutants(scheme, kind, h, w):
    """Every header field set to each of -2, -1, 0, 2^31 - 1 and its own value +- 1 (unsigned
    fields take the value modulo their width): the host half raises ValueError or yields
    records that pass check_records -- nothing else, and nothing reaches a launch.  The codec id
    is left alone: its other values select an external stego decoder, whose absence is a
    RuntimeError by design (pipeline._decompress)."""
    _img, _bits_, _mv, raw, _st, _side, fmt, vals, body = _file_case(scheme, kind, h, w)
    codes = [c for c in fmt if c.isalpha()]
    assert len(codes) == len(vals) == (12 if scheme == 1 else 26)
    assert _host_half(raw) == "accepted"
    count = {"accepted": 0, "rejected": 0}
    for i, c in enumerate(codes):
        if i == 1:
            continue
        for v in (-2, -1, 0, 2 ** 31 - 1, vals[i] - 1, vals[i] + 1):
            if v == vals[i] or (c == "i" and not -2 ** 31 <= v < 2 ** 31):
                continue
            mut = list(vals)
            mut[i] = v & 0xFF if c == "B" else (v & 0xFFFFFFFF if c == "I" else v)
            count[_host_half(_frame(struct.pack(fmt, *mut), body))] += 1
    assert count["rejected"] > 3 * len(codes) and count["accepted"] >= 1   # e.g. L - 1: an understated L is legal
    # the header length itself: too short for the fields, or longer than the file
    hdr = struct.pack(fmt, *vals)
    for bad in (_frame(hdr[:-1], body), container.MAGIC + struct.pack(">I", len(hdr) + len(body) + 1) + hdr + body):
        assert _host_half(bad) == "rejected"


@pytest.mark.parametrize("scheme,kind,h,w", FILES)
def test_oracle_file_bad_location_map_blobs(scheme, kind, h, w):
    """A corrupted location-map blob (not zlib; a wrong checksum; a truncated stream), one that
    inflates to fewer bits than end + 1 and one that inflates without bound each raise
    ValueError; lm_from_blob inflates no more than the bytes it needs."""
    _img, _b, _mv, raw, st, side, fmt, vals, body = _file_case(scheme, kind, h, w)
    ps = (side["passes"] if scheme == 2 else [side])[0]
    size_i = 11 if scheme == 1 else 13            # pass 0's blob size field
    blob = body[: vals[size_i]]
    assert ps["end"] >= 8 and blob == container.lm_blob(ps["lm"])
    rest = body[len(blob):]
    bomb = zlib.compress(b"\0" * 50_000_000, 9)
    assert len(bomb) < 100_000
    for label, new in (("zeros", b"\0" * len(blob)), ("checksum", blob[:-1] + bytes([blob[-1] ^ 0x55])),
                       ("cut stream", blob[:-3]), ("fewer bits", container.lm_blob(ps["lm"][:-8])),
                       ("more bits", container.lm_blob(np.concatenate([ps["lm"], np.zeros(16, bool)]))), ("bomb", bomb)):
        mut = list(vals)
        mut[size_i] = len(new)
        with pytest.raises(ValueError):
            pipeline.read_pee_bytes(_frame(struct.pack(fmt, *mut), new + rest))
            pytest.fail(f"blob mutant '{label}' was accepted")
        with pytest.raises(ValueError):
            container.lm_from_blob(new, ps["end"])
    np.testing.assert_array_equal(container.lm_from_blob(blob, ps["end"]), ps["lm"])
    assert container.lm_from_blob(bomb, -1).size == 0


def test_extract_multi_argument_shapes():
    """Scheme 2's extract takes lm [4, B, lm_words], meta [4, B, PEE_META_BYTES] and a payload of
    at least [B, payload_words] (rows payload_words apart): scheme-1-shaped tensors, which would
    make the library read 4 * B records past them, are refused before any launch."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import _lib
    B, lmw, pw = 3, 2, 5
    meta = torch.zeros((4, B, _lib.PEE_META_BYTES), dtype=torch.uint8)
    lm = torch.zeros((4, B, lmw), dtype=torch.int64)
    pay = torch.zeros((B, pw), dtype=torch.int64)
    _check_multi_args(B, lmw, meta, lm, payload=pay, payload_words=pw)
    _check_multi_args(1, lmw, meta[:, :1].contiguous(), lm[:, :1].contiguous(), payload=torch.zeros((1, 17), dtype=torch.int64)[:, :1],
                      payload_words=1)
    bad = [dict(meta=meta[0]), dict(lm=lm[0]), dict(meta=meta[:, :2].contiguous()), dict(lm=lm[:, :, :1].contiguous()),
           dict(lm=lm.transpose(0, 1).contiguous().transpose(0, 1)), dict(lm=lm.to(torch.int32)),
           dict(payload=pay[:, : pw - 1]), dict(payload=pay[:2]), dict(payload=pay[0]), dict(payload=pay.to(torch.int32)),
           dict(payload=torch.zeros((B, pw + 1), dtype=torch.int64)[:, :pw]), dict(payload_words=0)]
    for kw in bad:
        args = dict(meta=meta, lm=lm, payload=pay, payload_words=pw)
        args.update(kw)
        with pytest.raises(ValueError):
            _check_multi_args(B, lmw, args["meta"], args["lm"], payload=args["payload"], payload_words=args["payload_words"])


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(16, 16), (9, 7), (33, 41), (3, 2)])
@pytest.mark.parametrize("kind", ["u8", "ct12"])
@pytest.mark.parametrize("scheme", [1, 2])
def test_gpu_decodes_files_the_oracle_wrote(scheme, kind, h, w, tmp_path):
    """Cross-implementation decode: decode_bin_pee on files written from the oracle's embedding
    alone (payload half the capacity, the capacity, beyond it) returns the oracle's bits and the
    original cover."""
    pytest.importorskip("torch")
    _dtype, mv = KINDS[kind]
    img = _image(kind, h, w, 31)
    if h >= 9:
        img[1::2, 1::4] = mv
    for rule in ("half", "cap", "over"):
        bits = _payload(rule, img, 2, mv, scheme, 32)
        raw, st, side = _oracle_file(img, bits, 2, mv, scheme)[:3]
        path = str(tmp_path / f"{rule}.bin")
        with open(path, "wb") as f:
            f.write(raw)
        got, cover = pipeline.decode_bin_pee(path)
        exp_bits, exp_cover = (P.pee_extract_multi if scheme == 2 else P.pee_extract)(st, side)
        np.testing.assert_array_equal(exp_cover, img)
        np.testing.assert_array_equal(got, exp_bits)
        np.testing.assert_array_equal(got, bits[: side["L"]])
        np.testing.assert_array_equal(cover, img)


# every scheme-1 extract path, selected as tests/test_pee.py's PATHS do, at 64 x 64 (8 | W, 256
# items: the smallest shape the fused sweep and the single pass take)
X_PATHS = {"tile": {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_FUSED": "0"},
           "tile_scalar": {"CODEC_PEE_ONEPASS": "0", "CODEC_PEE_FUSED": "0", "_w": "62"},
           "gs": {"CODEC_PEE_ONEPASS": "0"},
           "onepass_selfclean": {"CODEC_PEE_ONEPASS": "1"},
           "onepass_zeroing": {"CODEC_PEE_ONEPASS": "1", "CODEC_PEE_SELFCLEAN": "0"},
           "onepass_lanes": {"CODEC_PEE_ONEPASS": "1", "CODEC_PEE_FLAT_MAXB": "0"},
           "slice_serial": {"CODEC_PEE_SS": "1"}}


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("path", sorted(X_PATHS))
def test_gpu_understated_L_follows_the_oracle(path, inplace, monkeypatch):
    """A record whose L is smaller than the embedding's (here 64 of 600 bits, payload_words = 1):
    the oracle's pee_extract returns bits[:L], so word 0 holds the first 64 bits, nothing is
    written past it and the cover is restored whole -- on every scheme-1 extract path.

    Memory: the payload row is the first word of a zeroed [1, 17] buffer.  A kernel without the
    bound writes one bit per inner candidate, at most nc = 32 * 32 = 1024 (31 * 32 at W = 62)
    bits, i.e. words 0 .. 1023 // 64 = 15: inside the buffer, where the test sees them (words
    1 .. 16 must still be zero)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import _lib
    from codec_tcc_amd.pee import PeeCodec
    env = dict(X_PATHS[path])
    h, w, T, mv = 64, int(env.pop("_w", 64)), 4, 4095
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img = _image("ct12", h, w, 41)
    bits = _bits(600, 42)
    assert (h // 2) * (w // 2) <= 1024 and P.capacity(img, T, mv) >= 600
    st, side = P.pee_embed(img, bits, T, maxval=mv)
    codec = PeeCodec(1, h, w, dtype="uint16", T=T, maxval=mv)
    enc = codec.embed(torch.from_numpy(img[None]).cuda(), [bits])
    np.testing.assert_array_equal(enc.stego.cpu().numpy()[0], st)
    rec = enc.records()[0]
    assert (rec.L, rec.end, rec.status) == (600, side["end"], 0)
    rec.L = 64
    check_records([rec], h, w, scheme=1, payload_words=1, lm_words=codec.lm_words, bytes=2)   # a legal record
    meta = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).view(1, -1).cuda()
    buf = torch.zeros((1, 17), dtype=torch.int64, device="cuda")
    work = enc.stego.clone()
    _words, cover = codec.extract(work, meta, enc.lm, payload_words=1, payload=buf[:, :1], cover=work if inplace else None)
    host = buf.cpu().numpy()[0]
    exp_bits, exp_cover = P.pee_extract(st, dict(side, L=64))
    assert exp_bits.size == 64
    print(f"{path}: words written past the row: {np.flatnonzero(host[1:]).tolist()}")
    np.testing.assert_array_equal(framing.unpack_bits(host[:1], 64), exp_bits)
    np.testing.assert_array_equal(framing.unpack_bits(host[:1], 64), bits[:64])
    assert not host[1:].any(), "payload words past payload_words were written"
    np.testing.assert_array_equal(cover.cpu().numpy()[0], img)
    np.testing.assert_array_equal(exp_cover, img)
    assert not codec.lookback_failed(1)


@pytest.mark.gpu
@pytest.mark.parametrize("ss", ["tile", "ss"])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_gpu_end_beyond_the_lattice_is_clamped(p, ss, monkeypatch):
    """Scheme 2 at 16 x 16, pass p's record with end = 63 although its lattice has nc_p = 49 or
    56 candidates (the map's 64 bits allow it; check_records refuses it, so the record goes to
    extract() directly): the kernels take end as nc_p - 1 -- the result equals the oracle's with
    that pass's end set to nc_p - 1, and the slices either side of the image are untouched.

    Memory: the image is the middle slice of a [3, 16, 16] buffer, extracted in place.  Without
    the clamp a candidate k <= 63 of a lattice with wc >= 7 lies in row <= 2 + 2 * (63 // 7) = 20
    and column <= 15, i.e. at most 20 * 16 + 15 = 335 elements into the 256-element slice: inside
    the third slice, where the sentinel comparison sees it; its neighbours lie above and to the
    left, never before the slice.  tile_end = 63 // 1024 = 0 is the slice's one tile slot, the
    map word is word 0 of lm_words = 1, the slice-serial kernel walks 63 // 4096 + 1 = 1 chunk,
    and both kernels' LDS is static and indexed by thread and payload rank only."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_LAT_SS", "0" if ss == "tile" else "1")
    h = w = 16
    T, mv = 2, 4095
    img = _image("ct12", h, w, 51)
    caps = [ps["capacity"] for ps in P.pee_embed_multi(img, _bits(h * w, 3), T, maxval=mv)[1]["passes"]]
    bits = _bits(sum(caps[:p]) + caps[p] // 2, 52)          # pass p stops half way
    st, side = P.pee_embed_multi(img, bits, T, maxval=mv)
    _y0, _x0, hc, wc = lattice_geometry(p, h, w)
    nc = hc * wc
    assert nc in (49, 56) and wc >= 7 and side["passes"][p]["status"] == 0 and side["passes"][p]["end"] < nc - 1
    recs = _records(side, h, w, 2)
    recs[p][0].end = 63                                      # tile_end stays 0
    with pytest.raises(ValueError, match=f"pass {p}: end = 63"):
        _check(recs, h, w, 2, 2, side["L"])
    lm = np.zeros((4, 1, 64), dtype=bool)
    for q, ps in enumerate(side["passes"]):
        lm[q, 0, : ps["end"] + 1] = ps["lm"]
    clamped = dict(side, passes=[dict(ps) for ps in side["passes"]])
    clamped["passes"][p]["end"] = nc - 1
    clamped["passes"][p]["lm"] = lm[p, 0, :nc]
    # pee_extract_multi's passes one by one: pass q's bits belong at offset L_0 + .. + L_{q-1} of
    # the payload row (include/codec_tcc.h).  The over-long pass restores candidates that were
    # never embedded, so an earlier pass may find fewer than L_q inner candidates on those
    # pixels; pee_extract_multi would close the gap by concatenating, the row keeps the offsets
    exp_cover, exp_row, base = st, np.zeros(side["L"], np.uint8), [0]
    for ps in clamped["passes"]:
        base.append(base[-1] + ps["L"])
    for q in (3, 2, 1, 0):
        got_q, exp_cover = P.pee_extract(exp_cover, clamped["passes"][q])
        exp_row[base[q]: base[q] + got_q.size] = got_q
    assert np.array_equal(exp_cover, P.pee_extract_multi(st, clamped)[1])
    sentinel = 0xA5A5
    host3 = np.full((3, h, w), sentinel, np.uint16)
    host3[1] = st
    buf = torch.from_numpy(host3).cuda()
    view = buf[1:2]
    meta = torch.frombuffer(bytearray(b"".join(bytes(pr[0]) for pr in recs)), dtype=torch.uint8).view(4, 1, -1).cuda()
    lm_t = torch.from_numpy(np.packbits(lm, axis=-1, bitorder="little").view(np.int64).copy()).cuda()
    pw = max(1, (side["L"] + 63) // 64)
    codec = PeeCodec(1, h, w, dtype="uint16", T=T, maxval=mv, scheme=2)
    words, cover = codec.extract(view, meta, lm_t, payload_words=pw, cover=view)
    out = buf.cpu().numpy()
    assert (out[0] == sentinel).all() and (out[2] == sentinel).all(), "a write outside the image"
    np.testing.assert_array_equal(out[1], exp_cover)
    np.testing.assert_array_equal(framing.unpack_bits(words.cpu().numpy()[0], side["L"]), exp_row)
    assert not framing.unpack_bits(words.cpu().numpy()[0], 64 * pw)[side["L"]:].any()


def _lss_pay_maxw():
    """LSS_PAY_MAXW of codec_pee.hip (the payload words the slice-serial kernel stages in LDS)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "codec_tcc_amd", "csrc",
                            "codec_pee.hip")).read()
    pad = re.search(r"#define LSS_PAD_WORDS \((\d+) \* 1024\)", src)
    base = re.search(r"#define LSS_PAY_BASE (\d+)", src)
    assert pad and base and re.search(r"#define LSS_PAY_MAXW \(\(LSS_PAD_WORDS - LSS_PAY_BASE\) / 2\)", src)
    return (int(pad.group(1)) * 1024 - int(base.group(1))) // 2


@pytest.mark.gpu
def test_gpu_lat_ss_without_prefetch_takes_long_payload_rows(monkeypatch):
    """CODEC_PEE_LAT_SS_PF=0 (the no-prefetch A/B launch) with a uint16 batch whose payload row is
    longer than the LDS staging area: the launch must not stage it (it did, unconditionally);
    embed and extract equal the oracle.  64 x 96 with one 700 000-bit payload, the shape and row
    tests/test_pee2_auto.py's global-payload test uses (the long slice truncates)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd.pee import PeeCodec
    monkeypatch.setenv("CODEC_PEE_LAT_SS", "1")
    monkeypatch.setenv("CODEC_PEE_LAT_SS_PF", "0")
    h, w, T, mv = 64, 96, 2, 4095
    covers = np.stack([synth.ct12(h, w, 300 + i) for i in range(3)])
    bits_list = [_bits(100, 61), _bits(700_000, 62), _bits(0, 63)]
    codec = PeeCodec(3, h, w, dtype="uint16", T=T, maxval=mv, scheme=2)
    enc = codec.embed(torch.from_numpy(covers).cuda(), bits_list)
    assert enc.payload_words == (700_000 + 63) // 64 > _lss_pay_maxw()
    st = enc.stego.cpu().numpy()
    prs = enc.pass_records()
    words, cover = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    host = words.cpu().numpy()
    for b in range(3):
        exp, side = P.pee_embed_multi(covers[b], bits_list[b], T, maxval=mv)
        np.testing.assert_array_equal(st[b], exp)
        for q, ps in enumerate(side["passes"]):
            assert (prs[q][b].L, prs[q][b].end, prs[q][b].status) == (ps["L"], ps["end"], ps["status"])
        np.testing.assert_array_equal(framing.unpack_bits(host[b], side["L"]), bits_list[b][: side["L"]])
        assert not host[b][(side["L"] + 63) // 64:].any()
    np.testing.assert_array_equal(cover.cpu().numpy(), covers)
    assert prs[3][1].status == 1


@pytest.mark.gpu
def test_gpu_extract_and_decode_refuse_foreign_shapes_and_records():
    """extract() of a scheme-2 codec refuses scheme-1-shaped meta / lm and a short payload buffer;
    decode() refuses an embedding whose record was altered (end beyond its lattice)."""
    torch = pytest.importorskip("torch")
    from codec_tcc_amd import _lib
    from codec_tcc_amd.pee import PeeCodec
    h = w = 16
    covers = np.stack([_image("ct12", h, w, 70 + i) for i in range(2)])
    codec = PeeCodec(2, h, w, dtype="uint16", T=2, maxval=4095, scheme=2)
    enc = codec.embed(torch.from_numpy(covers).cuda(), [_bits(60, 71), _bits(20, 72)])
    for kw in (dict(meta=enc.meta[0]), dict(lm=enc.lm[0]), dict(payload=torch.zeros((2, enc.payload_words - 1), dtype=torch.int64,
                                                                                 device="cuda"))):
        args = dict(meta=enc.meta, lm=enc.lm, payload=None)
        args.update(kw)
        with pytest.raises(ValueError):
            codec.extract(enc.stego, args["meta"], args["lm"], payload_words=enc.payload_words, payload=args["payload"])
    got, cover = codec.decode(enc)
    np.testing.assert_array_equal(cover.cpu().numpy(), covers)
    assert [g.size for g in got] == [60, 20]
    raw = bytearray(enc.meta.cpu().numpy().tobytes())
    rec = _lib.PeeMeta.from_buffer_copy(bytes(raw), _lib.PEE_META_BYTES * 2)   # pass 1, slice 0
    assert rec.reserved[0] == 1 and rec.L > 0
    rec.end = 49
    raw[_lib.PEE_META_BYTES * 2: _lib.PEE_META_BYTES * 3] = bytes(rec)
    enc.meta = torch.frombuffer(raw, dtype=torch.uint8).view(4, 2, -1).cuda()
    with pytest.raises(ValueError, match="slice 0, pass 1: end = 49"):
        codec.decode(enc)
