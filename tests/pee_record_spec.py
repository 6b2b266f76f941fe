"""An independent statement of the MED-PEE exchange records (include/codec_tcc.h, "exchange
records of the MED-PEE side information"): plain Python over individual bits, written from the
header's rule.  Test infrastructure: it is what codec_pee_pack_records /
codec_pee_unpack_records (codec_tcc_amd/csrc/codec_records.hip) and their host restatement
(codec_tcc_amd/distributed.py) are compared with, and it generates the known-answer vectors
tests/golden/pee_records_kat.json.  It takes the struct size and the field offsets from
codec_tcc_amd._lib and nothing else from the package; no torch, no code of distributed.py.

Representation: a meta is the list of codec_pee_meta's 16 int32 fields, a map row a list of
lm_words uint64 words (bit k of the map = bit k % 64 of word k // 64), a record a list of
HDR_WORDS + width uint64 words.

What the header leaves implicit, written out:
  * sparse form iff 0 <= lm_count <= 2 * width.  The slots hold the first lm_count set bits of
    [0, min(end, 64 * lm_words - 1)], ascending, as uint32 (slot 2i in the low half of payload
    word i), the rest zero.  If fewer are found, the header's lm_count becomes the number found
    and flags |= RECOUNTED; every other header field travels untouched;
  * dense form otherwise: words 0 .. width - 1 of the map with every bit k > end cleared (a
    word the map does not have is zero).  An `end` past the map clears nothing; end < -1
    counts as -1;
  * an understated lm_count truncates: the first lm_count indices travel, no more;
  * unpack, sparse: the listed indices below 64 * lm_cols are set; dense: the first
    min(width, lm_cols, ceil((end + 1) / 64)) payload words are copied, the rest is zero.
    Unpack does not mask again.
"""
from __future__ import annotations

import functools

from codec_tcc_amd import _lib

FIELDS = _lib.PEE_META_BYTES // 4                       # int32 fields of codec_pee_meta
HDR_WORDS = (_lib.PEE_META_BYTES + 7) // 8              # CODEC_PEE_RECORD_HDR_WORDS
END = _lib.PeeMeta.end.offset // 4
LM_COUNT = _lib.PeeMeta.lm_count.offset // 4
FLAGS = _lib.PeeMeta.flags.offset // 4
RECOUNTED = 2                                           # CODEC_PEE_RECORD_RECOUNTED
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


@functools.lru_cache(maxsize=None)
def _set_bits(row: tuple) -> tuple:
    """Indices of the row's set bits, ascending (one bit at a time)."""
    out = []
    for k in range(64 * len(row)):
        if (row[k >> 6] >> (k & 63)) & 1:
            out.append(k)
    return tuple(out)


def set_bits(lm_row, end: int):
    """The set bits of [0, min(end, 64 * lm_words - 1)], ascending."""
    return [k for k in _set_bits(tuple(int(w) & M64 for w in lm_row)) if k <= end]


def _words(bits, cols: int):
    out = [0] * cols
    for k in bits:
        if k < 64 * cols:
            out[k >> 6] |= 1 << (k & 63)
    return out


def map_prefix(end: int, lm_row, cols: int):
    """`cols` words of the map with every bit past `end` cleared."""
    return _words(set_bits(lm_row, end), cols)


def width_needed(metas, cap=None) -> int:
    """max over slices of min(ceil(lm_count / 2), ceil((end + 1) / 64)), at least 1, at most cap."""
    w = 1
    for m in metas:
        w = max(w, min(_ceil_div(m[LM_COUNT], 2), _ceil_div(m[END] + 1, 64)))
    return w if cap is None else min(w, int(cap))


def dense_words_needed(metas) -> int:
    """ceil((max end + 1) / 64), at least 1: the dense prefix every map fits in."""
    return max([1] + [_ceil_div(m[END] + 1, 64) for m in metas])


def header_words(meta):
    """The 16 int32 fields as 8 little-endian uint64 words."""
    assert len(meta) == FIELDS
    return [(meta[2 * i] & M32) | ((meta[2 * i + 1] & M32) << 32) for i in range(HDR_WORDS)]


def header_fields(words):
    out = []
    for w in words[:HDR_WORDS]:
        for half in (w & M32, (w >> 32) & M32):
            out.append(half - (1 << 32) if half >> 31 else half)
    return out


def is_sparse(lm_count: int, width: int) -> bool:
    return 0 <= lm_count <= 2 * width


def pack(meta, lm_row, width: int):
    """One slice's record: HDR_WORDS + width uint64 words."""
    meta = list(meta)
    cnt, end = meta[LM_COUNT], meta[END]
    if is_sparse(cnt, width):
        found = set_bits(lm_row, end)[:cnt]
        if len(found) < cnt:
            meta[LM_COUNT] = len(found)
            meta[FLAGS] |= RECOUNTED
        slots = found + [0] * (2 * width - len(found))
        payload = [slots[2 * i] | (slots[2 * i + 1] << 32) for i in range(width)]
    else:
        payload = map_prefix(end, lm_row, width)
    return header_words(meta) + payload


def unpack(record, width: int, lm_cols: int):
    """(meta, lm_cols map words) of one record."""
    assert len(record) == HDR_WORDS + width
    meta = header_fields(record)
    cnt, end = meta[LM_COUNT], meta[END]
    pay = record[HDR_WORDS:]
    if is_sparse(cnt, width):
        slots = [(pay[s >> 1] >> (32 * (s & 1))) & M32 for s in range(cnt)]
        return meta, _words(slots, lm_cols)
    dw = min(width, lm_cols, max(0, _ceil_div(end + 1, 64)))
    return meta, [pay[w] if w < dw else 0 for w in range(lm_cols)]
