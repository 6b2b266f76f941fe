#!/usr/bin/env python3
"""Known-answer vectors of the MED-PEE exchange records -> tests/golden/pee_records_kat.json.

Computed by the bit-by-bit statement tests/pee_record_spec.py (not by the kernels or the host
rule they then check).  Small cases (lm_words <= 4) of both forms: the 2 * width boundary from
both sides, an odd count (half a payload word), a word with all 64 bits set, the recount
(with end = -1 too), an understated count, end = -1 / 63 / 64 / -70, an `end` past the map in
both forms, width > lm_words.  Every map carries bits past its `end`; the meta fields other
than end / lm_count hold distinct non-zero values.

    python tests/golden/make_pee_records_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pee_record_spec as S  # noqa: E402

A, F, G = 0xAAAAAAAAAAAAAAAA, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001
# (name, map words, end, lm_count or "true" (+ n), width, the two lm_cols)
CASES = [
    ("sparse", [0x8000000000000011, 0x0000000000000104, F], 100, "true", 3, (1, 3)),
    ("sparse_odd_count", [0x17, 0x8000000000000000, A], 127, "true", 3, (2, 4)),   # 5 indices in 3 words
    ("boundary_2w", [0x8421, 0x30, F], 70, "true", 3, (1, 2)),           # 6 bits = 2 * 3: sparse
    ("boundary_2w_plus_1", [0x8421, 0x70, F], 70, "true", 3, (1, 2)),    # 7 bits = 2 * 3 + 1: dense
    ("full_word_sparse", [1, F, 0x10, F], 132, "true", 33, (2, 5)),      # 1 + 64 + 1 = 66 = 2 * 33
    ("recount", [0x8000000000000011, 0x104, F], 100, "true+4", 5, (1, 3)),
    ("recount_end_minus_1", [A, F], -1, 3, 2, (1, 2)),
    ("end_minus_1_dense", [A, F], -1, 3, 1, (1, 2)),
    ("end_63_dense", [G, F], 63, -1, 2, (1, 2)),
    ("end_63_sparse", [G, F], 63, "true", 2, (1, 2)),
    ("end_64_dense", [A, F], 64, 1000000, 2, (1, 3)),
    ("end_64_sparse", [G, F], 64, "true", 2, (1, 3)),
    ("end_minus_70", [A, F], -70, "true", 2, (1, 2)),
    ("end_minus_70_dense", [A, F], -70, -1, 2, (1, 2)),
    ("end_past_map_dense", [A, 1, 0, F], 300, 1000000, 4, (1, 4)),
    ("end_past_map_sparse", [0x11, 0, 0, 0xF000000000000000], 300, "true", 3, (4, 5)),
    ("understated", [0xFF, 0xFF00, F], 127, 7, 4, (1, 2)),
    ("width_above_lm_words", [A, A], 127, -5, 5, (2, 6)),
]


def meta_of(i, end, cnt):
    m = [(0x01010101 * (f + 1) + 0x100 * i) & 0x7FFFFFFF for f in range(S.FIELDS)]
    m[S.FLAGS] &= ~S.RECOUNTED
    m[S.END], m[S.LM_COUNT] = end, cnt
    return m


def build():
    out = []
    for i, (name, row, end, cnt, width, cols) in enumerate(CASES):
        if isinstance(cnt, str):
            cnt = len(S.set_bits(row, end)) + int(cnt[4:] or 0)
        meta = meta_of(i, end, cnt)
        rec = S.pack(meta, row, width)
        out.append({"name": name, "lm_words": len(row), "meta": meta, "lm": ["%016x" % w for w in row], "width": width,
                    "form": "sparse" if S.is_sparse(cnt, width) else "dense",
                    "record": ["%016x" % w for w in rec],
                    "unpack": [{"lm_cols": c, "lm": ["%016x" % w for w in S.unpack(rec, width, c)[1]]} for c in cols]})
    return out


if __name__ == "__main__":
    cases = build()
    with open(os.path.join(HERE, "pee_records_kat.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")   # one case per line
    print(f"{len(cases)} cases -> pee_records_kat.json")
