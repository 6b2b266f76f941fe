#!/usr/bin/env python3
"""Known answers of the tile checksums -> tests/golden/tile_crc_kat.json.

Written from zlib alone (tests/tile_crc_spec.py): seeded images of odd and even shapes, both
pixel types, tiles 4, 8, (16, 8) and 64.  The images are regenerated from their seeds
(numpy's default_rng(seed).integers(0, top, shape)); the tables are written out in full.

    python tests/golden/make_tile_crc_kat.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tile_crc_spec as S  # noqa: E402

# (shape, dtype, seed, top): pixel values in [0, top)
IMAGES = [
    ((37, 53), "uint16", 11, 4096),
    ((40, 56), "uint16", 12, 65536),
    ((64, 128), "uint16", 13, 4096),
    ((33, 47), "uint8", 14, 256),
    ((64, 128), "uint8", 15, 256),
    ((5, 130), "uint16", 16, 65536),
]
TILES = [4, 8, (16, 8), 64]


def image(shape, dtype, seed, top):
    return np.random.default_rng(seed).integers(0, top, shape).astype(dtype)


def main():
    cases = []
    for shape, dtype, seed, top in IMAGES:
        img = image(shape, dtype, seed, top)
        for tile in TILES:
            cases.append({"shape": list(shape), "dtype": dtype, "seed": seed, "top": top,
                          "tile": list(tile) if isinstance(tile, tuple) else tile,
                          "grid": list(S.grid(shape[0], shape[1], tile)),
                          "table": S.tile_table(img, tile).tolist()})
    out = os.path.join(HERE, "tile_crc_kat.json")
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
