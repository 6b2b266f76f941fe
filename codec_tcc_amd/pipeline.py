"""File-level pipeline around the GPU path: the reference's main() encode (codec.py:847-913)
and decode_bin() (codec.py:795-842), with the STGC container and the DICOM reader/writer;
plus the same file round trip for the MED-PEE scheme (encode_file_pee / decode_bin_pee).

The pixel work (decomposition, block search, embedding, bitmaps, extraction, MED-PEE) runs
on the MI355X through the C ABI; this module only moves bytes (zlib, struct, files).

Stego codecs (compress_image / decompress_image, codec.py:108-209):
  raw  this build's uncompressed little-endian pixels (container id 0)
  png  the reference's Deflated Explicit VR Little Endian DICOM (codec.py:151-162, 203-206),
       written and read by dicom.py (zlib raw deflate)
  jxl  cjxl -d 0 -e 3 / djxl (codec.py:111-129, 169-182): runs where the binaries exist
  j2k, jls  gdcmconv (codec.py:132-149, 184-201): the binary and a JPEG 2000 / JPEG-LS
       pixel decoder are absent from this image; both raise RuntimeError naming what is missing
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import api, container, dicom, framing
from .codec import Codec, _require_gpu, _torch, meta_records


def _compress(stego: np.ndarray, codec: str) -> bytes:
    if codec == "raw":
        return container.encode_stego_raw(stego)
    if codec == "png":   # codec.py:151-162: create_dicom + DeflatedExplicitVRLittleEndian
        return dicom.create_dicom_bytes(stego, transfer_syntax=dicom.DEFLATED_LE)
    if codec in ("j2k", "jls"):   # codec.py:132-149
        raise RuntimeError(f"codec '{codec}' needs the gdcmconv binary and a JPEG 2000 / JPEG-LS decoder "
                           "(both absent on this image)")
    if codec == "jxl":   # codec.py:111-129 (cjxl -d 0 -e 3: lossless), only where the binary exists
        exe = shutil.which("cjxl") or shutil.which("cjxl.exe")
        if not exe:
            raise RuntimeError("codec 'jxl' needs the cjxl binary on PATH (absent on this image)")
        from PIL import Image
        with tempfile.TemporaryDirectory() as d:
            png, jxl = os.path.join(d, "in.png"), os.path.join(d, "out.jxl")
            Image.fromarray(stego.astype(np.uint16)).save(png)
            subprocess.run([exe, png, jxl, "-d", "0", "-e", "3"], check=True, capture_output=True)
            return open(jxl, "rb").read()
    raise ValueError(f"Codec '{codec}' não suportado.")   # codec.py:165


def _decompress(data: bytes, codec: str, height: int, width: int) -> np.ndarray:
    if codec in ("raw", "unknown"):
        return container.decode_stego_raw(data, height, width)
    if codec == "png":   # codec.py:203-206: dcmread(force=True).pixel_array
        img = dicom.read_dicom(data)[0]
        if img.shape != (height, width):
            raise ValueError("png (deflated DICOM) stego does not match the header's width x height")
        return img
    if codec in ("j2k", "jls"):   # codec.py:184-201
        raise RuntimeError(f"codec '{codec}' needs the gdcmconv binary and a JPEG 2000 / JPEG-LS decoder "
                           "(both absent on this image)")
    if codec == "jxl":   # codec.py:169-182
        exe = shutil.which("djxl") or shutil.which("djxl.exe")
        if not exe:
            raise RuntimeError("codec 'jxl' needs the djxl binary on PATH (absent on this image)")
        from PIL import Image
        with tempfile.TemporaryDirectory() as d:
            jxl, png = os.path.join(d, "in.jxl"), os.path.join(d, "out.png")
            open(jxl, "wb").write(data)
            subprocess.run([exe, jxl, png], check=True, capture_output=True)
            with Image.open(png) as im:
                return np.array(im)
    raise ValueError(f"Codec '{codec}' não suportado.")   # codec.py:209


def encode_file(image, message: str, out_path: str, *, beta: float = 0.4, block: int = 16,
                codec: str = "raw", version: Optional[int] = None) -> Dict:
    """main() (codec.py:856-909): load -> decompose (beta) -> hybrid embed (block) -> merge
    -> stego codec -> zlib(bitmaps) -> header -> .bin.  `image` is an array or a DICOM path.
    version None: 1 (reference layout, start_offset written as 0 like codec.py:903) when the
    fields fit 16 bits, else 2 (32-bit fields, real offset)."""
    _require_gpu()
    torch = _torch()
    img = image if isinstance(image, np.ndarray) else dicom.read_dicom(image)[0]
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    c = Codec(1, h, w, dtype=str(img.dtype), beta=beta, block=block)
    enc = c.encode(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [message])
    m = meta_records(enc.meta)[0]
    s = m.s
    dense = c.expand_maps(enc.maps, enc.meta, map_words=enc.payloads.map_words, smax=s).cpu().numpy()[0]
    stego = enc.stego.cpu().numpy()[0]
    blob = container.bitmaps_blob(dense)
    sizes = [m.sizes[p] for p in range(s)]
    perm = [m.perm[j] for j in range(s)]
    fits16 = w <= 0xFFFF and h <= 0xFFFF and all(0 <= x <= 0xFFFF for x in sizes)
    ver = version if version is not None else (1 if fits16 else 2)
    hdr = container.create_header(codec, s, sizes, perm, len(blob), w, h, 0 if ver == 1 else m.start_offset,
                                  False, version=ver, search_block_size=block if ver == 2 else None)
    size = container.create_binary_file(out_path, hdr, _compress(stego, codec), blob)
    return {"path": out_path, "bytes": size, "version": ver, "s": s, "segments_lengths": sizes,
            "segment_indices": perm, "start_offset": m.start_offset, "stego": stego}


def decode_bin(filepath: str, output_prefix: Optional[str] = None) -> Tuple[str, np.ndarray]:
    """decode_bin (codec.py:795-842): the reference's message (its lossy decode_message,
    bit-exact) and the stego image.  Files are written only when output_prefix is given."""
    md, blob, payload = container.parse_bin_file(filepath)
    s = md["s"]
    stego = _decompress(payload, md["codec"], md["height"], md["width"])
    bitmaps = container.split_bitmaps(blob, s)
    message = api.decode_message(api.extract_local_planes(stego, s), bitmaps, md)
    if output_prefix is not None:
        with open(f"{output_prefix}_mensagem.txt", "w", encoding="utf-8") as f:
            f.write(message)
        dicom.save_dicom(stego, f"{output_prefix}_imagem.dcm")
    return message, stego


def decode_bin_exact(filepath: str, search_block_size: Optional[int] = None) -> Tuple[str, np.ndarray]:
    """Exact payload bits and the restored cover from a .bin.

    Version 2 files carry the real start offset (and the search block size), which are used
    as stored.  Version 1 files (the reference's layout) store start_offset = 0
    (codec.py:903): the offset is re-derived by the block search on the restored plane 0,
    which needs the block size the file was encoded with -- search_block_size (default 16,
    main()'s value, codec.py:875); a different size decodes the wrong window."""
    md, blob, payload = container.parse_bin_file(filepath)
    s = md["s"]
    stego = _decompress(payload, md["codec"], md["height"], md["width"])
    bitmaps = container.split_bitmaps(blob, s)
    block = search_block_size or md.get("search_block_size") or 16
    offset = md["start_offset"] if md["version"] == 2 else None
    return api.decode_positional(stego, bitmaps, md, search_block_size=block,
                                 align_across_planes=bool(md["align_flag"]), start_offset=offset)


# ------------------------------------------------------------------ MED-PEE files
def encode_file_pee(image, payload, out_path: str, *, T=2, tmax: int = 16, maxval: Optional[int] = None,
                    codec: str = "raw", scheme: int = 1, tmin: int = 1, checksum=False, gate=None, tile=64,
                    roi=None, key=None, nonce=None) -> Dict:
    """MED-PEE embed of one slice into a version-16 STGC file.  `image` is an array or a
    DICOM path; maxval defaults to the DICOM's full scale 2**BitsStored - 1 (4095 for the
    reference's 12-bit pe.dcm), else the dtype maximum.  T = 'auto' picks the smallest
    T <= tmax whose capacity holds the payload.  A payload beyond the capacity is truncated
    (status 1, 'L' = bits embedded); the file stays exactly reversible.  scheme 2: four
    sublattice passes (container scheme byte 2); with T = 'auto' the smallest T in tmin..tmax whose
    four passes hold the payload, which the header and the returned 'T' then carry.
    checksum=True: the header ends with the checksum extension (container.pee_crc_extension:
    CRC-32 of the cover, from the GPU pass queued before the embed, and of the embedded
    payload bits), which decode_bin_pee verifies; without it the file's bytes are unchanged.
    checksum="tiles": the tile extension follows it (container.pee_tile_extension: the cover's
    CRC-32 per `tile`, an int or (th, tw) in 4..1024), so that decode_bin_pee names the tiles of a
    cover that fails its check; readers that know only the checksum extension read the file as ever.
    gate (scheme 1): a smoothness gate 0..65535 or 'auto' (PeeCodec): the file then carries scheme
    byte 3 and the chosen gate after scheme 1's fixed header fields ('gate' in the result);
    without it the file's bytes are unchanged.
    roi (scheme 1): a rectangle (y0, x0, y1, x1) the stego leaves bit-identical to the cover
    (PeeCodec.embed): the file then carries scheme byte 4 -- byte 3's fields (the gate
    65535 when none was asked for) and the rectangle ('roi' in the result).  An empty rectangle is
    no rectangle: the file is what it is without roi=.  Without roi the file's bytes are unchanged.
    key (32 bytes) / nonce (8 bytes, fresh when None): a keyed file (PeeCodec.embed(key=), DESIGN
    §3j): the stego carries the ChaCha20 ciphertext and the header ends with the keyed extension
    (container.pee_aead_extension: nonce and Poly1305 tag; 'nonce' / 'tag' in the result), after
    the checksum extensions when those are asked for -- their payload field is then 0 and not
    verified (the tag covers the payload; a CRC of the plaintext would tell about it).  A payload
    truncated by capacity does not authenticate.  Without key the file's bytes are unchanged."""
    from . import aead as _aead
    from . import checksum as _ck
    key, nonce, _index0 = _aead.check_call(key, nonce, lone="nonce= goes with key=")   # before the GPU is touched
    from .pee import PeeCodec, check_gate_args, check_roi_args, lm_bits
    checksum, tiled = _ck.checksum_mode(checksum)
    tile = _ck.check_tile_args(tile) if tiled else None
    if gate is not None:
        shape = getattr(image, "shape", (0, 0))
        check_gate_args(gate, T, tmax, (int(shape[-2]) // 2) * (int(shape[-1]) // 2) if len(shape) >= 2 else 0, scheme)
    _require_gpu()
    torch = _torch()
    if isinstance(image, np.ndarray):
        img = image
    else:
        img, attrs = dicom.read_dicom(image)
        if maxval is None and attrs.get("bits_stored"):
            maxval = (1 << int(attrs["bits_stored"])) - 1
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    if roi is not None:   # judged before the codec is built or anything queued; an empty rectangle: none
        rect = check_roi_args(roi, 1, h, w, scheme=scheme, T=T, tmax=tmax, gate=gate)
        roi = tuple(int(v) for v in rect[0]) if rect[0].any() else None
    bits = framing.to_bits(payload)
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=T, tmin=tmin, tmax=tmax, maxval=maxval, scheme=scheme, gate=gate)
    enc = pc.embed(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [bits],
                   checksum="tiles" if tiled else checksum, **({"tile": tile} if tiled else {}),
                   **({"roi": roi} if roi is not None else {}),
                   **({"key": key, "nonce": nonce} if key is not None else {}))

    def ext(embedded: int) -> Tuple[bytes, Dict]:
        xb, crcs = b"", {}
        if checksum:
            crcs = {"cover_crc32": _ck.crc_list(enc.cover_crc)[0],
                    "payload_crc32": _ck.payload_crc32(bits[:embedded]) if key is None else 0}
            xb = container.pee_crc_extension(crcs["cover_crc32"], crcs["payload_crc32"])
            if tiled:
                crcs["tile"] = tile
                crcs["tile_crc32"] = enc.cover_tile_crc[0].cpu().numpy().view(np.uint32)
                xb += container.pee_tile_extension(tile[0], tile[1], crcs["tile_crc32"])
        if key is not None:
            crcs.update(nonce=nonce, tag=_aead.tag_bytes(enc.tag)[0])
            xb += container.pee_aead_extension(nonce, crcs["tag"])
        return xb, crcs
    if scheme == 2:
        prs = [pr[0] for pr in enc.pass_records()]
        blobs = [container.lm_blob(lm_bits(enc, 0, p)) if prs[p].end >= 0 else b"" for p in range(4)]
        embedded = enc.embedded()[0]
        status = 1 if embedded < len(bits) else 0
        stego = enc.stego.cpu().numpy()[0]
        t_used = int(prs[0].T)   # T = 'auto': the slice's chosen T (every pass records it)
        hdr = container.create_pee2_header(codec, img.dtype.itemsize, w, h, t_used, pc.maxval, embedded, status,
                                           [(r.L, r.end, r.status, len(b)) for r, b in zip(prs, blobs)])
        xb, crcs = ext(embedded)
        size = container.create_binary_file(out_path, hdr + xb, _compress(stego, codec), b"".join(blobs))
        return {"path": out_path, "bytes": size, "T": t_used, "L": embedded, "maxval": pc.maxval, "status": status,
                "scheme": 2, "passes": [{"L": r.L, "end": r.end, "status": r.status, "lm_count": r.lm_count}
                                        for r in prs], "stego": stego, **crcs}
    r = enc.records()[0]
    embedded = min(len(bits), r.capacity) if r.status == 1 else len(bits)
    lmb = container.lm_blob(lm_bits(enc, 0)) if r.end >= 0 else b""
    stego = enc.stego.cpu().numpy()[0]
    gated = {}
    if roi is not None:   # the gate and the rectangle the record carries
        from .roi import record_roi
        gated = {"gate": int(r.reserved[1]) - 1, "roi": record_roi(r), "scheme": container.PEE_SCHEME_ROI}
        hdr = container.create_pee_roi_header(codec, img.dtype.itemsize, w, h, r.T, embedded, r.end, r.maxval,
                                              r.status, len(lmb), gated["gate"], gated["roi"])
    elif gate is None:
        hdr = container.create_pee_header(codec, img.dtype.itemsize, w, h, r.T, embedded, r.end, r.maxval, r.status,
                                          len(lmb))
    else:   # the gate the record carries (gate='auto': the slice's chosen one)
        gated = {"gate": int(r.reserved[1]) - 1, "scheme": container.PEE_SCHEME_GATE}
        hdr = container.create_pee_gate_header(codec, img.dtype.itemsize, w, h, r.T, embedded, r.end, r.maxval,
                                               r.status, len(lmb), gated["gate"])
    xb, crcs = ext(embedded)
    size = container.create_binary_file(out_path, hdr + xb, _compress(stego, codec), lmb)
    return {"path": out_path, "bytes": size, "T": r.T, "L": embedded, "end": r.end, "maxval": r.maxval,
            "status": r.status, "lm_count": r.lm_count, "stego": stego, **gated, **crcs}


def encode_dicom_pee(image_or_path, payload, out_path: str, T: int = 2, checksum: bool = True,
                     maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    """Blind MED-PEE (PeeCodec.embed_blind) of `payload` (str / bytes / 0-1 vector, as
    encode_file_pee takes it) into a plain DICOM: the file's pixel data is the stego
    (dicom.save_dicom), which carries its own header and location map, so decode_dicom_pee needs
    the file alone and any DICOM store keeps it like every other image.  maxval: the DICOM's
    BitsStored when the image is one, else the dtype's maximum.  checksum=True: the header holds
    the cover's CRC-32.  ValueError when the payload and its side bits do not fit."""
    from .pee import PeeCodec
    _require_gpu()
    torch = _torch()
    if isinstance(image_or_path, np.ndarray):
        img = image_or_path
    else:
        img, attrs = dicom.read_dicom(image_or_path)
        if maxval is None and attrs.get("bits_stored"):
            maxval = (1 << int(attrs["bits_stored"])) - 1
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    bits = framing.to_bits(payload)
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=T, maxval=maxval)
    stego, info = pc.embed_blind(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [bits], checksum=bool(checksum),
                                 max_entries=max_entries)
    out = stego.cpu().numpy()[0]
    size = dicom.save_dicom(out, out_path)
    row = [int(v) for v in info.cpu().tolist()[0]]
    return {"path": out_path, "bytes": size, "T": int(T), "maxval": pc.maxval, "stego": out,
            **dict(zip(("status", "L", "E", "n_side", "end", "region_row"), row))}


def encode_dicom_pee_auto(image_or_path, payload, out_path: str, tmax: int = 16, checksum: bool = True,
                          maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    """encode_dicom_pee with T chosen on the device (PeeCodec.embed_blind_auto): the
    smallest T in 1..tmax that takes the payload and its side bits.  The result's "T" is the chosen
    one; decode_dicom_pee reads the file as it is.  ValueError when no T <= tmax serves."""
    from .pee import PeeCodec
    _require_gpu()
    torch = _torch()
    if isinstance(image_or_path, np.ndarray):
        img = image_or_path
    else:
        img, attrs = dicom.read_dicom(image_or_path)
        if maxval is None and attrs.get("bits_stored"):
            maxval = (1 << int(attrs["bits_stored"])) - 1
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    bits = framing.to_bits(payload)
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=1, tmax=tmax, maxval=maxval)
    stego, info, ts = pc.embed_blind_auto(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [bits],
                                          checksum=bool(checksum), max_entries=max_entries)
    out = stego.cpu().numpy()[0]
    size = dicom.save_dicom(out, out_path)
    row = [int(v) for v in info.cpu().tolist()[0]]
    return {"path": out_path, "bytes": size, "T": int(ts.cpu().tolist()[0]), "maxval": pc.maxval, "stego": out,
            **dict(zip(("status", "L", "E", "n_side", "end", "region_row"), row))}


def encode_dicom_pee_gated(image_or_path, payload, out_path: str, tmax: int = 4, gate="auto", T=None, checksum: bool = True,
                           maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    """encode_dicom_pee with (T, gate) chosen on the device (PeeCodec.embed_blind_gated):
    only candidates in flat surroundings are modified.  The result's "T" and "G" are the chosen pair;
    decode_dicom_pee reads the file as it is.  ValueError when no pair serves."""
    from .pee import PeeCodec
    _require_gpu()
    torch = _torch()
    if isinstance(image_or_path, np.ndarray):
        img = image_or_path
    else:
        img, attrs = dicom.read_dicom(image_or_path)
        if maxval is None and attrs.get("bits_stored"):
            maxval = (1 << int(attrs["bits_stored"])) - 1
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    bits = framing.to_bits(payload)
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=1, maxval=maxval)
    stego, info, ts, gs = pc.embed_blind_gated(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [bits], gate=gate, T=T,
                                               tmax=tmax, checksum=bool(checksum), max_entries=max_entries)
    out = stego.cpu().numpy()[0]
    size = dicom.save_dicom(out, out_path)
    row = [int(v) for v in info.cpu().tolist()[0]]
    return {"path": out_path, "bytes": size, "T": int(ts.cpu().tolist()[0]), "G": int(gs.cpu().tolist()[0]),
            "maxval": pc.maxval, "stego": out, **dict(zip(("status", "L", "E", "n_side", "end", "region_row"), row))}


def decode_dicom_pee(path, verify=True) -> Tuple[np.ndarray, np.ndarray]:
    """(payload bits as a 0/1 uint8 vector, restored cover) from a DICOM written by
    encode_dicom_pee (a path or the file's bytes): PeeCodec.decode_blind on its pixels.  ValueError
    for an image that carries no blind MED-PEE header, IntegrityError when the restored cover
    fails the CRC-32 its header carries (verify as decode_blind's)."""
    from .pee import PeeCodec
    img, _attrs = dicom.read_dicom(path)
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    _require_gpu()
    h, w = img.shape
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=1)
    bits, cover = pc.decode_blind(_torch().from_numpy(np.ascontiguousarray(img)[None]).cuda(), verify=verify)
    return bits[0], cover.cpu().numpy()[0]


def _series_pixels(items, maxval=None):
    """([H,W] arrays stacked, maxval): a series given as arrays or DICOM paths / bytes, all of one
    shape and dtype."""
    imgs = []
    for it in items:
        if isinstance(it, np.ndarray):
            img = it
        else:
            img, attrs = dicom.read_dicom(it)
            if maxval is None and attrs.get("bits_stored"):
                maxval = (1 << int(attrs["bits_stored"])) - 1
        if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
            raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
        imgs.append(np.ascontiguousarray(img))
    if not imgs or len({(a.shape, a.dtype) for a in imgs}) != 1:
        raise ValueError("a series is one or more slices of one shape and dtype")
    return np.stack(imgs), maxval


def encode_dicom_series_pee(images_or_paths, payload, out_dir: str, tmax: int = 16, policy: str = "even",
                            checksum: bool = True, maxval: Optional[int] = None, max_entries: int = 256,
                            volume_id=None) -> Dict:
    """One payload across a DICOM series as blind volume stegos (PeeCodec.embed_blind_volume; DESIGN
    §3n): one plain DICOM per slice in out_dir (slice_00000.dcm, ...), each carrying its place in the
    stream, so decode_dicom_series_pee reads the files back in any order.  ValueError when the payload
    exceeds the series' capacity at tmax (nothing is written)."""
    import os
    from .pee import PeeCodec
    _require_gpu()
    torch = _torch()
    stack, maxval = _series_pixels(images_or_paths, maxval)
    B, h, w = stack.shape
    pc = PeeCodec(B, h, w, dtype=str(stack.dtype), T=1, tmax=tmax, maxval=maxval)
    stego, info, ts = pc.embed_blind_volume(torch.from_numpy(stack).cuda(), payload, volume_id=volume_id, policy=policy,
                                            checksum=bool(checksum), max_entries=max_entries)
    out = stego.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, f"slice_{b:05d}.dcm") for b in range(B)]
    sizes = [dicom.save_dicom(out[b], p) for b, p in enumerate(paths)]
    v = [int(x) for x in info["volume"].cpu().tolist()]
    return {"paths": paths, "bytes": sizes, "volume_id": info["volume_id"], "T": v[1], "N": v[5], "carriers": v[4],
            "capacity": v[3], "n": info["n"].cpu().tolist(), "off": info["off"].cpu().tolist(), "ts": ts.cpu().tolist(),
            "maxval": pc.maxval, "stego": out}


def decode_dicom_series_pee(paths, verify=True, partial: bool = False):
    """(payload bits, restored covers [B,H,W] in the order given) from the DICOMs of
    encode_dicom_series_pee, in any order and with unmarked slices among them
    (PeeCodec.decode_blind_volume); partial=True also returns the missing bit ranges instead of
    raising when slices are absent."""
    from .pee import PeeCodec
    stack, _mv = _series_pixels(paths)
    _require_gpu()
    B, h, w = stack.shape
    pc = PeeCodec(B, h, w, dtype=str(stack.dtype), T=1)
    out = pc.decode_blind_volume(_torch().from_numpy(stack).cuda(), verify=verify, partial=partial)
    return (out[0], out[1].cpu().numpy()) + tuple(out[2:])


def encode_dicom_pee_keyed(image_or_path, payload, out_path: str, key, T: int = 2, tmax=None, nonce=None,
                           maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    """encode_dicom_pee under a 32-byte key (PeeCodec.embed_blind_keyed): the file's pixels
    carry the nonce, the Poly1305 tag of (cover, ciphertext) and the encrypted payload, so
    decode_dicom_pee_keyed needs the file and the key alone.  tmax in 1..16: T chosen on the device
    instead of the fixed T.  The result names the T used, the nonce and the payload bits ("L";
    "n_user" is the header's count, frame included)."""
    from . import aead as _aead
    from .pee import PeeCodec
    if key is None:
        raise ValueError("encode_dicom_pee_keyed takes a 32-byte key; encode_dicom_pee is the unkeyed call")
    key, nonce, _i = _aead.check_call(key, nonce)   # before the GPU is touched; a fresh nonce when None
    _require_gpu()
    torch = _torch()
    if isinstance(image_or_path, np.ndarray):
        img = image_or_path
    else:
        img, attrs = dicom.read_dicom(image_or_path)
        if maxval is None and attrs.get("bits_stored"):
            maxval = (1 << int(attrs["bits_stored"])) - 1
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    h, w = img.shape
    bits = framing.to_bits(payload)
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=T if tmax is None else 1, tmax=16 if tmax is None else tmax, maxval=maxval)
    stego, info, ts = pc.embed_blind_keyed(torch.from_numpy(np.ascontiguousarray(img)[None]).cuda(), [bits], key=key,
                                           nonce=nonce, tmax=tmax, max_entries=max_entries)
    out = stego.cpu().numpy()[0]
    size = dicom.save_dicom(out, out_path)
    row = [int(v) for v in info.cpu().tolist()[0]]
    return {"path": out_path, "bytes": size, "T": int(ts.cpu().tolist()[0]), "maxval": pc.maxval, "stego": out,
            "nonce": nonce, "L": int(bits.size),
            **dict(zip(("status", "n_user", "E", "n_side", "end", "region_row"), row))}


def decode_dicom_pee_keyed(path, key, verify=True) -> Tuple[np.ndarray, np.ndarray]:
    """(payload bits as a 0/1 uint8 vector, restored cover) from a DICOM written by
    encode_dicom_pee_keyed (a path or the file's bytes) and its key: PeeCodec.decode_blind_keyed on
    its pixels.  ValueError for an image without a keyed header (an unkeyed one is
    decode_dicom_pee's), IntegrityError when the tag fails."""
    from . import aead as _aead
    from .pee import PeeCodec
    _aead.check_key(key)
    img, _attrs = dicom.read_dicom(path)
    if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
        raise ValueError("A imagem deve ser 2D uint8 ou uint16.")
    _require_gpu()
    h, w = img.shape
    pc = PeeCodec(1, h, w, dtype=str(img.dtype), T=1)
    bits, cover = pc.decode_blind_keyed(_torch().from_numpy(np.ascontiguousarray(img)[None]).cuda(), key, verify=verify)
    return bits[0], cover.cpu().numpy()[0]


@dataclass
class PeeFile:
    """The host half of a MED-PEE file decode (read_pee_bytes): everything the launch needs."""
    md: Dict                 # the header's side information
    scheme: int              # 1 or 2
    records: List            # checked codec_pee_meta records: [pass][slice] (one slice)
    lm: np.ndarray           # bool [passes, 1, 64 * lm_words]: the location-map bits
    stego: np.ndarray        # [H, W] uint8 / uint16
    payload_words: int
    lm_words: int


def read_pee_bytes(raw: bytes) -> PeeFile:
    """File bytes -> checked records, location-map bits, the stego array and the payload word
    count, on the host alone (no GPU): decode_bin_pee launches on what this returns.  A file
    that is truncated, malformed or whose header fields contradict each other raises
    ValueError here (container.parse_pee*_bytes for the structure, pee.check_records for the
    records), before anything reaches a kernel."""
    from .pee import check_records, make_record
    scheme = container.pee_scheme(raw)
    gate = roi = None
    if scheme == 2:
        md, blobs, data = container.parse_pee2_bytes(raw)
        passes = md["passes"]
    elif scheme == container.PEE_SCHEME_ROI:    # scheme 1 with a protected rectangle: one ROI record
        md, blob, data = container.parse_pee_roi_bytes(raw)   # (refuses a rectangle outside the image)
        blobs, passes = [blob], [{"L": md["L"], "end": md["end"], "status": md["status"]}]
        scheme, gate, roi = 1, md["gate"], md["roi"]
    elif scheme == container.PEE_SCHEME_GATE:   # scheme 1 with a smoothness gate: one gated record
        md, blob, data = container.parse_pee_gate_bytes(raw)
        blobs, passes = [blob], [{"L": md["L"], "end": md["end"], "status": md["status"]}]
        scheme, gate = 1, md["gate"]
    else:
        md, blob, data = container.parse_pee_bytes(raw)
        blobs, passes = [blob], [{"L": md["L"], "end": md["end"], "status": md["status"]}]
    h, w = md["height"], md["width"]
    if h * w > 0x7FFFFFFF:
        raise ValueError(f"MED-PEE header: {w} x {h} pixels exceed the codec's 2^31 - 1")
    stego = _decompress(data, md["codec"], h, w)
    if stego.shape != (h, w) or stego.dtype.itemsize != md["bytes"]:
        raise ValueError("stego pixels do not match the MED-PEE header's shape / pixel size")
    lm_words = max(1, ((h // 2) * (w // 2) + 63) // 64)
    pw = max(1, (md["L"] + 63) // 64)
    records = [[make_record(h, w, T=md["T"], maxval=md["maxval"], L=ps["L"], end=ps["end"], status=ps["status"],
                            lattice=p, gate=gate, roi=roi)] for p, ps in enumerate(passes)]
    check_records(records, h, w, scheme=scheme, payload_words=pw, lm_words=lm_words, bytes=md["bytes"],
                  lengths=[md["L"]] if scheme == 2 else None)
    if md["status"] not in (0, 1) or any(ps["status"] not in (0, 1) for ps in passes):
        raise ValueError("MED-PEE header: a status other than 0 / 1 (files hold finished embeddings)")
    lm = np.zeros((len(passes), 1, lm_words * 64), dtype=bool)
    for p, ps in enumerate(passes):   # end < 64 * lm_words: checked above
        if ps["end"] >= 0:
            lm[p, 0, : ps["end"] + 1] = container.lm_from_blob(blobs[p], ps["end"])
    return PeeFile(md=md, scheme=scheme, records=records, lm=lm, stego=stego, payload_words=pw, lm_words=lm_words)


def decode_bin_pee(filepath: str, verify=True, key=None) -> Tuple[np.ndarray, np.ndarray]:
    """(payload bits as a 0/1 uint8 vector, restored cover) from a version-16 STGC file
    (either scheme): read_pee_bytes on the host, then one extract launch.
    verify=True: a file with the checksum extension is checked -- the restored cover's CRC-32
    (one GPU pass behind the extract) and the payload's against the header's; IntegrityError
    names what failed, and for a file with the tile extension its `tiles` attribute maps the tiles
    of the cover that differ.  False skips it; 'require' also raises for a file without checksums.
    key: required for a file with the keyed extension (encode_file_pee(key=)); a keyed file without
    key=, or key= for a file without the extension, is a ValueError before the GPU is touched.  The
    restored cover and the extracted rows are tagged and compared on the device; IntegrityError
    (.keyed, .slices == [0]) when the tag fails, and no plaintext reaches the host.  verify=False
    decrypts without the tag pass.  What follows the extract is pee_verify.after_extract, as for
    PeeCodec.decode: a scheme-1 extract whose look-back gave up raises decode()'s RuntimeError."""
    from . import checksum as _ck, pee_verify as _pv
    from .pee import PeeCodec, PeeEncoded
    mode = _ck.verify_mode(verify)
    with open(filepath, "rb") as f:
        pf = read_pee_bytes(f.read())
    md, (h, w) = pf.md, pf.stego.shape
    keyed = "aead_tag" in md
    key = _pv.check_key(keyed, key, "file", "its header carries the A1 extension", "A1 extension")
    _require_gpu()
    torch = _torch()
    have = "cover_crc32" in md
    _pv.check_require(mode, keyed, have, have, "MED-PEE file", "the header", named=False)
    pc = PeeCodec(1, h, w, dtype=str(pf.stego.dtype), T=md["T"], maxval=md["maxval"], scheme=pf.scheme)
    metas = b"".join(bytes(r) for pr in pf.records for r in pr)
    meta_t = torch.frombuffer(bytearray(metas), dtype=torch.uint8).view(len(pf.records), 1, -1).cuda()
    lm_t = torch.from_numpy(np.packbits(pf.lm, axis=-1, bitorder="little").view(np.int64).copy()).cuda()
    if pf.scheme == 1:
        meta_t, lm_t = meta_t[0], lm_t[0]
    # what the header states, as an embedding: the records were judged on the host (read_pee_bytes) and
    # are not read back; the tile table stays on the host until a cover fails; a keyed file's payload
    # CRC field is not verified (the tag covers the payload)
    enc = PeeEncoded(stego=torch.from_numpy(np.ascontiguousarray(pf.stego)[None]).cuda(), lm=lm_t, meta=meta_t,
                     lengths=[md["L"]], payload_words=pf.payload_words, scheme=pf.scheme,
                     cover_crc=[md["cover_crc32"]] if have else None,
                     payload_crc=[md["payload_crc32"]] if have and not keyed else None,
                     cover_tile_crc=md["tile_crc32"].view(np.int32)[None].copy() if "tile_crc32" in md else None,
                     tile=md.get("tile"), nonce=md.get("aead_nonce"))
    if keyed and mode is not None:
        enc.tag = torch.from_numpy(np.frombuffer(md["aead_tag"], dtype="<i4").reshape(1, 4).copy()).cuda()
    words, cover = pc.extract(enc.stego, meta_t, lm_t, payload_words=pf.payload_words,
                              **({"gated": True} if "gate" in md else {}), **({"roi": True} if "roi" in md else {}))
    # scheme 1's B = 1 out-of-place extract takes the flat look-back route: its flag is read (as decode() does)
    rows, _total = _pv.after_extract(pc, enc, cover, words, mode, key, what="MED-PEE file", lookback=pf.scheme == 1)
    return framing.unpack_bits(rows[0], md["L"]), cover.cpu().numpy()[0]
