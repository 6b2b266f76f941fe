"""CRC-32 checksums of covers and payloads (include/codec_tcc_crc.h): what MED-PEE decode
verifies, so that a stego, record or location map that is not what was embedded raises
IntegrityError instead of decoding to garbage.

CRC-32 as zlib computes it (reflected 0xEDB88320, init and final xor 0xFFFFFFFF):
  cover checksum of a slice   = zlib.crc32 of its pixels, row-major, little-endian bytes;
  payload checksum of a slice = zlib.crc32 of its L bits packed LSB-first into ceil(L / 8)
                                bytes, pad bits zero (framing.pack_bits' packing).

The cover checksum is one read-only streaming HIP pass on the caller's stream
(codec_crc32_slices); there is no CPU fallback.  CRC-32 detects corruption and
inconsistency, not an adversary.
"""
from __future__ import annotations

import ctypes as C
import zlib
from typing import List, Optional

import numpy as np

from . import _lib
from .codec import _require_gpu, _stream, _torch


class IntegrityError(ValueError):
    """A decoded cover or payload does not have the checksum recorded at embed time."""


def chunk_bytes() -> int:
    """Bytes of one slice one workgroup of the kernel covers (codec_crc32_chunk_bytes)."""
    return int(_lib.load().codec_crc32_chunk_bytes())


def crc32_slices(images, out=None):
    """CRC-32 of every slice of a [B,H,W] (or [H,W]) uint8 / uint16 GPU tensor: an int32 device
    tensor of B words holding the checksums' 32 bits (crc_list() gives them as Python ints).
    Asynchronous on the current stream, capturable; `out` (int32 [B], same device) is written
    when given.  ValueError for a non-contiguous tensor or another dtype; any byte alignment
    of the tensor's storage offset is exact."""
    _require_gpu()
    torch = _torch()
    if not isinstance(images, torch.Tensor):
        raise ValueError("crc32_slices takes a torch tensor on the GPU")
    if images.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"crc32_slices takes uint8 or uint16 pixels, got {images.dtype}")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or min(images.shape) < 1:
        raise ValueError("crc32_slices takes a [B,H,W] or [H,W] tensor with no empty dimension")
    if not images.is_cuda:
        raise ValueError("crc32_slices takes a tensor on the GPU")
    if not images.is_contiguous():
        raise ValueError("crc32_slices takes a contiguous tensor (the checksum is of the bytes as they lie)")
    B, H, W = (int(v) for v in images.shape)
    nbytes = images.element_size()
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=images.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B,) or not out.is_contiguous() or out.device != images.device:
        raise ValueError(f"out must be a contiguous int32 [{B}] tensor on the images' device")
    lib = _lib.load()
    ws = int(lib.codec_crc32_workspace_bytes(B, H, W, nbytes))
    if ws == 0:
        raise ValueError(f"crc32_slices: a batch of {B} x {H} x {W} is beyond the kernel's limits")
    work = torch.empty(ws, dtype=torch.uint8, device=images.device)
    _lib.check(lib.codec_crc32_slices(B, H, W, nbytes, images.data_ptr(), out.data_ptr(), work.data_ptr(), ws,
                                      _stream()), "codec_crc32_slices")
    return out


def crc_list(t) -> List[int]:
    """The checksums of a crc32_slices() tensor as unsigned Python ints (one read-back)."""
    return [int(v) & 0xFFFFFFFF for v in t.detach().cpu().tolist()]


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """CRC-32 of A || B from a = CRC-32(A), b = CRC-32(B) and B's length in bytes (pure host,
    the library's GF(2) routine: codec_crc32_combine)."""
    if len_b < 0:
        raise ValueError("len_b must be >= 0")
    out = C.c_uint32(0)
    _lib.check(_lib.load().codec_crc32_combine(int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF, int(len_b), C.byref(out)),
               "codec_crc32_combine")
    return int(out.value)


def payload_crc32(bits) -> int:
    """Payload checksum of one slice's 0/1 bit vector (host only)."""
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1)
    return zlib.crc32(np.packbits(bits, bitorder="little").tobytes()) & 0xFFFFFFFF


def payload_crc32_packed(words: np.ndarray, nbits: int) -> int:
    """payload_crc32 of the first nbits bits of one row of framing.pack_bits' packing (or of an
    extract's payload row) without unpacking it; bits past nbits in the last byte are ignored."""
    raw = np.ascontiguousarray(words).view(np.uint8).reshape(-1)
    nbits = int(nbits)
    nb = (nbits + 7) // 8
    if nb > raw.size:
        raise ValueError(f"{nbits} bits do not fit the row's {raw.size} bytes")
    if nbits % 8 == 0:
        return zlib.crc32(raw[:nb].tobytes()) & 0xFFFFFFFF
    last = bytes([int(raw[nb - 1]) & ((1 << (nbits % 8)) - 1)])
    return zlib.crc32(last, zlib.crc32(raw[:nb - 1].tobytes())) & 0xFFFFFFFF


def cover_crc32_host(image: np.ndarray) -> int:
    """The cover checksum of one slice computed on the host (zlib): what crc32_slices gives."""
    a = np.ascontiguousarray(image)
    return zlib.crc32(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()) & 0xFFFFFFFF


def verify_mode(verify) -> Optional[str]:
    """Normalise decode's `verify`: False -> None, True -> 'present', 'require' -> 'require'."""
    if verify is False:
        return None
    if verify is True:
        return "present"
    if verify == "require":
        return "require"
    raise ValueError("verify must be True, False or 'require'")


def raise_mismatch(bad_cover, bad_payload, what: str = "MED-PEE decode"):
    """IntegrityError naming the slices whose cover / payload checksum failed (none: returns)."""
    if not bad_cover and not bad_payload:
        return
    parts = []
    if bad_cover:
        parts.append(f"cover checksum mismatch in slices {list(bad_cover)}")
    if bad_payload:
        parts.append(f"payload checksum mismatch in slices {list(bad_payload)}")
    raise IntegrityError(f"{what}: {'; '.join(parts)} (CRC-32: this is not what was embedded)")
