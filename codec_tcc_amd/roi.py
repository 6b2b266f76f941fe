"""Regions of interest for MED-PEE (include/codec_tcc_roi.h): a per-slice pixel
rectangle that the embed never modifies.

    roi = roi_bbox(masks, level=0, margin=4)            # device int32 [B, 4], from a mask or a cover
    enc = codec.embed(covers, payloads, roi=roi)        # or roi=(y0, x0, y1, x1) for every slice
    bits, cover = codec.decode(enc)                     # the rectangle travels in the records
    enc.roi                                             # [(y0, x0, y1, x1), ...] read from them

A rectangle is half-open, (y0, x0, y1, x1) with 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W; an
empty one (y0 == y1 or x0 == x1) is "no ROI" and normalises to (0, 0, 0, 0).  The record carries
it as two unsigned words, reserved[0] = y0 << 16 | x0 and reserved[2] = y1 << 16 | x1
(reserved[2] == 0: none), hence H, W <= 65535.

normalize_roi, pack_words and unpack_words are pure host code: no GPU, no library load.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

ROI_MAX_DIM = 65535
FIELDS = ("y0", "x0", "y1", "x1")


def check_roi_shape(H: int, W: int) -> None:
    """ROI calls take H, W <= 65535 (the record words hold 16 bits per coordinate): ValueError
    before any device operation."""
    if int(H) > ROI_MAX_DIM or int(W) > ROI_MAX_DIM:
        raise ValueError(f"a ROI call takes H, W <= {ROI_MAX_DIM} (the record carries 16 bits per coordinate), "
                         f"got {int(H)} x {int(W)}")


def normalize_roi(roi, B: int, H: int, W: int) -> Optional[np.ndarray]:
    """None, one (y0, x0, y1, x1) for every slice, or a [B, 4] array / list / device tensor ->
    None or a host int32 [B, 4] array with every empty rectangle as (0, 0, 0, 0).  A device
    tensor is read back (one sync): the library cannot judge device values, so this layer does.
    Raises ValueError naming slice and field."""
    if roi is None:
        return None
    B, H, W = int(B), int(H), int(W)
    check_roi_shape(H, W)
    if hasattr(roi, "detach"):   # a torch tensor, any device
        if roi.is_floating_point() or roi.dtype.is_complex or str(roi.dtype) == "torch.bool":
            raise ValueError(f"roi must hold integers, got {roi.dtype}")
        roi = roi.detach().cpu().numpy()
    a = np.asarray(roi)
    if a.dtype == object or a.dtype.kind not in "iu":
        raise ValueError(f"roi must hold integers (y0, x0, y1, x1), got {a.dtype}")
    if a.ndim == 1:
        if a.shape != (4,):
            raise ValueError(f"one rectangle is (y0, x0, y1, x1), got {a.shape[0]} values")
        a = np.broadcast_to(a, (B, 4))
    if a.shape != (B, 4):
        raise ValueError(f"roi must be one (y0, x0, y1, x1) or [B, 4] = [{B}, 4], got shape {tuple(a.shape)}")
    a = a.astype(np.int64)
    lim = (H, W, H, W)
    for b in range(B):
        for f in range(4):
            v = int(a[b, f])
            if not 0 <= v <= lim[f]:
                raise ValueError(f"roi of slice {b}: {FIELDS[f]} = {v} (0..{lim[f]} on a {H} x {W} slice)")
        if a[b, 0] > a[b, 2]:
            raise ValueError(f"roi of slice {b}: y0 = {int(a[b, 0])} (above y1 = {int(a[b, 2])})")
        if a[b, 1] > a[b, 3]:
            raise ValueError(f"roi of slice {b}: x0 = {int(a[b, 1])} (above x1 = {int(a[b, 3])})")
    out = np.ascontiguousarray(a, dtype=np.int32).copy()   # dense row-major [B, 4]: one 4-tuple arrives as a stride-0 broadcast
    out[(out[:, 0] == out[:, 2]) | (out[:, 1] == out[:, 3])] = 0
    return out


class PackedRoi:
    """Rectangles already judged and uploaded (PeeCodec.pack_roi): embed(..., roi=) takes one as it
    comes -- no read-back, no upload in the call, so the call can be captured into a graph.
    host: the normalised int32 [B, 4] array; device: the same values on the GPU."""

    def __init__(self, host: np.ndarray, device):
        self.host, self.device = host, device


def pack_words(rect) -> Tuple[int, int]:
    """(reserved[0], reserved[2]) of one rectangle as unsigned bit patterns; an empty one gives (0, 0)."""
    y0, x0, y1, x1 = (int(v) for v in rect)
    if not (0 <= y0 <= y1 <= ROI_MAX_DIM and 0 <= x0 <= x1 <= ROI_MAX_DIM):
        raise ValueError(f"no rectangle of at most {ROI_MAX_DIM} pixels a side: {(y0, x0, y1, x1)}")
    if y0 == y1 or x0 == x1:
        return 0, 0
    return (y0 << 16) | x0, (y1 << 16) | x1


def unpack_words(w0: int, w2: int) -> Tuple[int, int, int, int]:
    """(y0, x0, y1, x1) of a record's reserved[0] and reserved[2] (signed or unsigned);
    reserved[2] == 0 is "no ROI": (0, 0, 0, 0)."""
    w0, w2 = int(w0) & 0xFFFFFFFF, int(w2) & 0xFFFFFFFF
    if w2 == 0:
        return 0, 0, 0, 0
    return w0 >> 16, w0 & 0xFFFF, w2 >> 16, w2 & 0xFFFF


def as_signed(word: int) -> int:
    """An unsigned record word as the int32 a codec_pee_meta field holds."""
    word = int(word) & 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word


def record_roi(rec) -> Tuple[int, int, int, int]:
    """The rectangle a scheme-1 record carries."""
    return unpack_words(rec.reserved[0], rec.reserved[2])


def records_roi(recs) -> List[Tuple[int, int, int, int]]:
    return [record_roi(r) for r in recs]


def roi_bbox(images, level: int = 0, margin: int = 0):
    """Device int32 [B, 4]: per slice the tight bounding rectangle (y0, x0, y1, x1) of the pixels
    with value > level, grown by margin >= 0 pixels on every side and clamped to the image;
    (0, 0, 0, 0) for a slice without such a pixel.  images: a [B, H, W] (or [H, W]) uint8 /
    uint16 tensor on the GPU, contiguous (at any storage offset) -- a segmentation mask (level
    0) or a cover thresholded against its background.  One read-only pass on the current
    stream (codec_roi_bbox): no allocation besides the result, no sync, capturable."""
    from . import _lib
    from .codec import _elem_bytes, _require_gpu, _stream, _torch
    torch = _torch()
    if isinstance(level, bool) or int(level) != level or not 0 <= int(level) <= 65535:
        raise ValueError(f"level must be an integer in 0..65535, got {level!r}")
    if isinstance(margin, bool) or int(margin) != margin or not 0 <= int(margin) <= 65535:
        raise ValueError(f"margin must be an integer in 0..65535, got {margin!r}")
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"images must be a torch tensor on the GPU, got {type(images).__name__}")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or min(images.shape) < 1:
        raise ValueError(f"images must be [B, H, W] with no empty dimension, got shape {tuple(images.shape)}")
    if images.dtype not in (torch.uint8, torch.uint16, torch.int16):
        raise ValueError(f"images must hold uint8 or uint16 pixels, got {images.dtype}")
    if not images.is_contiguous():
        raise ValueError(f"images must be contiguous (a dense [B, H, W] block at any storage offset), got strides "
                         f"{tuple(images.stride())}")
    B, H, W = (int(v) for v in images.shape)
    check_roi_shape(H, W)
    _require_gpu()
    if images.device.type != "cuda":
        raise TypeError(f"images is on {images.device}: roi_bbox runs on the GPU")
    nbytes = _elem_bytes(images)
    out = torch.empty((B, 4), dtype=torch.int32, device=images.device)
    P = _lib.PeeParams(B=B, H=H, W=W, bytes=nbytes, T=1, maxval=65535 if nbytes == 2 else 255, payload_words=1,
                       lm_words=max(1, ((H // 2) * (W // 2) + 63) // 64))
    _lib.check(_lib.load().codec_roi_bbox(C.byref(P), images.data_ptr(), int(level), int(margin), out.data_ptr(),
                                          _stream()), "codec_roi_bbox")
    return out
