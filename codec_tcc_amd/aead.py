"""Keyed MED-PEE: ChaCha20-Poly1305 (RFC 8439) over payload rows and covers
(include/codec_tcc_aead.h; the specification is tests/aead_spec.py).

The slice's cover is the associated data, the payload row the plaintext; the stego carries the
ciphertext and a 16-byte tag travels with the records.  A caller gives a 32-byte key and an
8-byte nonce; slice b of a call has the global index index0 + b (the nonce of RFC 8439 is
LE32(index) || nonce), and 0x80000000 is reserved for a volume's stream.

Key and nonce live in a 48-byte block in DEVICE memory (upload_ctx): they never enter a kernel's
argument list, and a captured graph is replayed under a fresh nonce by rewriting the block
(write_ctx).  Replaying a captured graph without rewriting it reuses the nonce.

Everything here is queued on the current stream; no tag is ever compared on the host (release).
There is no CPU fallback.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from . import _lib
from .codec import _require_gpu, _stream, _torch

KEY_BYTES, NONCE_BYTES, TAG_WORDS = 32, 8, 4
STREAM_INDEX = _lib.AEAD_STREAM_INDEX


def check_key(key) -> bytes:
    """The key as bytes: exactly 32 (ValueError otherwise; str is refused, not encoded)."""
    if not isinstance(key, (bytes, bytearray)) or len(key) != KEY_BYTES:
        raise ValueError(f"key must be {KEY_BYTES} bytes (bytes or bytearray)")
    return bytes(key)


def check_nonce(nonce) -> bytes:
    if not isinstance(nonce, (bytes, bytearray)) or len(nonce) != NONCE_BYTES:
        raise ValueError(f"nonce must be {NONCE_BYTES} bytes (bytes or bytearray)")
    return bytes(nonce)


def fresh_nonce() -> bytes:
    return os.urandom(NONCE_BYTES)


def check_index(index0, B: int = 1) -> int:
    """index0 when slices index0 .. index0 + B - 1 are all < 2^31, or the call is the stream's
    (STREAM_INDEX with B = 1); ValueError otherwise."""
    if isinstance(index0, bool) or not isinstance(index0, (int, np.integer)):
        raise ValueError(f"index0 must be an integer, got {index0!r}")
    index0, B = int(index0), int(B)
    if index0 == STREAM_INDEX and B == 1:
        return index0
    if index0 < 0 or index0 + B > 1 << 31:
        raise ValueError(f"slice indices {index0} .. {index0 + B - 1} must lie in 0 .. 2^31 - 1 "
                         f"(0x80000000 is reserved for a volume's stream)")
    return index0


def check_call(key, nonce, index0=0, B: int = 1, *, fresh: bool = True,
               lone: Optional[str] = "nonce= and index0= go with key="):
    """(key, nonce, index0) of a call's key= / nonce= / index0=, judged before anything is queued.
    key=None: the other two must be absent (ValueError `lone`; lone=None leaves that to a later
    check).  fresh: a missing nonce is drawn from os.urandom."""
    if key is None:
        if lone and (nonce is not None or index0 != 0):
            raise ValueError(lone)
        return None, nonce, index0
    key = check_key(key)
    nonce = (fresh_nonce() if fresh else None) if nonce is None else check_nonce(nonce)
    return key, nonce, check_index(index0, B)


def ctx_bytes(key, nonce) -> bytes:
    """The 48-byte codec_aead_ctx of (key, nonce) (pure host)."""
    return check_key(key) + check_nonce(nonce) + bytes(8)


def upload_ctx(key, nonce, device=None):
    """A device uint8 [48] tensor holding the call's codec_aead_ctx.  key / nonce are judged
    first: ValueError before anything is queued."""
    raw = ctx_bytes(key, nonce)
    _require_gpu()
    torch = _torch()
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device if device is not None else "cuda")


def write_ctx(ctx, key, nonce):
    """Rewrite a context block in place (a copy queued on the current stream): the way to replay a
    captured graph under a fresh nonce."""
    raw = ctx_bytes(key, nonce)
    torch = _torch()
    _check_ctx(ctx)
    ctx.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8), non_blocking=False)
    return ctx


def _check_ctx(ctx):
    torch = _torch()
    if not isinstance(ctx, torch.Tensor) or ctx.dtype != torch.uint8 or ctx.numel() != _lib.AEAD_CTX_BYTES \
            or not ctx.is_cuda or not ctx.is_contiguous() or ctx.data_ptr() % 4:
        raise ValueError("ctx must be upload_ctx()'s tensor: 48 contiguous uint8 on the GPU")


def _check_rows(rows, lengths, what: str):
    torch = _torch()
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 2 or not rows.is_cuda \
            or not rows.is_contiguous() or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError(f"{what}: rows must be a contiguous int64 [B, row_words] tensor on the GPU")
    if rows.shape[1] > _lib.AEAD_MAX_ROW_WORDS:
        raise ValueError(f"{what}: a row holds at most 2^31 - 1 bits ({_lib.AEAD_MAX_ROW_WORDS} words)")
    B = int(rows.shape[0])
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) \
            or not lengths.is_contiguous() or lengths.device != rows.device:
        raise ValueError(f"{what}: lengths must be a contiguous int32 [{B}] tensor on the rows' device")
    return B, int(rows.shape[1])


def _check_out(out, like, name: str):
    if out is None:
        return _torch().empty_like(like)
    if out.dtype != like.dtype or out.shape != like.shape or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"{name} must match the rows: contiguous {like.dtype} {tuple(like.shape)} on {like.device}")
    return out


def _check_tags(t, B: int, device, name: str):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B, TAG_WORDS) \
            or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous int32 [{B}, {TAG_WORDS}] tensor on {device}")
    return t


def chunk_bytes() -> int:
    """Bytes of one slice's AAD one workgroup of the Poly1305 pass covers."""
    return int(_lib.load().codec_poly1305_chunk_bytes())


def chacha20_rows(ctx, rows, lengths, index0: int = 0, out=None):
    """rows [B, row_words] int64 xor the keystream of slices index0 .. on their first lengths[b]
    bits, zero past them (its own inverse).  out may be rows; a new tensor when None."""
    _require_gpu()
    _check_ctx(ctx)
    B, rw = _check_rows(rows, lengths, "chacha20_rows")
    index0 = check_index(index0, B)
    out = _check_out(out, rows, "out")
    _lib.check(_lib.load().codec_chacha20_rows(ctx.data_ptr(), B, index0, rows.data_ptr(), rw, lengths.data_ptr(),
                                               out.data_ptr(), _stream()), "codec_chacha20_rows")
    return out


def _aad_args(aad, B: Optional[int], what: str):
    torch = _torch()
    if aad is None:
        return None, 0, B
    if not isinstance(aad, torch.Tensor) or not aad.is_cuda or not aad.is_contiguous() or aad.dim() < 1 \
            or aad.shape[0] < 1 or aad.numel() == 0:
        raise ValueError(f"{what}: aad must be a contiguous [B, ...] tensor on the GPU (the tag is of the bytes as they lie)")
    if B is not None and int(aad.shape[0]) != B:
        raise ValueError(f"{what}: {int(aad.shape[0])} slices of associated data for {B} rows")
    B = int(aad.shape[0])
    return aad.data_ptr(), aad.numel() // B * aad.element_size(), B


def _tags(fn_name: str, aad, rows, lengths, out):
    """The arguments the two tag calls share, judged; the output and the workspace allocated."""
    _require_gpu()
    torch = _torch()
    B = rp = lp = None
    rw = 0
    if rows is not None or lengths is not None:
        B, rw = _check_rows(rows, lengths, fn_name)
        rp, lp = rows.data_ptr(), lengths.data_ptr()
    ap, nbytes, B = _aad_args(aad, B, fn_name)
    if B is None:
        raise ValueError(f"{fn_name}: neither associated data nor rows")
    device = aad.device if aad is not None else rows.device
    out = torch.empty((B, TAG_WORDS), dtype=torch.int32, device=device) if out is None else _check_tags(out, B, device, "out")
    lib = _lib.load()
    ws = int(lib.codec_aead_workspace_bytes(B, nbytes, rw))
    if ws == 0:
        raise ValueError(f"{fn_name}: a batch of {B} slices of {nbytes} bytes is beyond the kernel's limits")
    work = torch.empty(ws, dtype=torch.uint8, device=device)
    return lib, B, ap, nbytes, rp, rw, lp, out, work, ws


def poly1305_tags(ctx, aad, rows=None, lengths=None, index0: int = 0, out=None):
    """int32 [B, 4] device tensor: the tags (16 bytes as little-endian words) of slices index0 ..:
    AAD = slice b of `aad` ([B, ...], any dtype, or None), CT = the first lengths[b] bits of
    rows[b] (or none).  Read-only on both."""
    _check_ctx(ctx)
    lib, B, ap, nbytes, rp, rw, lp, out, work, ws = _tags("poly1305_tags", aad, rows, lengths, out)
    index0 = check_index(index0, B)
    _lib.check(lib.codec_poly1305_tags(ctx.data_ptr(), B, index0, ap, nbytes, rp, rw, lp, out.data_ptr(), work.data_ptr(),
                                       ws, _stream()), "codec_poly1305_tags")
    return out


def poly1305_tags_otk(otk, aad, rows=None, lengths=None, out=None):
    """poly1305_tags with the one-time keys given: otk int32 [B, 8] on the GPU (r unclamped, then s)."""
    torch = _torch()
    lib, B, ap, nbytes, rp, rw, lp, out, work, ws = _tags("poly1305_tags_otk", aad, rows, lengths, out)
    if not isinstance(otk, torch.Tensor) or otk.dtype != torch.int32 or tuple(otk.shape) != (B, 8) or not otk.is_cuda \
            or not otk.is_contiguous():
        raise ValueError(f"otk must be a contiguous int32 [{B}, 8] tensor on the GPU")
    _lib.check(lib.codec_poly1305_tags_otk(otk.data_ptr(), B, ap, nbytes, rp, rw, lp, out.data_ptr(), work.data_ptr(), ws,
                                           _stream()), "codec_poly1305_tags_otk")
    return out


def release(ctx, tags_got, tags_want, rows, lengths, index0: int = 0, out=None, ok=None):
    """(plaintext rows, ok): ok int32 [B] = 1 where all 128 bits of the two tags agree; the row
    decrypted there, all zeros elsewhere.  The comparison runs on the device, branch-free."""
    _require_gpu()
    torch = _torch()
    _check_ctx(ctx)
    B, rw = _check_rows(rows, lengths, "release")
    index0 = check_index(index0, B)
    _check_tags(tags_got, B, rows.device, "tags_got")
    _check_tags(tags_want, B, rows.device, "tags_want")
    out = _check_out(out, rows, "out")
    if ok is None:
        ok = torch.empty(B, dtype=torch.int32, device=rows.device)
    elif ok.dtype != torch.int32 or tuple(ok.shape) != (B,) or not ok.is_contiguous() or ok.device != rows.device:
        raise ValueError(f"ok must be a contiguous int32 [{B}] tensor on the rows' device")
    _lib.check(_lib.load().codec_aead_release(ctx.data_ptr(), B, index0, tags_got.data_ptr(), tags_want.data_ptr(),
                                              rows.data_ptr(), rw, lengths.data_ptr(), out.data_ptr(), ok.data_ptr(),
                                              _stream()), "codec_aead_release")
    return out, ok


# ------------------------------------------------------------------ one nonce per slice (include/codec_tcc_blind_keyed.h)
def _check_nonce12(n12, B: int, device):
    torch = _torch()
    if not isinstance(n12, torch.Tensor) or n12.dtype != torch.int32 or tuple(n12.shape) != (B, 3) \
            or not n12.is_contiguous() or n12.device != device:
        raise ValueError(f"nonce12 must be a contiguous int32 [{B}, 3] tensor on {device}: (g, nonce word 0, nonce word 1)")
    return n12


def nonce12_rows(nonce, index0: int, B: int, device=None):
    """int32 [B, 3] device tensor: (index0 + b, the nonce's two little-endian words), i.e. what the
    calls that take (nonce, index0) use for slice b."""
    nonce = check_nonce(nonce)
    index0 = check_index(index0, B)
    _require_gpu()
    torch = _torch()
    w = np.frombuffer(nonce, dtype="<u4").astype(np.int64)
    rows = np.stack([(index0 + np.arange(B, dtype=np.int64)) & 0xFFFFFFFF, np.full(B, w[0]), np.full(B, w[1])], axis=1)
    return torch.from_numpy(rows.astype(np.uint32).view(np.int32)).to(device if device is not None else "cuda")


def chacha20_rows_n(ctx, nonce12, rows, lengths, out=None):
    """chacha20_rows with slice b under nonce12[b] = (g, nonce words) and ctx's key (ctx's own nonce
    is ignored).  No index rule: a decoder takes g from the stego."""
    _require_gpu()
    _check_ctx(ctx)
    B, rw = _check_rows(rows, lengths, "chacha20_rows_n")
    _check_nonce12(nonce12, B, rows.device)
    out = _check_out(out, rows, "out")
    _lib.check(_lib.load().codec_chacha20_rows_n(ctx.data_ptr(), B, nonce12.data_ptr(), rows.data_ptr(), rw, lengths.data_ptr(),
                                                 out.data_ptr(), _stream()), "codec_chacha20_rows_n")
    return out


def poly1305_tags_n(ctx, nonce12, aad, rows=None, lengths=None, out=None):
    """poly1305_tags with slice b's one-time key derived under nonce12[b]."""
    _check_ctx(ctx)
    lib, B, ap, nbytes, rp, rw, lp, out, work, ws = _tags("poly1305_tags_n", aad, rows, lengths, out)
    _check_nonce12(nonce12, B, out.device)
    _lib.check(lib.codec_poly1305_tags_n(ctx.data_ptr(), B, nonce12.data_ptr(), ap, nbytes, rp, rw, lp, out.data_ptr(),
                                         work.data_ptr(), ws, _stream()), "codec_poly1305_tags_n")
    return out


def release_n(ctx, nonce12, tags_got, tags_want, rows, lengths, out=None, ok=None):
    """release with slice b decrypted under nonce12[b]."""
    _require_gpu()
    torch = _torch()
    _check_ctx(ctx)
    B, rw = _check_rows(rows, lengths, "release_n")
    _check_nonce12(nonce12, B, rows.device)
    _check_tags(tags_got, B, rows.device, "tags_got")
    _check_tags(tags_want, B, rows.device, "tags_want")
    out = _check_out(out, rows, "out")
    if ok is None:
        ok = torch.empty(B, dtype=torch.int32, device=rows.device)
    elif ok.dtype != torch.int32 or tuple(ok.shape) != (B,) or not ok.is_contiguous() or ok.device != rows.device:
        raise ValueError(f"ok must be a contiguous int32 [{B}] tensor on the rows' device")
    _lib.check(_lib.load().codec_aead_release_n(ctx.data_ptr(), B, nonce12.data_ptr(), tags_got.data_ptr(),
                                                tags_want.data_ptr(), rows.data_ptr(), rw, lengths.data_ptr(), out.data_ptr(),
                                                ok.data_ptr(), _stream()), "codec_aead_release_n")
    return out, ok


def tag_bytes(tags) -> list:
    """The tags of a poly1305_tags() tensor as 16-byte strings (one read-back)."""
    raw = tags.detach().cpu().contiguous().numpy().astype("<i4").tobytes()
    return [raw[16 * i:16 * i + 16] for i in range(len(raw) // 16)]
