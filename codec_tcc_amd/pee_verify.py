"""What follows a MED-PEE extract, written once ("One path after the extract"):
PeeCodec.decode (both schemes), PeeCodec.decode_volume and pipeline.decode_bin_pee hand the
restored cover and the extracted rows to after_extract() and get the rows back on the host, or
the error.  Nothing of a call is kept on the codec: values come in as arguments and leave as
return values or as attributes of the exception."""
from __future__ import annotations

from typing import List

from . import aead as _aead, checksum as _ck
from .codec import _torch

LOOKBACK_TIMEOUT = ("codec_pee_extract: in-place cursor look-back timed out; the recovered payload is invalid "
                    "(the restored cover is exact)")


def check_require(mode, keyed: bool, have_c: bool, have_p: bool, what: str = "MED-PEE decode",
                  carrier: str = "the embedding", named: bool = True):
    """verify='require' with a checksum absent and no tag to stand in for it: IntegrityError
    before any launch.  named=False (a file: both or none): the text names no checksum."""
    if mode != "require" or keyed or (have_c and have_p):
        return
    missing = " / ".join(n for n, h in (("cover", have_c), ("payload", have_p)) if not h)
    raise _ck.IntegrityError(f"{what}: verify='require' and {carrier} carries no "
                             + (f"{missing} checksum" if named else "checksums"))


def check_key(keyed: bool, key, noun: str = "embedding", has: str = "enc.tag", lacks: str = "enc.tag"):
    """decode's key= against what is decoded, before any launch: the checked key, or None for
    an unkeyed one.  ValueError when one is there without the other."""
    if keyed and key is None:
        raise ValueError(f"the {noun} is keyed ({has}): decode it with key=")
    if not keyed and key is not None:
        raise ValueError(f"key= given for a{'n' if noun[0] in 'aeiou' else ''} {noun} that is not keyed (no {lacks})")
    return _aead.check_key(key) if keyed else None


def tile_maps(enc, cover, bad):
    """IntegrityError.tiles of a failed verify: None without a tile table, {} when no cover
    failed, else the differing-tile maps of the slices in `bad` -- the only place a decode runs
    the tile pass (crc32_tiles on the restored cover + compare_tiles, one read-back of counts and
    bitmap).  A table still on the host (a file header's, an ndarray) is uploaded here, so only
    once a cover has failed."""
    table = enc.cover_tile_crc
    if table is None:
        return None
    if not bad:
        return {}
    if not hasattr(table, "detach"):
        table = _torch().from_numpy(table).to(cover.device)
    return _ck.tile_mismatch_maps(cover, table, enc.tile, bad)


def cover_mismatches(got, want, B: int) -> List[int]:
    """Slices whose restored cover's CRC-32 (got: crc32_slices' device tensor) differs from the
    stated one (want: a device tensor -- one read-back for both -- or a host list)."""
    if hasattr(want, "detach"):
        if want.numel() != B:
            raise ValueError(f"{want.numel()} cover checksums for {B} slices")
        both = _ck.crc_list(_torch().cat([got, want.reshape(-1).to(got)]))
        got, want = both[:B], both[B:]
    else:
        got, want = _ck.crc_list(got), [int(v) & 0xFFFFFFFF for v in want]
        if len(want) != B:
            raise ValueError(f"{len(want)} cover checksums for {B} slices")
    return [b for b in range(B) if got[b] != want[b]]


def _keyed_stream(ctx, enc, vol, cover, rows, total_t, verify: bool):
    """A keyed volume's launches: the stream is one row at the reserved index, tagged over the
    device-side total; every cover has a tag with an empty ciphertext -- so two releases.
    Returns the device tensors of the one read-back: plaintext, [ok of the stream, ok per cover]."""
    torch = _torch()
    if not verify:
        return [_aead.chacha20_rows(ctx, rows, total_t, _aead.STREAM_INDEX)]
    B = cover.shape[0]
    stag = _aead.poly1305_tags(ctx, None, rows, total_t, _aead.STREAM_INDEX)
    ctag = _aead.poly1305_tags(ctx, cover, index0=enc.index0)
    pt, ok_s = _aead.release(ctx, stag, vol.tag, rows, total_t, _aead.STREAM_INDEX)
    none = torch.zeros((B, 1), dtype=torch.int64, device=cover.device)   # the covers' tags: an empty CT
    _z, ok_c = _aead.release(ctx, ctag, enc.tag, none, torch.zeros(B, dtype=torch.int32, device=cover.device), enc.index0)
    return [pt, ok_s, ok_c]


def _keyed_slices(ctx, enc, cover, rows, verify: bool):
    """A keyed embedding's launches: decrypt only, or tags over the restored cover and the
    extracted rows, then the release (rows of a slice whose tag differs are zeroed on the device)."""
    torch = _torch()
    lens_t = torch.tensor([int(n) for n in enc.lengths], dtype=torch.int32, device=cover.device)
    if not verify:
        return [_aead.chacha20_rows(ctx, rows, lens_t, enc.index0)]
    got = _aead.poly1305_tags(ctx, cover, rows, lens_t, enc.index0)
    return list(_aead.release(ctx, got, enc.tag, rows, lens_t, enc.index0))


def after_extract(codec, enc, cover, words, mode, key, *, what: str = "MED-PEE decode", lookback: bool = True, vol=None):
    """The sequence behind an extract.  cover, words: what was extracted (device); a volume
    (vol given) hands its stream as one row with the device-side total in the word behind it.
    enc (and vol) state the embedding: cover_crc (device tensor or host list), payload_crc,
    cover_tile_crc / tile, tag / nonce / index0, lengths.  mode: checksum.verify_mode();
    key: check_key()'s.  what opens the messages; lookback: the extract can leave the flag.
      1. crc32_slices(cover), queued behind the extract, when a cover CRC is to be verified;
      2. the keyed launches (mode None: decrypt only; else tags, then release);
      3. ONE read-back of the rows, with ok;
      4. the look-back flag: reset() and RuntimeError;
      5. the keyed failure, 6. the CRC comparison -- IntegrityError, with tile maps when a table
         exists (step 6: only for covers that failed), .rows = the rows as step 3 brought them.
    Returns (rows on the host, the stream's total or None)."""
    B, verify, stream = codec.B, mode is not None, vol is not None
    got_crc = _ck.crc32_slices(cover) if verify and enc.cover_crc is not None else None
    n = words.numel() - stream   # the words to decrypt: all but a stream's total
    if key is None:   # the launch-bound case: the read-back and nothing else
        host = words.cpu().numpy().reshape(-1)
    else:
        torch = _torch()
        flat = words.reshape(-1)
        ctx = _aead.upload_ctx(key, enc.nonce, codec.device)
        parts = _keyed_stream(ctx, enc, vol, cover, flat[:n].reshape(1, n), flat[n:].view(torch.int32)[:1], verify) \
            if stream else _keyed_slices(ctx, enc, cover, words, verify)
        parts[1:1] = [flat[n:]] if stream else []
        dev = parts[0] if len(parts) == 1 else torch.cat([p.reshape(-1).to(torch.int64) for p in parts])
        host = dev.cpu().numpy().reshape(-1)
    host_rows = host[:n] if stream else host[:n].reshape(words.shape)
    total = min(int(host[n:n + 1].view("int32")[0]), int(vol.total_bits)) if stream else None
    if lookback and codec.lookback_failed(enc.payload_words):
        codec.reset()
        raise RuntimeError(LOOKBACK_TIMEOUT)
    shape = (codec.H, codec.W)
    if key is not None and verify:
        ok = host[n + stream:]
        bad_stream = stream and not ok[0]
        bad = [b for b in range(B) if not ok[b + stream]]
        if bad or bad_stream:
            tiles = tile_maps(enc, cover, bad)
            where = f"in slices {bad}" if not stream else "for " + " and ".join(
                ([f"the covers of slices {bad}"] if bad else []) + (["the stream"] if bad_stream else []))
            raise _ck.IntegrityError(
                f"{what}: authentication failed {where} (Poly1305 tag mismatch: wrong key or nonce, or cover / payload "
                f"/ tag altered)" + _ck.tiles_text(tiles, enc.tile, shape),
                slices=bad, keyed=True, stream=bad_stream, tiles=tiles, tile=enc.tile, rows=host_rows)
    if verify:
        bad_c = cover_mismatches(got_crc, enc.cover_crc, B) if got_crc is not None else []
        bad_p, bad_s = [], False
        if stream:
            bad_s = vol.payload_crc is not None and \
                _ck.payload_crc32_packed(host_rows, total) != int(vol.payload_crc) & 0xFFFFFFFF
        elif enc.payload_crc is not None:
            if len(enc.payload_crc) != B:
                raise ValueError(f"{len(enc.payload_crc)} payload checksums for {B} slices")
            bad_p = [b for b in range(B) if _ck.payload_crc32_packed(host_rows[b], enc.lengths[b])
                     != int(enc.payload_crc[b]) & 0xFFFFFFFF]
        if bad_c or bad_p or bad_s:
            _ck.raise_mismatch(bad_c, bad_p, what, tiles=tile_maps(enc, cover, bad_c), tile=enc.tile, shape=shape,
                               stream=bad_s, rows=host_rows)
    return host_rows, total
