"""ctypes binding of libcodec_hip.so (include/codec_tcc.h, include/codec_tcc_ext.h,
include/codec_tcc_crc.h, include/codec_tcc_vol.h, include/codec_tcc_gate.h, include/codec_tcc_gvol.h,
include/codec_tcc_tile.h, include/codec_tcc_roi.h, include/codec_tcc_aead.h, include/codec_tcc_blind.h,
include/codec_tcc_blind_auto.h, include/codec_tcc_blind_keyed.h, include/codec_tcc_blind_vol.h,
include/codec_tcc_blind_gate.h).

The library is built in-tree (codec_tcc_amd/libcodec_hip.so, see build.py).  There is no
CPU fallback: if the library cannot be loaded, every entry point raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CODEC_TCC_LIB: an alternative build of the same library (A/B benchmarking, tools/archive/ab_bench.sh)
_DEFAULT_PATH = os.path.join(_HERE, "libcodec_hip.so")
LIB_PATH = os.environ.get("CODEC_TCC_LIB") or _DEFAULT_PATH

MAX_PLANES = 16
MODE_HYBRID = 0
MODE_MULTI = 1
FLAG_OVERLAP = 1
FLAG_LOSSY = 2
FLAG_BADLUT = 4
FLAG_DECIDE_TIMEOUT = 8   # split decision: a plane workgroup never reported (status 2)
FLAG_INFO_FAST = 16      # s decided by the guard band: mi[] = H(X), cum_info their sum
FLAG_GUARD_FALLBACK = 32 # a prefix within 1e-9 of the target: the exact numpy-order sums decided

I16 = C.c_int32 * MAX_PLANES
D16 = C.c_double * MAX_PLANES


class Params(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("in_bytes", C.c_int32), ("out_bytes", C.c_int32), ("nbits", C.c_int32),
        ("block", C.c_int32), ("align", C.c_int32), ("mode", C.c_int32),
        ("fixed_s", C.c_int32), ("fixed_offset", C.c_int32), ("all_mi", C.c_int32),
        ("payload_words", C.c_int32), ("map_words", C.c_int32), ("n_classes", C.c_int32),
        ("reserved", C.c_int32), ("beta", C.c_double),
    ]


class Layout(C.Structure):
    _fields_ = [("sizes", I16), ("perm", I16), ("src", I16), ("len", I16)]


class SliceMeta(C.Structure):
    _fields_ = [
        ("s", C.c_int32), ("start_offset", C.c_int32), ("total_used", C.c_int32),
        ("flags", C.c_uint32), ("npix", C.c_int32), ("nbits", C.c_int32),
        ("status", C.c_int32), ("nonzero_bins", C.c_int32),
        ("perm", I16), ("sizes", I16), ("n", I16), ("src", I16), ("off", I16), ("cat", I16),
        ("entropy", C.c_double), ("target", C.c_double), ("cum_info", C.c_double),
        ("span_lo", C.c_int32), ("span_len", C.c_int32), ("mi", D16),
    ]


class PeeParams(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("bytes", C.c_int32),
                ("T", C.c_int32), ("maxval", C.c_int32), ("payload_words", C.c_int32), ("lm_words", C.c_int32)]


class PeeMeta(C.Structure):
    _fields_ = [("T", C.c_int32), ("maxval", C.c_int32), ("L", C.c_int32), ("end", C.c_int32),
                ("nc", C.c_int32), ("ntiles", C.c_int32), ("tile_end", C.c_int32), ("status", C.c_int32),
                ("capacity", C.c_int32), ("lm_count", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


def tuning_knob(name: str, default: int) -> int:
    """A Python-side launch-shape knob, honoured like the library's (include/codec_tcc.h,
    codec_set_tuning): the environment value only when CODEC_TUNING=1, else the default."""
    if os.environ.get("CODEC_TUNING", "0") != "1":
        return default
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default


PEE_PARTIAL = 1
PEE_RECORD_HDR_WORDS = 8   # CODEC_PEE_RECORD_HDR_WORDS: codec_pee_meta in uint64 words
META_BYTES = C.sizeof(SliceMeta)
PEE_META_BYTES = C.sizeof(PeeMeta)
CODEC_PEE_ELOOKBACK = 2  # meta.status: look-back gave up (include/codec_tcc.h)
LAYOUT_BYTES = C.sizeof(Layout)

_VP = C.c_void_p
_SIGS = {
    "codec_abi_version": (C.c_int, []),
    "codec_build_digest": (C.c_char_p, []),
    "codec_set_tuning": (C.c_int, [C.c_int32]),
    "codec_last_error": (C.c_char_p, []),
    "codec_workspace_bytes": (C.c_size_t, [C.POINTER(Params)]),
    "codec_plan": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_embed": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, _VP, _VP, _VP]),
    "codec_encode": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, C.c_size_t,
                               _VP, _VP, _VP]),
    "codec_extract": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, _VP, _VP, _VP]),
    "codec_refdecode": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
    "codec_refdecode_dense": (C.c_int, [C.POINTER(Params), _VP, C.c_int32, _VP, C.c_int32, _VP, _VP,
                                        C.c_int32, _VP, _VP]),
    "codec_expand_maps": (C.c_int, [C.POINTER(Params), _VP, _VP, _VP, C.c_int32, _VP]),
    "codec_restore_dense": (C.c_int, [C.POINTER(Params), _VP, _VP, C.c_int32, _VP, _VP, _VP]),
    "codec_unpack_planes": (C.c_int, [C.POINTER(Params), _VP, C.c_int32, C.c_int32, _VP, C.c_int32, _VP]),
    "codec_merge_planes": (C.c_int, [C.POINTER(Params), _VP, C.c_int32, C.c_int32, _VP, _VP]),
    "codec_pee_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams)]),
    "codec_pee_extract_flag_offset": (C.c_size_t, [C.POINTER(PeeParams)]),
    "codec_pee_diag_offset": (C.c_size_t, [C.POINTER(PeeParams)]),
    "codec_pee_reset": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_size_t, _VP]),
    "codec_debug_res_trace": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "codec_pee_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_embed_ts": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_capacity": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_embed_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP,
                                       C.c_size_t, _VP]),
    "codec_pee_multi_embed_pass": (C.c_int, [C.POINTER(PeeParams), C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                             C.c_size_t, _VP]),
    "codec_pee_multi_extract_pass": (C.c_int, [C.POINTER(PeeParams), C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                               C.c_size_t, _VP]),
    "codec_pee_multi_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_multi_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_pack_records": (C.c_int, [C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP]),
    "codec_pee_unpack_records": (C.c_int, [C.c_int32, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP]),
    "codec_quality_moments": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "codec_block_variance": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP]),
    "codec_lsb_runs": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, _VP, _VP, _VP, C.c_int64, _VP, C.c_int32, _VP]),
    "codec_profile_begin": (C.c_int, [C.c_int32]),
    "codec_profile_end": (C.c_int, [_VP, _VP, C.c_int32]),
}
KERNEL_TAGS = {1: "k_scan_fast", 2: "k_scan_generic", 3: "k_block_exact", 4: "k_decide",
               5: "k_embed", 6: "k_restore", 7: "k_gather", 8: "other", 9: "k_pee_scan", 10: "k_pee_locate",
               11: "k_pee_embed", 12: "k_pee_copy", 13: "k_pee_dcount", 14: "k_pee_recover",
               15: "k_pee_embed1", 16: "k_pee_extract1", 17: "k_scan_read", 18: "k_unxor",
               19: "k_scan_rows", 20: "k_scan_rows_read", 21: "k_quality", 22: "k_decide_embed",
               23: "k_pee_capacity", 24: "k_pee_embed_ss", 25: "k_pee_extract_ss",
               26: "k_pee_embed_ss_auto", 27: "k_pee_embed_res", 28: "k_scan_decide",
               29: "k_pee_lat_count", 30: "k_pee_lat_embed", 31: "k_pee_lat_dcount", 32: "k_pee_lat_recover",
               33: "k_pee_lat_ss_embed", 34: "k_pee_lat_ss_extract", 35: "k_pee_lat_auto",
               36: "k_crc32", 37: "k_crc32_combine", 38: "k_vol_plan", 39: "k_vol_scatter", 40: "k_vol_gather",
               41: "k_pee_gate_table", 42: "k_gvol_plan", 43: "k_tile_crc", 44: "k_tile_crc_bytes",
               45: "k_tile_compare", 46: "k_roi_bbox", 47: "k_chacha20_rows", 48: "k_poly1305_prep", 49: "k_poly1305",
               50: "k_poly1305_finish", 51: "k_aead_release", 52: "k_blind_rows", 53: "k_blind_rows_auto",
               54: "k_bvol_plan", 55: "k_bvol_rows", 56: "k_bvol_order", 57: "k_bvol_gather",
               58: "k_blind_rows_gate"}
EXPORTS = tuple(_SIGS)
# include/codec_tcc_ext.h: entries added after codec_tcc.h's list (EXPORTS) was fixed
_SIGS_EXT = {
    "codec_pee_multi_embed_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                             _VP, _VP, C.c_size_t, _VP]),
}
EXPORTS_EXT = tuple(_SIGS_EXT)
# include/codec_tcc_crc.h: the CRC-32 entries (checksum.py)
_SIGS_CRC = {
    "codec_crc32_chunk_bytes": (C.c_size_t, []),
    "codec_crc32_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "codec_crc32_slices": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_crc32_combine": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]),
}
EXPORTS_CRC = tuple(_SIGS_CRC)


class PeeVolumeInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("T", C.c_int32), ("total", C.c_int32), ("requested", C.c_int32),
                ("capacity", C.c_int32), ("policy", C.c_int32), ("B", C.c_int32), ("tmax", C.c_int32)]


PEE_VOLUME_INFO_BYTES = C.sizeof(PeeVolumeInfo)
VOL_POLICIES = {"even": 0, "fill": 1}   # CODEC_VOL_EVEN / CODEC_VOL_FILL
# include/codec_tcc_vol.h: MED-PEE volume payloads (pee.py embed_volume / decode_volume)
_SIGS_VOL = {
    "codec_pee_volume_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32]),
    "codec_pee_volume_plan": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP,
                                        _VP]),
    "codec_pee_volume_scatter": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "codec_pee_volume_gather": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_volume_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP,
                                         _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP, C.c_size_t, _VP]),
    "codec_pee_volume_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP,
                                           C.c_size_t, _VP, C.c_size_t, _VP]),
}
EXPORTS_VOL = tuple(_SIGS_VOL)
# include/codec_tcc_gate.h: smoothness-gated MED-PEE (pee.py, PeeCodec(gate=...))
GATES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535)   # the capacity table's ladder
GATE_TMAX = 16            # CODEC_PEE_GATE_TMAX
GATE_MAX = 65535          # CODEC_PEE_GATE_MAX
GATE_MAX_NC = 1 << 26     # CODEC_PEE_GATE_MAX_NC
_SIGS_GATE = {
    "codec_pee_gate_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32]),
    "codec_pee_gate_capacity": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP,
                                          _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_gate_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_gate_embed_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP,
                                            _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_gate_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
}
EXPORTS_GATE = tuple(_SIGS_GATE)


class PeeGvolInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("T", C.c_int32), ("total", C.c_int32), ("requested", C.c_int32),
                ("capacity", C.c_int32), ("policy", C.c_int32), ("B", C.c_int32), ("tmax", C.c_int32),
                ("gate", C.c_int32), ("reserved", C.c_int32)]


PEE_GVOL_INFO_BYTES = C.sizeof(PeeGvolInfo)
# include/codec_tcc_gvol.h: gated volume payloads (pee.py embed_volume(gate=...))
_SIGS_GVOL = {
    "codec_pee_gvol_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32]),
    "codec_pee_gvol_plan": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _VP,
                                      _VP, _VP, _VP, _VP, _VP]),
    "codec_pee_gvol_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP, C.c_size_t, _VP,
                                       C.c_size_t, _VP]),
    "codec_pee_gvol_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_size_t,
                                         _VP, C.c_size_t, _VP]),
}
EXPORTS_GVOL = tuple(_SIGS_GVOL)
# include/codec_tcc_tile.h: tile checksums (checksum.py crc32_tiles / compare_tiles)
TILE_MIN, TILE_MAX = 4, 1024            # CODEC_TILE_MIN / CODEC_TILE_MAX
TILE_ROUTE_BYTES, TILE_ROUTE_VECTOR = 1, 2   # CODEC_TILE_ROUTE_*
_SIGS_TILE = {
    "codec_crc32_tiles_grid": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32)]),
    "codec_crc32_tiles_route": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "codec_crc32_tiles": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP]),
    "codec_crc32_tiles_compare": (C.c_int, [C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
}
EXPORTS_TILE = tuple(_SIGS_TILE)
# include/codec_tcc_roi.h: ROI-protected MED-PEE (roi.py; pee.py, PeeCodec.embed(roi=...))
ROI_MAX_DIM = 65535       # CODEC_PEE_ROI_MAX_DIM
_SIGS_ROI = {
    "codec_pee_roi_capacity": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP,
                                         _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_roi_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t,
                                      _VP]),
    "codec_pee_roi_embed_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP,
                                           _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_roi_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_roi_bbox": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, C.c_int32, _VP, _VP]),
}
EXPORTS_ROI = tuple(_SIGS_ROI)


class AeadCtx(C.Structure):
    _fields_ = [("key", C.c_uint32 * 8), ("nonce", C.c_uint32 * 2), ("reserved", C.c_uint32 * 2)]


AEAD_CTX_BYTES = C.sizeof(AeadCtx)           # 48
AEAD_STREAM_INDEX = 0x80000000               # CODEC_AEAD_STREAM_INDEX
AEAD_MAX_ROW_WORDS = 1 << 25                 # CODEC_AEAD_MAX_ROW_WORDS
# include/codec_tcc_aead.h: keyed MED-PEE, ChaCha20-Poly1305 (aead.py; pee.py, PeeCodec.embed(key=...))
_SIGS_AEAD = {
    "codec_poly1305_chunk_bytes": (C.c_size_t, []),
    "codec_aead_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32]),
    "codec_chacha20_rows": (C.c_int, [_VP, C.c_int32, C.c_uint32, _VP, C.c_int32, _VP, _VP, _VP]),
    "codec_poly1305_tags": (C.c_int, [_VP, C.c_int32, C.c_uint32, _VP, C.c_int64, _VP, C.c_int32, _VP, _VP, _VP,
                                      C.c_size_t, _VP]),
    "codec_poly1305_tags_otk": (C.c_int, [_VP, C.c_int32, _VP, C.c_int64, _VP, C.c_int32, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_aead_release": (C.c_int, [_VP, C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
}
EXPORTS_AEAD = tuple(_SIGS_AEAD)
# include/codec_tcc_blind.h: blind MED-PEE (blind.py; pee.py, PeeCodec.embed_blind / decode_blind)
BLIND_MAGIC = 0x4D504231          # CODEC_PEE_BLIND_MAGIC
BLIND_HDR_WORDS = 6               # CODEC_PEE_BLIND_HDR_WORDS
BLIND_MAX_ENTRIES = 65536         # CODEC_PEE_BLIND_MAX_ENTRIES
BLIND_INFO_WORDS = 8              # CODEC_PEE_BLIND_INFO_WORDS
BLIND_FLAG_CRC = 1                # CODEC_PEE_BLIND_FLAG_CRC
_SIGS_BLIND = {
    "codec_pee_blind_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32]),
    "codec_pee_blind_plan": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, C.c_int32, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_blind_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP,
                                        _VP, C.c_size_t, _VP]),
    "codec_pee_blind_headers": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP]),
    "codec_pee_blind_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_size_t, _VP]),
}
EXPORTS_BLIND = tuple(_SIGS_BLIND)
# include/codec_tcc_blind_auto.h: blind MED-PEE with T chosen per slice (blind.py embed_auto / capacity_curve)
BLIND_TMAX = 16                   # CODEC_PEE_BLIND_TMAX
_SIGS_BLIND_AUTO = {
    "codec_pee_blind_auto_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32, C.c_int32]),
    "codec_pee_blind_plan_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP,
                                            C.c_size_t, _VP]),
    "codec_pee_blind_embed_auto": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32,
                                             _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
}
EXPORTS_BLIND_AUTO = tuple(_SIGS_BLIND_AUTO)
# include/codec_tcc_blind_keyed.h: keyed blind MED-PEE (blind.py embed_keyed / decode_keyed; aead.py, the *_n calls)
BLIND_FLAG_KEYED = 2              # CODEC_PEE_BLIND_FLAG_KEYED
BLIND_FRAME_BITS = 224            # CODEC_PEE_BLIND_FRAME_BITS
BLIND_FRAME_WORDS = 7             # CODEC_PEE_BLIND_FRAME_WORDS
_SIGS_BLIND_KEYED = {
    "codec_chacha20_rows_n": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP]),
    "codec_poly1305_tags_n": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_int32, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_aead_release_n": (C.c_int, [_VP, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "codec_pee_blind_frames": (C.c_int, [_VP, C.c_int32, C.c_uint32, _VP, _VP, _VP]),
    "codec_pee_blind_embed_keyed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32, C.c_int32,
                                              _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_blind_unframe": (C.c_int, [C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
}
EXPORTS_BLIND_KEYED = tuple(_SIGS_BLIND_KEYED)
# include/codec_tcc_blind_vol.h: blind volume payloads (blind_volume.py; pee.py embed_blind_volume / decode_blind_volume)
BLIND_FLAG_VOLUME = 4             # CODEC_PEE_BLIND_FLAG_VOLUME
BVOL_FRAME_WORDS = 6              # CODEC_PEE_BVOL_FRAME_WORDS
BVOL_FRAME_BITS = 192             # CODEC_PEE_BVOL_FRAME_BITS
BVOL_FRAME_CRC = 0x10000          # CODEC_PEE_BVOL_FRAME_CRC
BVOL_MAX_B = 65535                # CODEC_PEE_BVOL_MAX_B
BVOL_INFO_WORDS = 8               # CODEC_PEE_BVOL_INFO_WORDS
BLIND_SKIPPED = 3                 # CODEC_PEE_BLIND_SKIPPED
_SIGS_BLIND_VOL = {
    "codec_pee_blind_volume_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32, C.c_int32]),
    "codec_pee_blind_volume_plan": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, C.c_int64, C.c_int32, C.c_uint32,
                                              C.c_int32, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "codec_pee_blind_volume_embed": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP,
                                               _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_blind_volume_order": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_size_t,
                                               _VP]),
    "codec_pee_blind_volume_gather": (C.c_int, [C.POINTER(PeeParams), _VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_size_t,
                                                _VP]),
    "codec_pee_blind_volume_extract": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP,
                                                 C.c_int64, _VP, _VP, _VP, C.c_size_t, _VP]),
}
EXPORTS_BLIND_VOL = tuple(_SIGS_BLIND_VOL)
# include/codec_tcc_blind_gate.h: gated blind MED-PEE (blind.py embed_gated / capacity_gated)
BLIND_FLAG_GATED = 8              # CODEC_PEE_BLIND_FLAG_GATED
BLIND_FLAG_GATE_SHIFT = 4         # CODEC_PEE_BLIND_FLAG_GATE_SHIFT
_SIGS_BLIND_GATE = {
    "codec_pee_blind_gate_workspace_bytes": (C.c_size_t, [C.POINTER(PeeParams), C.c_int32, C.c_int32]),
    "codec_pee_blind_plan_gate": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP,
                                            _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "codec_pee_blind_embed_gate": (C.c_int, [C.POINTER(PeeParams), _VP, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
}
EXPORTS_BLIND_GATE = tuple(_SIGS_BLIND_GATE)

_lib = None
_load_error = None
# -D flags of diagnostic builds (tools/): never the product library
_DIAG_DEFINES = {"-DDECIDE_TS", "-DDECIDE_TS_SCAN_ONLY", "-DCODEC_ST_SC", "-DPEE_LB_TRACE", "-DPEE_SS_TRACE",
                 "-DCODEC_DEBUG_KNOBS", "-DRES_TRACE", "-DPEE_X_COPYONLY"}


def load(path: str = LIB_PATH):
    """Load (once) and return the library; raise RuntimeError if it is missing."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    # torch must be imported first: it ships its own libamdhip64 (soname libamdhip64.so.7).
    # Loaded first, it is the one our NEEDED entry binds to; loaded second, the process
    # would hold two HIP runtimes and device pointers from one are unknown to the other.
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise RuntimeError(f"libcodec_hip.so not found at {path}: build it with "
                           f"`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)")
    in_tree = os.path.abspath(path) == os.path.abspath(_DEFAULT_PATH)
    if in_tree:
        _check_digest(path)
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover - environment specific
        _load_error = e
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in {**_SIGS, **_SIGS_EXT, **_SIGS_CRC, **_SIGS_VOL, **_SIGS_GATE, **_SIGS_GVOL,
                              **_SIGS_TILE, **_SIGS_ROI, **_SIGS_AEAD, **_SIGS_BLIND, **_SIGS_BLIND_AUTO,
                              **_SIGS_BLIND_KEYED, **_SIGS_BLIND_VOL, **_SIGS_BLIND_GATE}.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if name == "codec_build_digest" and not in_tree:   # a diagnostic build (tools/)
                continue
            raise RuntimeError(f"{path} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    if lib.codec_abi_version() != 1:
        raise RuntimeError("libcodec_hip.so ABI mismatch")
    _lib = lib
    return lib


def _check_digest(path: str):
    """Refuse an in-tree library not built from the tree's sources: its
    embedded digest (build.library_digest, read from the file before loading it) must equal
    the digest of csrc/*, include/codec_tcc.h and the build flags.  No rebuild here: on the
    GPU box the prebuilt library is the product, and a mismatch there is an error."""
    from . import build
    # the flags the library was built with travel inside it: a build for another
    # CODEC_OFFLOAD_ARCH / CODEC_BUILD_DEFS loads without that environment, and a mismatch
    # names the sources as the cause only when they are
    flags = build.library_flags(path)
    # a diagnostic build matches its own digest but is not the product: phase
    # stamps, a scan that returns before deciding (DECIDE_TS_SCAN_ONLY), trace buffers ...
    diag = sorted({f for f in (flags or []) if f.split("=")[0] in _DIAG_DEFINES})
    if diag and os.environ.get("CODEC_ALLOW_DIAG_LIB") != "1":
        raise RuntimeError(f"{path} is a diagnostic build ({' '.join(diag)}); rebuild the product library with "
                           "`python -c 'import __graft_entry__ as g; g.build()'` (CODEC_ALLOW_DIAG_LIB=1 loads it anyway)")
    if flags is not None and flags != build.FLAGS and not diag:
        import warnings
        warnings.warn(f"{path} was built with non-default flags {' '.join(flags)}", RuntimeWarning, stacklevel=3)
    have, want = build.library_digest(path), build.source_digest(flags)
    if have != want:
        extra = "" if flags is None or flags == build.FLAGS else \
            f" (built with flags {' '.join(flags)}; this environment's are {' '.join(build.FLAGS)})"
        raise RuntimeError(f"{path} was not built from these sources (library digest {have}, sources {want}){extra}: "
                           "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")


def check(rc: int, what: str):
    if rc != 0:
        msg = load().codec_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def ptr(t) -> int | None:
    """Raw device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()
