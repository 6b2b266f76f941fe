"""codec_tcc_amd -- MI355X-native (gfx950) implementation of wesleyfn/codec-tcc's
embed/extract pixel path: the reference's LSB bit-plane scheme (bit-exact with
src/codec.py) and the MED-PEE scheme the north star names.  See DESIGN.md and
INTEGRATION.md.

Batched API (torch tensors in HBM):   encode(covers, payloads, method="lsb"|"pee", ...),
                                      decode(enc), decode_ref_compat, Codec, PeeCodec
One payload across a slice stack:     encode_volume(covers, payload), decode_volume(vol) (MED-PEE scheme 1)
Stegos that decode on their own:      encode_blind(covers, payloads), decode_blind(stego) (MED-PEE scheme 1)
... gated, (T, gate) per slice:       encode_blind_gated(covers, payloads) (decode_blind reads them)
One payload across blind stegos:      encode_blind_volume(covers, payload), decode_blind_volume(stego) (any slice order)
... under a 32-byte key:              encode_blind_keyed(covers, payloads, key), decode_blind_keyed(stego, key)
Reference drop-ins (numpy in/out):    codec_tcc_amd.api (same names as src/codec.py)
"""
from .codec import Codec, Encoded, Payloads, decode, decode_ref_compat, encode, make_payloads, meta_dict, meta_records
from .framing import distribute_message_segments, message_to_bits
from .checksum import IntegrityError, crc32_slices
from .pee import (PeeCodec, PeeEncoded, PeeVolume, decode_blind, decode_blind_keyed, decode_blind_volume, decode_volume,
                  encode_blind, encode_blind_auto, encode_blind_gated, encode_blind_keyed, encode_blind_volume, encode_volume)

__all__ = [
    "encode_blind_volume", "decode_blind_volume", "encode_blind", "encode_blind_auto", "encode_blind_gated", "decode_blind", "encode_blind_keyed", "decode_blind_keyed",
    "Codec", "Encoded", "Payloads", "encode", "decode", "decode_ref_compat", "make_payloads",
    "meta_records", "meta_dict", "message_to_bits", "distribute_message_segments", "PeeCodec", "PeeEncoded",
    "crc32_slices", "IntegrityError", "PeeVolume", "encode_volume", "decode_volume",
]
