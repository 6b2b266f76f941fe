"""The one path behind every MED-PEE extract (codec_tcc_amd/pee_verify.py) on the host: the shared
precondition and key checks keep each caller's texts, and pipeline.decode_bin_pee asks the codec
whether the extract's look-back gave up -- shown with a stub codec on CPU tensors.  No GPU."""
import struct

import numpy as np
import pytest

from codec_tcc_amd import IntegrityError, container, pee, pee_checks, pee_verify, pipeline


def test_require_texts_are_the_callers():
    pee_verify.check_require("present", False, False, False)
    pee_verify.check_require("require", True, False, False)     # a tag stands in for the checksums
    pee_verify.check_require("require", False, True, True)
    with pytest.raises(IntegrityError) as e:
        pee_verify.check_require("require", False, True, False)
    assert str(e.value) == "MED-PEE decode: verify='require' and the embedding carries no payload checksum"
    assert e.value.rows is None
    with pytest.raises(IntegrityError) as e:
        pee_verify.check_require("require", False, False, False, carrier="the volume")
    assert str(e.value) == "MED-PEE decode: verify='require' and the volume carries no cover / payload checksum"
    with pytest.raises(IntegrityError) as e:
        pee_verify.check_require("require", False, False, False, "MED-PEE file", "the header", named=False)
    assert str(e.value) == "MED-PEE file: verify='require' and the header carries no checksums"


def test_key_texts_are_the_callers():
    assert pee_verify.check_key(False, None) is None
    assert pee_verify.check_key(True, bytearray(32)) == bytes(32)
    with pytest.raises(ValueError, match=r"^the embedding is keyed \(enc\.tag\): decode it with key=$"):
        pee_verify.check_key(True, None)
    with pytest.raises(ValueError, match=r"^key= given for an embedding that is not keyed \(no enc\.tag\)$"):
        pee_verify.check_key(False, bytes(32))
    file = ("file", "its header carries the A1 extension", "A1 extension")
    with pytest.raises(ValueError, match=r"^the file is keyed \(its header carries the A1 extension\): decode it with key=$"):
        pee_verify.check_key(True, None, *file)
    with pytest.raises(ValueError, match=r"^key= given for a file that is not keyed \(no A1 extension\)$"):
        pee_verify.check_key(False, bytes(32), *file)
    with pytest.raises(ValueError, match="32 bytes"):
        pee_verify.check_key(True, b"short")


def test_pee_re_exports_the_host_checks():
    for name in ("lattice_geometry", "make_record", "check_records", "check_volume_args", "check_gate_args",
                 "check_roi_args", "check_gvol_args", "check_buffers", "_check_multi_args", "_bad_device", "_bad_pixels",
                 "_bad_side", "_bad_overlap", "_dense", "_on_device", "_pix_dtypes"):
        assert getattr(pee, name) is getattr(pee_checks, name), name


class _StubCodec:
    """What after_extract and decode_bin_pee ask of a codec, on CPU tensors."""
    made, fail = [], True

    def __init__(self, B, H, W, **_kw):
        import torch
        self.B, self.H, self.W, self.device = B, H, W, torch.device("cpu")
        self.resets, self.asked = 0, []
        _StubCodec.made.append(self)

    def extract(self, stego, meta, lm, *, payload_words, **_kw):
        import torch
        return torch.full((self.B, payload_words), 5, dtype=torch.int64), stego.clone()

    def lookback_failed(self, payload_words=1):
        self.asked.append(payload_words)
        return _StubCodec.fail

    def reset(self):
        self.resets += 1


def test_decode_bin_pee_consults_the_look_back_flag(tmp_path, monkeypatch):
    import torch
    blob = container.lm_blob(np.zeros(4, dtype=bool))                     # end = 3: four map bits
    hdr = container.create_pee_header("raw", 2, 6, 4, 2, 3, 3, 4095, 0, len(blob))
    path = tmp_path / "f.bin"
    path.write_bytes(container.MAGIC + struct.pack(">I", len(hdr)) + hdr + blob + bytes(48))
    monkeypatch.setattr(pipeline, "_require_gpu", lambda: None)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(pee, "PeeCodec", _StubCodec)
    _StubCodec.made.clear()
    monkeypatch.setattr(_StubCodec, "fail", True)
    with pytest.raises(RuntimeError) as e:
        pipeline.decode_bin_pee(str(path), verify=False)
    assert str(e.value) == pee_verify.LOOKBACK_TIMEOUT and "in-place cursor look-back timed out" in str(e.value)
    (codec,) = _StubCodec.made
    assert codec.asked == [1] and codec.resets == 1
    _StubCodec.fail = False                                                # the flag clear: the rows come back
    bits, cover = pipeline.decode_bin_pee(str(path), verify=False)
    assert bits.tolist() == [1, 0, 1] and cover.shape == (4, 6) and _StubCodec.made[1].resets == 0
