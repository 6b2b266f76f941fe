"""Every MED-PEE decode -- PeeCodec.decode (both schemes, gated, ROI), decode_volume,
pipeline.decode_bin_pee (scheme bytes 1..4) -- over plain, checksummed, tiled and keyed embeddings,
clean and with one altered context pixel, at verify True / False / 'require': the ORDERED kernel
tags the call records (codec_profile_*) and what it raises are those of
tests/golden/decode_launch_tags.json.

The fixture was recorded on the commit before the three decode paths were folded into
codec_tcc_amd/pee_verify.py (tests/golden/make_decode_launch_tags.py says how).  It pins that the
fold changed no launch, no order and no error; it must NEVER be regenerated from the code under
test -- a difference is a finding about the code, not about the fixture."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_decode_launch_tags",
                                                  os.path.join(GOLDEN, "make_decode_launch_tags.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _generator()
with open(os.path.join(GOLDEN, "decode_launch_tags.json")) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_every_case():
    assert sorted(WANT) == sorted(f"{k}/{e}" for k in M.KINDS for e in M.EMBEDDINGS)
    cases = sorted(f"{s}/{v}" for s in M.STATES for v in M.VERIFY)
    assert all(sorted(WANT[k]) == cases for k in WANT)
    # 'require' with nothing to verify made no launch; every keyed decode ran the cipher
    for name, recs in WANT.items():
        for state in M.STATES:
            if name.endswith("/plain"):
                assert recs[f"{state}/require"]["result"] == "IntegrityError" and recs[f"{state}/require"]["tags"] == []
            if "keyed" in name:
                assert all(any(t.startswith(("k_chacha", "k_poly", "k_aead")) for t in recs[f"{state}/{v}"]["tags"])
                           for v in M.VERIFY)


@pytest.mark.parametrize("embedding", M.EMBEDDINGS)
@pytest.mark.parametrize("kind", M.KINDS)
def test_launches_and_errors_are_the_recorded_ones(kind, embedding):
    got, want = M.run(kind, embedding), WANT[f"{kind}/{embedding}"]
    for case in want:
        print(kind, embedding, case, got[case])
        assert got[case] == want[case], (kind, embedding, case)


@pytest.mark.parametrize("kind", ["s1", "s2", "volume", "file1"])
def test_the_error_carries_the_rows_of_the_one_read_back(kind):
    """IntegrityError.rows: None before any read-back; else what the read-back brought -- the real
    rows for a CRC failure, the released zeros for the slices of a keyed failure."""
    import tempfile
    from codec_tcc_amd import IntegrityError
    with tempfile.TemporaryDirectory() as tmp:
        dec, _bits, _covers = M._decoders(kind, "plain", tmp)
        with pytest.raises(IntegrityError) as e:
            dec["clean"]("require")
        assert e.value.rows is None
        dec, _bits, _covers = M._decoders(kind, "crc", tmp)
        with pytest.raises(IntegrityError) as e:
            dec["altered"](True)
        assert not e.value.keyed and isinstance(e.value.rows, np.ndarray) and e.value.rows.any()
        dec, _bits, _covers = M._decoders(kind, "keyed", tmp)
        with pytest.raises(IntegrityError) as e:
            dec["altered"](True)
        rows = e.value.rows
        if kind == "volume":
            assert rows.ndim == 1 and (not rows.any()) == e.value.stream
        else:
            B = 1 if kind == "file1" else 3
            assert rows.shape[0] == B and e.value.slices and all(not rows[b].any() for b in e.value.slices)
            assert all(rows[b].any() for b in range(B) if b not in e.value.slices)


def test_a_file_decode_asks_whether_the_look_back_gave_up(monkeypatch):
    """decode_bin_pee reads the flag after its payload read-back, as decode() does: with the flag
    standing (patched -- no timeout is provoked) it resets the workspace and raises decode()'s error."""
    import tempfile
    from codec_tcc_amd.pee import PeeCodec
    resets = []
    with tempfile.TemporaryDirectory() as tmp:
        dec, bits, _covers = M._decoders("file1", "crc", tmp)
        got, _cover = dec["clean"](True)
        assert np.array_equal(got, bits)
        monkeypatch.setattr(PeeCodec, "lookback_failed", lambda self, payload_words=1: True)
        reset = PeeCodec.reset
        monkeypatch.setattr(PeeCodec, "reset", lambda self: (resets.append(1), reset(self))[1])
        with pytest.raises(RuntimeError, match="look-back timed out; the recovered payload is invalid"):
            dec["clean"](True)
    assert len(resets) >= 2   # the codec's construction, then the failed decode
