"""The codecs' buffer contract (codec_tcc_amd.pee.check_buffers), on CPU tensors.

The library sees a pointer and (B, H, W, bytes) and assumes a dense block on the codec's
device, so the Python layer has to refuse everything else before a launch.  The validator looks
at shapes, strides, devices and pointers only; it runs here on CPU tensors with the expected
device passed in.  One accepted and one rejected case per rule; every rejection asserts the
exception type and that the message names the offending argument.  The same rules on a real
codec, with the library stubbed out, are in tests/test_pee_placement.py."""
import pytest

torch = pytest.importorskip("torch")

from codec_tcc_amd import _lib  # noqa: E402
from codec_tcc_amd.pee import check_buffers  # noqa: E402

B, H, W = 3, 8, 64
LMW = ((H // 2) * (W // 2) + 63) // 64   # 2 words, as PeeCodec.lm_words
CPU = torch.device("cpu")


def _pix(dtype=torch.uint16, shape=(B, H, W)):
    return torch.zeros(shape, dtype=dtype)


def _check(device=CPU, nbytes=2, scheme=1, **kw):
    check_buffers(device, B, H, W, nbytes, lm_words=LMW, scheme=scheme, **kw)


def _sides(scheme=1):
    lead = (4, B) if scheme == 2 else (B,)
    return dict(lm=torch.zeros(lead + (LMW,), dtype=torch.int64),
                meta=torch.zeros(lead + (_lib.PEE_META_BYTES,), dtype=torch.uint8))


# ------------------------------------------------------------------------------ pixel tensors
def test_dense_and_offset_views_are_accepted():
    _check(covers=_pix())
    _check(covers=_pix(torch.int16))          # the 16-bit pixels' other dtype
    _check(nbytes=1, covers=_pix(torch.uint8))
    big = _pix(shape=(B + 4, H, W))
    row = big[2:2 + B]                        # a contiguous row-slice of a larger stack
    assert row.is_contiguous() and row.storage_offset() == 2 * H * W
    _check(covers=row)
    flat = torch.zeros(B * H * W + 7, dtype=torch.uint16)
    view = flat[3:3 + B * H * W].view(B, H, W)   # any storage offset, here 6 bytes
    assert view.data_ptr() % 16 != flat.data_ptr() % 16
    _check(covers=view, stego=_pix())


@pytest.mark.parametrize("name", ["covers", "stego", "cover"])
@pytest.mark.parametrize("view", ["strided", "transposed", "crop"])
def test_views_that_are_not_dense_are_rejected(name, view):
    t = {"strided": lambda: _pix(shape=(B, H, 2 * W))[:, :, ::2],
         "transposed": lambda: _pix(shape=(B, W, H)).transpose(1, 2),
         "crop": lambda: _pix(shape=(B, H + 2, W + 8))[:, :H, :W]}[view]()
    assert tuple(t.shape) == (B, H, W) and not t.is_contiguous()
    with pytest.raises(ValueError, match=rf"^{name} must be contiguous"):
        _check(**{name: t})


def test_wrong_dtype_rank_and_shape_are_rejected():
    with pytest.raises(ValueError, match=r"^covers must hold 2-byte pixels"):
        _check(covers=_pix(torch.uint8))
    with pytest.raises(ValueError, match=r"^covers must hold 2-byte pixels"):
        _check(covers=_pix(torch.float16))    # two bytes, but no pixel
    with pytest.raises(ValueError, match=r"^stego must hold 1-byte pixels"):
        _check(nbytes=1, covers=_pix(torch.uint8), stego=_pix(torch.int8))
    with pytest.raises(ValueError, match=r"^covers must have the codec's shape"):
        _check(covers=_pix(shape=(B * H, W)))               # rank 2
    with pytest.raises(ValueError, match=r"^covers must have the codec's shape"):
        _check(covers=_pix(shape=(1, B, H, W)))             # rank 4
    with pytest.raises(ValueError, match=r"^cover must have the codec's shape"):
        _check(stego=_pix(), cover=_pix(shape=(B, H, W + 1)))


def test_wrong_device_names_both_devices():
    cuda0 = torch.device("cuda", 0)           # comparing devices needs no GPU
    with pytest.raises(TypeError, match=r"^covers is on cpu, the codec is on cuda:0"):
        _check(device=cuda0, covers=_pix())
    with pytest.raises(TypeError, match=r"^lm is on cpu, the codec is on cuda:0"):
        check_buffers(cuda0, B, H, W, 2, lm_words=LMW, lm=_sides()["lm"])
    with pytest.raises(TypeError, match=r"^covers must be a torch tensor"):
        _check(covers=_pix().numpy())
    # a device given without an index names every card of its type
    _check(device=torch.device("cpu"), covers=_pix())


# ------------------------------------------------------------------------------ aliasing
def test_in_place_and_disjoint_pairs_are_accepted():
    a = _pix()
    _check(covers=a, stego=a)                              # identical pointers: in place
    _check(covers=a, stego=a.view(B, H, W))
    _check(stego=a, cover=a)
    _check(covers=a, stego=_pix())                         # disjoint allocations
    two = _pix(shape=(2 * B, H, W))
    _check(covers=two[:B], stego=two[B:])                  # adjacent, not overlapping
    _check(stego=two[B:], cover=two[:B])


@pytest.mark.parametrize("src,dst", [("covers", "stego"), ("stego", "cover")])
def test_overlap_that_is_not_in_place_is_rejected(src, dst):
    flat = torch.zeros(2 * B * H * W, dtype=torch.uint16)
    n = B * H * W
    a, ahead, behind = (flat[k:k + n].view(B, H, W) for k in (W, 2 * W, 0))   # one row apart
    with pytest.raises(ValueError, match=rf"^{dst} overlaps {src}"):
        _check(**{src: a, dst: ahead})
    with pytest.raises(ValueError, match=rf"^{dst} overlaps {src}"):
        _check(**{src: a, dst: behind})
    with pytest.raises(ValueError, match=rf"^{dst} overlaps {src}"):
        _check(**{src: flat[:n].view(B, H, W), dst: flat[n - 1:2 * n - 1].view(B, H, W)})   # by one pixel


# ------------------------------------------------------------------------------ side buffers
@pytest.mark.parametrize("scheme", [1, 2])
def test_side_buffers(scheme):
    s = _sides(scheme)
    pw = 2
    pay = torch.zeros((B, pw), dtype=torch.int64)
    _check(scheme=scheme, covers=_pix(), payload=pay, payload_words=pw, **s)
    _check(scheme=scheme, payload=torch.zeros((B + 1, pw), dtype=torch.int64)[:B], payload_words=pw)
    bad = {
        "lm": [s["lm"][..., :-1].contiguous(),                                                # a word short
               torch.zeros(s["lm"].shape[:-1] + (LMW + 1,), dtype=torch.int64)[..., :LMW],    # right shape, row pitch off
               s["lm"].to(torch.int32), s["lm"][..., 0]],
        "meta": [s["meta"][..., :-1].contiguous(), s["meta"].to(torch.int16),
                 torch.zeros(s["meta"].shape[:-1] + (2 * _lib.PEE_META_BYTES,), dtype=torch.uint8)[..., ::2]],
        "payload": [torch.zeros((B - 1, pw), dtype=torch.int64),     # a row short
                    torch.zeros((B, pw - 1), dtype=torch.int64),     # a word short
                    torch.zeros((B, pw), dtype=torch.int32), torch.zeros(B * pw, dtype=torch.int64)],
    }
    for name, tensors in bad.items():
        for t in tensors:
            args = dict(s, payload=pay)
            args[name] = t
            with pytest.raises(ValueError, match=rf"^{name} must be"):
                _check(scheme=scheme, payload_words=pw, **args)
    # rows further apart than payload_words: the library's row pitch is payload_words
    wide = torch.zeros((B, pw + 1), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"^payload must be rows .* apart"):
        _check(scheme=scheme, payload=wide, payload_words=pw)
    with pytest.raises(ValueError, match=r"^payload must be rows .* apart"):
        _check(scheme=scheme, payload=wide[:, :pw], payload_words=pw)
    if scheme == 1:   # scheme 2's shapes are another scheme's
        with pytest.raises(ValueError, match=r"^lm must be"):
            _check(scheme=1, **_sides(2))
    else:
        with pytest.raises(ValueError, match=r"^lm must be"):
            _check(scheme=2, **_sides(1))


def test_packed_payloads():
    words = torch.zeros((B, 3), dtype=torch.int64)
    lens_t = torch.zeros(B, dtype=torch.int32)
    _check(covers=_pix(), packed=(words, [0] * B, lens_t))
    with pytest.raises(ValueError, match=r"^packed\[0\] must be"):
        _check(packed=(words[:B - 1], [0] * B, lens_t))
    with pytest.raises(ValueError, match=r"^packed\[0\] must be"):
        _check(packed=(torch.zeros((B, 6), dtype=torch.int64)[:, ::2], [0] * B, lens_t))
    with pytest.raises(ValueError, match=r"^packed\[0\] must be"):
        _check(packed=(torch.zeros((B, 0), dtype=torch.int64), [0] * B, lens_t))
    with pytest.raises(ValueError, match=r"^packed\[1\] holds 2 lengths for 3 slices"):
        _check(packed=(words, [0] * (B - 1), lens_t))
    with pytest.raises(ValueError, match=r"^packed\[2\] must be"):
        _check(packed=(words, [0] * B, lens_t.to(torch.int64)))
    with pytest.raises(ValueError, match=r"^packed\[2\] must be"):
        _check(packed=(words, [0] * B, torch.zeros(B - 1, dtype=torch.int32)))
    with pytest.raises(TypeError, match=r"^packed\[0\] is on cpu, the codec is on cuda:0"):
        check_buffers(torch.device("cuda", 0), B, H, W, 2, lm_words=LMW, packed=(words, [0] * B, lens_t))


def test_the_validator_touches_no_data():
    """`meta` tensors have no storage: any read-back, copy or launch on them raises."""
    m = torch.device("meta")
    check_buffers(m, B, H, W, 2, lm_words=LMW, covers=torch.empty((B, H, W), dtype=torch.uint16, device=m),
                  lm=torch.empty((B, LMW), dtype=torch.int64, device=m),
                  meta=torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=m),
                  payload=torch.empty((B, 2), dtype=torch.int64, device=m), payload_words=2)
