"""BASELINE.json configs through the default launch shapes the benchmark uses:

* C3 -- 256 x 512^2 slices on one GPU;
* the headline shape -- 256 x 2048^2 (k_scan_rows, k_decide_embed, k_restore_gs for the
  reference's LSB path; k_pee_embed1 / k_pee_extract1 lane-order single pass for MED-PEE).

Each batch is compared with the oracles on a stride sample of slices (s, start offset,
stego; PEE stego, location map, end), the reference's own 2048^2 known answers are placed
as slices inside the headline batch, and every slice is checked by exact round trip
(restored cover and recovered payload bits).  Covers are generated on the device
(synth.ct12_torch); the sampled slices are copied back for the oracle."""
import hashlib
import os
import sys

import numpy as np
import pytest

import golden_io
from codec_tcc_amd import Codec, framing, make_payloads, synth
from oracle import pee_cpu as P
from oracle import ref_cpu as R

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import payload_equal  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _batch(B, H, W, seed):
    return synth.ct12_torch(B, H, W, "cuda", seed=seed).view(torch.uint16)


def _lsb_batch_check(covers, msgs, sample, kats=()):
    B, H, W = covers.shape
    codec = Codec(B, H, W, dtype="uint16", beta=0.4, block=16)
    pl = make_payloads(msgs, covers.device)
    enc = codec.encode(covers, pl)
    recs = enc.records()
    for i in sample:
        cov = covers[i].cpu().numpy()
        exp = R.encode_slice(cov, R.message_to_bits(msgs[i]), beta=0.4, sb=16)
        assert recs[i].s == exp["s"] and recs[i].start_offset == exp["start_offset"], i
        assert [recs[i].perm[j] for j in range(exp["s"])] == list(exp["segment_indices"])
        np.testing.assert_array_equal(enc.stego[i].cpu().numpy(), exp["stego"])
    for i, kat in kats:
        m = recs[i]
        assert m.s == kat["s"] and [m.perm[j] for j in range(m.s)] == kat["perm"]
        assert [m.sizes[p] for p in range(m.s)] == kat["sizes"]
        assert hashlib.sha256(enc.stego[i].cpu().numpy().tobytes()).hexdigest() == kat["stego_sha256"]
    words, cover = codec.decode(enc.stego, enc.maps, enc.meta, payload_words=pl.payload_words,
                                map_words=pl.map_words)
    assert torch.equal(cover.view(torch.int16), covers.view(torch.int16))
    assert all(r.total_used == n and r.status == 0 for r, n in zip(recs, pl.lengths))
    assert payload_equal(words, pl.words, pl.lengths)


def _pee_batch_check(covers, sample, T=2, chars=1024):
    from codec_tcc_amd.pee import PeeCodec, lm_bits
    B, H, W = covers.shape
    codec = PeeCodec(B, H, W, dtype="uint16", T=T)
    payloads = [framing.to_bits(synth.payload(chars, 300 + i)) for i in range(B)]
    packed = codec.pack_payloads(payloads)
    enc = codec.embed(covers, None, packed=packed)
    recs = enc.records()
    t_dev = codec.t_slices.cpu().numpy() if T == "auto" else None
    for i in sample:
        cov = covers[i].cpu().numpy()
        Ti = P.select_T(cov, len(payloads[i]), codec.tmax) if T == "auto" else T
        assert recs[i].T == Ti
        if t_dev is not None:
            assert t_dev[i] == Ti, i
        st, side = P.pee_embed(cov, payloads[i], Ti)
        assert recs[i].status == 0 and recs[i].end == side["end"], i
        np.testing.assert_array_equal(enc.stego[i].cpu().numpy(), st)
        np.testing.assert_array_equal(lm_bits(enc, i), side["lm"])
    words, cover = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    assert torch.equal(cover.view(torch.int16), covers.view(torch.int16))
    assert all(r.status == 0 for r in recs) and not codec.lookback_failed(enc.payload_words)
    assert payload_equal(words, packed[0], [len(p) for p in payloads])
    assert codec.repaired(enc.payload_words) == 0
    # in place on the same batch: the stego and the payload equal the out-of-place ones
    work = covers.clone()
    enc2 = codec.embed(work, None, stego=work, packed=packed)
    assert torch.equal(work.view(torch.int16), enc.stego.view(torch.int16))
    w2, _ = codec.extract(work, enc2.meta, enc2.lm, payload_words=enc2.payload_words, cover=work)
    assert torch.equal(work.view(torch.int16), covers.view(torch.int16))
    assert payload_equal(w2, packed[0], [len(p) for p in payloads])


def test_c3_lsb_256x512():
    B, H, W = 256, 512, 512
    covers = _batch(B, H, W, seed=1000)
    msgs = [synth.payload(1024, 5000 + i) for i in range(B)]
    _lsb_batch_check(covers, msgs, sample=range(0, B, 16))


@pytest.mark.parametrize("ss", ["auto", "res0", "0", "unfused"])
def test_c3_pee_256x512(ss, monkeypatch):
    """1 KB per 512^2 ct12 slice needs T ~ 4-5 (T = 2 holds ~4.4 kbit): capacity control.
    "auto": the default launch, the resident embed (k_pee_embed_res: the slice read once and
    kept on the CU while T is chosen); "res0": capacity fused into the two-phase slice-serial
    embed (CODEC_PEE_RES=0); "unfused": capacity pass + slice-serial embed as two launches;
    "0": capacity pass + look-back embed."""
    if ss == "unfused":
        monkeypatch.setenv("CODEC_PEE_AUTO_FUSED", "0")
    elif ss == "res0":
        monkeypatch.setenv("CODEC_PEE_RES", "0")
    elif ss != "auto":
        monkeypatch.setenv("CODEC_PEE_SS", ss)
    _pee_batch_check(_batch(256, 512, 512, seed=2000), sample=range(3, 256, 16), T="auto")


def test_headline_lsb_256x2048_with_kats():
    """The bench's launch shape, the reference's 2048^2 known answers (beta 0.4) as slices
    37 and 200 of the batch, oracle comparison on 4 more slices."""
    B, H, W = 256, 2048, 2048
    covers = _batch(B, H, W, seed=0)
    msgs = [synth.payload(1024, 7 + i) for i in range(B)]
    kats = []
    for pos, kat in zip((37, 200), [k for k in golden_io.kat2048() if k["beta"] == 0.4]):
        img = synth.GENERATORS[kat["kind"]](kat["h"], kat["w"], kat["seed"])
        assert hashlib.sha256(img.tobytes()).hexdigest() == kat["cover_sha256"]
        covers[pos].copy_(torch.from_numpy(img).view(torch.uint16))
        msgs[pos] = synth.payload(kat["payload_chars"], kat["payload_seed"])
        kats.append((pos, kat))
    assert len(kats) == 2
    _lsb_batch_check(covers, msgs, sample=(0, 85, 170, 255), kats=kats)


@pytest.mark.parametrize("ss", ["auto", "1"])
def test_headline_pee_256x2048(ss, monkeypatch):
    """Default dispatch at this shape (codec_pee.hip pee_use_slice_serial): out of place the
    look-back single pass (k_pee_embed1 / k_pee_extract1, chunk-parallel), in place the
    slice-serial pass (k_pee_embed_ss / k_pee_extract_ss).  "1" forces the slice-serial
    kernels out of place too, so the out-of-place k_pee_embed_ss runs once at 2048^2."""
    if ss != "auto":
        monkeypatch.setenv("CODEC_PEE_SS", ss)
    _pee_batch_check(_batch(256, 2048, 2048, seed=11), sample=(0, 101, 255))


def test_profile_pass_is_bounded_for_any_step_count():
    """bench._profile with a step count whose launches would not fit the library's event
    window (64 x steps > 2^20, e.g. the C2 leg's 10 x --steps of a long run): the pass runs
    PROFILE_MAX_STEPS calls and returns the kernel's mean time instead of failing."""
    import bench
    from codec_tcc_amd import _lib
    from codec_tcc_amd import quality as Q
    a = _batch(2, 64, 64, seed=5)
    b = _batch(2, 64, 64, seed=6)
    calls = []

    def fn():
        calls.append(1)
        Q.moments(a, b)

    kern = bench._profile(_lib.load(), _lib, fn, 10 * 2000)
    assert len(calls) == bench.PROFILE_MAX_STEPS and 64 * bench.PROFILE_MAX_STEPS <= 1 << 20
    assert kern.get("k_quality", 0) > 0, kern
    few = []
    bench._profile(_lib.load(), _lib, lambda: (few.append(1), Q.moments(a, b)), 3)
    assert len(few) == 3


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """`bench.py` without --full: the line holds the headline figure only (--steps timed
    steps, ms_per_step and value consistent with each other), none of the side legs, checks
    or baselines; --dump-outputs writes the last step's arrays as float32 / float64 .npy,
    and they equal an embed + extract made here from the same seeds (so the inputs of a run
    are a function of its arguments alone)."""
    import json
    import subprocess

    import bench
    from codec_tcc_amd import distributed as D
    from codec_tcc_amd.pee import PeeCodec
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, H, chars = 3, 256, 64
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", str(B), "--size", str(H), "--payload-chars", str(chars), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "Mpixels/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u16" and out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    # value and ms_per_step are rounded to 1 and 4 decimals: half a unit of each, relative
    px = B * H * H / 1e6
    assert out["value"] == pytest.approx(px / (out["ms_per_step"] / 1e3),
                                         rel=0.5e-4 / out["ms_per_step"] + 0.05 / out["value"] + 1e-9)
    for moved in ("pee", "inplace", "lsb", "quality", "c3", "c2", "cpu_baseline", "kernels_ms", "roofline",
                  "roundtrip_ok"):
        assert moved not in out, moved
    # the same step made here from the same seeds
    dev = torch.device("cuda", torch.cuda.current_device())
    covers = bench.make_covers(torch, "ct12", B, H, H, dev, seed=0)
    codec = PeeCodec(B, H, H, dtype="uint16", T=2, device=dev)
    enc = codec.embed(covers, [synth.payload(chars, 99 + i) for i in range(B)])
    words, cover = codec.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words)
    want = {"stego": enc.stego.cpu().numpy(), "cover": cover.cpu().numpy(),
            "side_info": enc.meta.view(torch.int32).cpu().numpy(),
            "payload": words.cpu().numpy().view(np.uint16),
            "location_map": D.map_prefix(enc.meta, enc.lm, codec.lm_words).cpu().numpy().view(np.uint16)}
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in want)
    total = 0
    for name, w in want.items():
        got = np.load(out_dir / (name + ".npy"))
        total += got.nbytes
        assert got.dtype == (np.float64 if name == "side_info" else np.float32), name
        np.testing.assert_array_equal(got, w.astype(got.dtype), err_msg=name)
    assert total <= 64e6
    np.testing.assert_array_equal(want["cover"], covers.cpu().numpy())
