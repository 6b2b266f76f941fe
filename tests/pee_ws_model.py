"""Model of the state a MED-PEE workspace carries from call to call.  TEST INFRASTRUCTURE ONLY:
plain Python, no torch, no GPU, and no code shared with codec_tcc_amd -- a restatement of the
rules of include/codec_tcc.h (codec_pee_workspace_bytes) and of the host side of
codec_tcc_amd/csrc/codec_pee.hip (pee_ws, pee_ws_enter, pee_lookback_setup, pee_ws_epoch), which
tests/test_pee_call_sequences.py checks against what the library leaves in the workspace.

Layout of one shape (B, H, W, bytes), byte offsets:
  cnt    0                                       tile counts of the two-pass routes, B * ntiles uint32
  off    align256(4 B ntiles)                    tile offsets, as many
  st     align256(off + 4 B ntiles)              status words: 2 buffers of B * nchunks uint64
  ctl    st + 16 B nchunks                       32 uint32, then a line of 32 per slice
                                                 (word 1 of ctl: the extract's look-back flag;
                                                 word 1 / 4 of a line: finished flag 0 / 1)
  diag   align16(ctl + 4 (32 + 32 B))            4 cumulative uint32 counters
  hist   align256(diag + 16)                     capacity bins B * 64 uint32, then B arrival counters
  sink   align256(hist + 4 B 65)                 slice-serial sink, 1024 B per slice
  total  align256(sink + 1024 B)
with ntiles = ceil((H/2)(W/2) / 1024) and nchunks = ceil((H/2)(W/8) / 1024), both at least 1.
The table of codec_pee_gate_capacity lies behind it: B * (17 * 16 + 1) uint32 at align256(total).

Registry, per workspace pointer: the shape of the last call that entered it, the epoch of its
self-cleaning calls (mod 126), whether its state region is known clean, where its diagnostic
counters lie, and the shape a call was captured into a graph with.
  enter      every workspace-taking call but codec_pee_multi_embed_auto (which keeps nothing in
             the workspace): another shape than the recorded one zeroes the workspace first and
             restarts the epochs at 0 -- the diagnostic counters too when the new layout puts
             them elsewhere; a call made under stream capture records its shape as captured
  self-cleaning   the scheme-1 look-back embed / extract when ungated, out of place, B <= 7,
             W % 8 == 0 with vector-aligned images, at least one item, not under capture, no
             other shape captured on the workspace, (H/2)(W/2) <= 2^24 - 2.  It draws the
             next epoch e: buffer e & 1, tag e % 63 + 1, and clears the other buffer's words
             and finished flags.  Every other look-back call zeroes both buffers and the
             control words first and uses buffer 1 with tag 0 (flag value 1); the two-pass
             routes (unaligned views) touch cnt / off only.
  reset      zeroes everything, records the shape, epoch 0.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

TILE = 1024          # candidates per tile
CHUNK = 1024         # 8-pixel row-pair items per look-back chunk
TMAX_MAX = 64        # capacity bins per slice
SINK_PER_SLICE = 1024
EPOCHS = 126         # the epoch counter's period: parity (2) x tag (63)
TAGS = 63
TAG_SHIFT, TAG_MASK = 56, 63
FLAT_MAXB = 7
SC_MAX_NC = (1 << 24) - 2
LINE_FIN = (1, 4)    # word of a slice's control line holding finished flag 0 / 1
GATE_BINS = 17 * 16  # per slice: (tmax_max + 1) rows of 16 classes

Shape = Tuple[int, int, int, int]   # B, H, W, bytes


def align_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


@dataclass(frozen=True)
class Layout:
    cnt: int
    off: int
    st: int
    ctl: int
    diag: int
    hist: int
    sink: int
    total: int
    ntiles: int
    nchunks: int
    B: int

    # ---- words a witness reads (byte offsets)
    def status_word(self, buf: int, b: int, c: int) -> int:
        return self.st + 8 * (buf * self.B * self.nchunks + b * self.nchunks + c)

    def fin_flag(self, buf: int, b: int) -> int:
        return self.ctl + 4 * (32 + 32 * b + LINE_FIN[buf])

    @property
    def extract_flag(self) -> int:
        return self.ctl + 4

    @property
    def arrivals(self) -> int:
        return self.hist + 4 * self.B * TMAX_MAX

    @property
    def hist_end(self) -> int:
        return self.hist + 4 * self.B * (TMAX_MAX + 1)

    @property
    def ctl_end(self) -> int:
        return self.ctl + 4 * (32 + 32 * self.B)


def layout(shape: Shape) -> Layout:
    B, H, W, _bytes = shape
    nc = (H // 2) * (W // 2)
    ntiles = max(1, (nc + TILE - 1) // TILE)
    items = (H // 2) * (W // 8)
    nchunks = max(1, (items + CHUNK - 1) // CHUNK)
    off = align_up(B * ntiles * 4, 256)
    st = align_up(off + B * ntiles * 4, 256)
    ctl = st + 2 * B * nchunks * 8
    diag = align_up(ctl + (32 + 32 * B) * 4, 16)
    hist = align_up(diag + 16, 256)
    sink = align_up(hist + B * (TMAX_MAX + 1) * 4, 256)
    total = align_up(sink + SINK_PER_SLICE * B, 256)
    return Layout(0, off, st, ctl, diag, hist, sink, total, ntiles, nchunks, B)


def gate_bins(shape: Shape) -> Tuple[int, int]:
    """[lo, hi): the bytes codec_pee_gate_capacity's bins and arrival counters take."""
    lo = align_up(layout(shape).total, 256)
    return lo, lo + 4 * shape[0] * (GATE_BINS + 1)


def gate_total(shape: Shape) -> int:
    lo, hi = gate_bins(shape)
    return lo + align_up(hi - lo, 256)


def tag_of(epoch: int) -> int:
    return epoch % TAGS + 1


def word_tag(word: int) -> int:
    return (word >> TAG_SHIFT) & TAG_MASK


# ------------------------------------------------------------------ the calls
# kind -> (enters the registry, runs the scheme-1 look-back kernel: "E" / "X" / None, gated)
KINDS: Dict[str, Tuple[bool, Optional[str], bool]] = {
    "embed": (True, "E", False),            # codec_pee_embed / _embed_ts
    "extract": (True, "X", False),          # codec_pee_extract
    "capacity": (True, None, False),        # codec_pee_capacity
    "multi_embed": (True, "E", False),      # codec_pee_multi_embed: pass 0 is scheme 1's embed
    "multi_extract": (True, None, False),   # codec_pee_multi_extract: tile passes only
    "multi_embed_auto": (False, None, False),
    "gate_capacity": (True, None, True),
    "gate_embed": (True, "E", True),
    "gate_extract": (True, "X", True),
}
# codec_pee_embed_auto is "capacity" then "embed" (small batches: not fused)


@dataclass
class Step:
    """What the model says of one call."""
    kind: str
    shape: Shape
    kernel: Optional[str]      # "E" / "X": the look-back kernel ran
    sc: bool                   # self-cleaning
    epoch: Optional[int]       # of a self-cleaning call
    par: Optional[int]         # status-word buffer the look-back used (zeroing calls: 1)
    tag: Optional[int]         # 1..63 self-cleaning, 0 zeroing
    rezero: bool               # the call zeroed the workspace first (shape change)
    moved_diag: bool           # ... the diagnostic counters too
    fresh: bool                # first self-cleaning call on a region not known clean


@dataclass
class Entry:
    shape: Shape
    epoch: int = 0
    sc_clean: bool = False
    diag: int = 0
    captured: Optional[Shape] = None


@dataclass
class Registry:
    """One workspace pointer's registry entry and the calls made on it."""
    entry: Optional[Entry] = None
    log: List[Step] = field(default_factory=list)

    def reset(self, shape: Shape) -> None:
        cap = self.entry.captured if self.entry else None
        self.entry = Entry(shape, 0, True, layout(shape).diag, cap)

    def _enter(self, shape: Shape, capturing: bool) -> Tuple[bool, bool]:
        changed = moved = False
        if self.entry is None:
            self.entry = Entry(shape, 0, False, layout(shape).diag)
        elif self.entry.shape != shape:
            moved = self.entry.diag != layout(shape).diag
            self.entry = Entry(shape, 0, True, layout(shape).diag, self.entry.captured)
            changed = True
        if capturing:
            self.entry.captured = shape
        return changed, moved

    def call(self, kind: str, shape: Shape, *, inplace: bool = False, aligned: bool = True,
             capturing: bool = False) -> Step:
        enters, kernel, gated = KINDS[kind]
        B, H, W, _bytes = shape
        rezero = moved = False
        if enters:
            rezero, moved = self._enter(shape, capturing)
        vec = W % 8 == 0 and aligned
        items = (H // 2) * (W // 8)
        lookback = kernel is not None and vec and items > 0
        e = self.entry
        sc = (lookback and not gated and not inplace and B <= FLAT_MAXB and not capturing
              and (e.captured is None or e.captured == shape) and (H // 2) * (W // 2) <= SC_MAX_NC)
        step = Step(kind, shape, kernel if lookback else None, sc, None, 1 if lookback else None,
                    0 if lookback else None, rezero, moved, False)
        if sc:
            step.fresh = not e.sc_clean
            e.sc_clean = True
            step.epoch = e.epoch
            step.par, step.tag = e.epoch & 1, tag_of(e.epoch)
            e.epoch = (e.epoch + 1) % EPOCHS
        self.log.append(step)
        return step
