"""Row-streaming convolutions (msau_amd/csrc/conv_rows.hip through msau_conv2d / msau_conv_pair): float64 references written from the
definitions in include/msau_hip.h, the bounds the GPU tests hold the kernels to, input generators, the tensor layout of a launch
and the descriptor plumbing.  Nothing here goes through the product's own helpers (plan.py, tests/hip_harness.py, the oracle):
tests/test_rows_cpu.py checks this file against autograd, tests/test_rows_gpu.py checks the kernels against this file.
(ACC and assert_rounded are imported from tests/test_launch_ulp_gpu.py, not restated; importing that module loads msau_amd.model,
msau_amd.plan and the oracle as a side effect -- nothing of them is used here.)

Host tensors are channel-last float64, [B][H][W][C], as the kernels store them; weights are OIHW float64 of the conv the LAUNCH
performs (a data-gradient launch performs a conv with the flipped, transposed weight: `dgrad_weight`).

    conv          v(b, y, x, co) = sum_{ky, kx, c} in(b, y + ky - pad_t, x + kx - pad_l, c) W[co][c][ky][kx] + bias[co]      (zero outside)
    transposed    the same over the zero-stuffed image s(2y, 2x) = in(y, x), pad 1, cropped to Hout x Wout in {2 Hin, 2 Hin - 1}
    pair forward  mid = relu(W1 * relu(x) + b1);  y = relu(W2 * mid + b2 + x);  z = relu(Wc * concat(prev, y) + bc);  2x2 max pool
                  of the zero-padded z (or y) with the position of the first maximum
    pair backward mid = (W1 * x) . [fwd mid > 0];  y = (W2 * mid) . [x0 > 0] + x        (mask first, then the add: msau_hip.h)
                  MSAU_PAIR_LRN_BWD: lrn_da = LRN'(lrn_a)(y) in place of y;  MSAU_PAIR_WGRAD1: slabs of sum mid (x) relu(x0) in
                  place of mid

Every stage that consumes a stored (bf16) tensor is referenced on the DEVICE's own stored tensor: nothing propagates.

Bounds.  `int` / `sparse` inputs: every product and partial sum is an integer below 2^24, every intermediate that passes through
LDS in bf16 is an integer of at most 256, so each stored element EQUALS the bf16 round-to-nearest-even of the exact value whatever
the order of the sums.  `rand` inputs: |stored - exact| <= half a bf16 ulp + ACC * S (tests/test_launch_ulp_gpu.py: assert_rounded,
ACC = 3e-5), S = the sum of the magnitudes of the element's terms (the same reference on absolute values).  LRN outputs: the bounds
of tests/elementwise_util.py (fast form) plus the half ulp.  Slabs: REL, ABS and check_slabs of tests/wgrad_util.py.
"""
import contextlib
import ctypes as C
import dataclasses
import functools
import os

import numpy as np
import torch

from msau_amd import _lib as L
from tests import elementwise_util as E
from tests import wgrad_util as WU
from tests.test_launch_ulp_gpu import ACC, assert_rounded

KINDS = ("int", "sparse", "rand")
LRN_ALPHA, LRN_BETA, LRN_K = 1e-4, 0.75, 1.0
# every switch conv_rows.hip reads that moves a route or a task split: unset while a test's own settings hold
ROWS_ENV = ("MSAU_PAIR_ROWS", "MSAU_CONV_ROWS", "MSAU_DOUT_ROWS", "MSAU_DECONV_ROWS", "MSAU_ROWS_SH", "MSAU_ROWS_SH16", "MSAU_ROWS_WAVES",
            "MSAU_ROWS_MIN_TASKS", "MSAU_ROWS_MAXC", "MSAU_PAIR_WGRAD", "MSAU_PAIR_COUPLE", "MSAU_COUPLE_WGRAD", "MSAU_LRN_BWD16")


@contextlib.contextmanager
def rows_env(**switches):
    """the row family's switches set to `switches` (every other one of ROWS_ENV unset) and read by the library; both restored on exit"""
    saved = {k: os.environ.pop(k) for k in ROWS_ENV if k in os.environ}
    try:
        for k, v in switches.items():
            assert k in ROWS_ENV, k
            os.environ[k] = str(v)
        L.load().msau_reload_env()
        yield
    finally:
        for k in ROWS_ENV:
            os.environ.pop(k, None)
        os.environ.update(saved)
        L.load().msau_reload_env()


# ---- deliberately wrong references (tests/test_rows_cpu.py: the comparisons of the GPU tests reject each of them) ----------------
@dataclasses.dataclass(frozen=True)
class Mut:
    """defects a row kernel could really have; `strip` / `sh` = the strip width and segment height of the kernel they model"""
    strip: int = 30
    sh: int = 10
    last_column: bool = False      # the last column of a strip takes its neighbour's (the next strip's first) value
    seam_halo: bool = False        # the halo row above a segment seam is read as zero
    tap_shift: bool = False        # the first tap reads one column to the right
    bias_hi: bool = False          # the bias is missing from output channels 4..7
    mask_ge: bool = False          # ReLU masks taken as >= 0 instead of > 0
    pool_last: bool = False        # a tie in a pool window goes to the LAST maximum
    rtz: bool = False              # stores truncate instead of rounding to nearest even
    add_first_strip: bool = False  # the residual / other-path add happens in the first strip only


EXACT = Mut()
MUTATIONS = ("last_column", "seam_halo", "tap_shift", "bias_hi", "mask_ge", "pool_last", "rtz", "add_first_strip")
ROUNDING_ONLY = ("rtz",)


# ---- the references --------------------------------------------------------------------------------------------------------------
def shift(x, dy, dx):
    """s(b, y, x) = x(b, y + dy, x + dx), zero outside the image"""
    _, H, W, _ = x.shape
    out = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def conv(x, w, b=None, pad=(1, 1), mut=EXACT, order=None):
    """SAME conv from the definition.  `order` None: float64.  Otherwise a float32 evaluation, one product at a time: `order` = a list
    of blocks of (tap, channel) indices -- each block is summed from zero in its order, the blocks are added to the bias in turn (one
    block: a plain running sum; blocks of 32: the k-steps of an MFMA chain)."""
    Co, Ci, KH, KW = w.shape
    assert x.shape[-1] == Ci
    rows = torch.arange(x.shape[1])
    taps = []
    for ky in range(KH):
        for kx in range(KW):
            dy, dx = ky - pad[0], kx - pad[1]
            if mut.tap_shift and ky == 0 and kx == 0:
                dx += 1
            s = shift(x, dy, dx)
            if mut.seam_halo and dy == -1:
                s = s * (rows % mut.sh != 0).to(s.dtype)[None, :, None, None]
            taps.append(s)
    bias = None
    if b is not None:
        bias = b.clone()
        if mut.bias_hi:
            bias[4:8] = 0
    if order is None:
        out = torch.zeros(*x.shape[:3], Co, dtype=torch.float64)
        for t, s in enumerate(taps):
            out = out + s @ w[:, :, t // KW, t % KW].T
        if bias is not None:
            out = out + bias
    else:
        f = torch.float32
        out = torch.zeros(*x.shape[:3], Co, dtype=f) + (bias.to(f) if bias is not None else 0)
        t32, w32 = [s.to(f) for s in taps], w.to(f)
        for block in order:
            part = torch.zeros_like(out)
            for t, c in block:
                part = part + t32[t][..., c:c + 1] * w32[:, c, t // KW, t % KW]
            out = out + part
        out = out.double()
    if mut.last_column:
        W = x.shape[2]
        cols = [c for c in range(W) if c % mut.strip == mut.strip - 1 and c + 1 < W]
        if cols:
            src = out.clone()
            out[:, :, cols] = src[:, :, [c + 1 for c in cols]]
    return out


def conv_mag(x, w, b=None, pad=(1, 1)):
    """S of a conv's elements: the sum of the magnitudes of their terms"""
    return conv(x.abs(), w.abs(), None if b is None else b.abs(), pad)


def orders(Ci, taps, seed):
    """the float32 summation orders of the headroom test: three shuffles as one running sum, the natural order in k-steps of 32"""
    rng = np.random.default_rng(seed)
    nat = [(t, c) for t in range(taps) for c in range(Ci)]
    out = [[[nat[i] for i in rng.permutation(len(nat))]] for _ in range(3)]
    out.append([nat[i:i + 32] for i in range(0, len(nat), 32)])
    return out


def stuffed(x, Hout, Wout):
    """the zero-stuffed image of a transposed conv on the output grid: s(2y, 2x) = x(y, x)"""
    B, Hin, Win, Cc = x.shape
    assert Hout in (2 * Hin, 2 * Hin - 1) and Wout in (2 * Win, 2 * Win - 1)
    s = torch.zeros(B, Hout, Wout, Cc, dtype=x.dtype)
    s[:, 0:2 * Hin:2, 0:2 * Win:2] = x
    return s


def deconv(x, w, b, Hout, Wout, mut=EXACT, order=None):
    """transposed conv 3x3, ups 2, pad 1 as msau_conv2d defines it: the conv of the stuffed image (taps beyond the output grid meet
    stuffed zeros or the image's end either way)"""
    return conv(stuffed(x, Hout, Wout), w, b, (1, 1), mut, order)


def dgrad_weight(w):
    """OIHW weight of a forward conv -> the OIHW weight of the conv its data gradient is: transposed and flipped"""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def mask(t, mut=EXACT):
    return ((t >= 0) if mut.mask_ge else (t > 0)).to(torch.float64)


def relu(t):
    return t.clamp_min(0)


def residual(v, add, mut=EXACT):
    if mut.add_first_strip:
        add = add.clone()
        add[:, :, mut.strip:] = 0
    return v + add


def store(v, mut=EXACT):
    """what a bf16 store leaves: round to nearest even (`v` is exact in float32 for int / sparse inputs and in the float32 model)"""
    f = v.float()
    if mut.rtz:
        return (f.view(torch.int32) & -65536).view(torch.float32).double()
    return f.bfloat16().double()


def pool(x, mut=EXACT):
    """-> (y, idx): elementwise_util.pool_fwd (first maximum in row-major order of the zero-padded window)"""
    if not mut.pool_last:
        return E.pool_fwd(x)
    v = E.pool_windows(x)
    best, idx = v[0].clone(), torch.zeros(v[0].shape, dtype=torch.uint8)
    for pos in range(1, 4):
        up = v[pos] >= best
        best = torch.where(up, v[pos], best)
        idx = torch.where(up, torch.full_like(idx, pos), idx)
    return best, idx


def pool_ties(x):
    """number of pool windows whose maximum occurs more than once"""
    v = E.pool_windows(x)
    return int(((v == v.max(0).values[None]).sum(0) > 1).sum())


def lrn_n(Cc):
    return Cc                                  # LocalResponseNorm(size = C) in both places the row kernels carry it


# ---- the cases: one per row of ROWPAIR_TABLE and ROWCONV_TABLE of conv_rows.hip -------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Shape:
    B: int
    H: int
    W: int
    why: str
    env: tuple = ()                # ((switch, value), ...) besides MSAU_ROWS_MIN_TASKS=1
    pad: int = None                # 4x4 instances: 1 (forward) or 2 (flipped data-gradient image)
    odd: tuple = (0, 0)            # transposed convs: (H, W) are the INPUT's, the output is 2 H - odd[0] by 2 W - odd[1]

    @property
    def id(self):
        e = "".join(f"-{k.replace('MSAU_ROWS_', '').lower()}{'.' if k[-1].isdigit() else ''}{v}" for k, v in self.env)
        p = f"-pad{self.pad}" if self.pad else ""
        o = f"-odd{self.odd[0]}{self.odd[1]}" if self.odd != (0, 0) else ""
        return f"{self.B}x{self.H}x{self.W}{e}{p}{o}"

    @property
    def switches(self):
        return dict(self.env, MSAU_ROWS_MIN_TASKS=1)

    @property
    def out_hw(self):
        return 2 * self.H - self.odd[0], 2 * self.W - self.odd[1]


SH = "MSAU_ROWS_SH"
# C8 pair: strips of 30 columns; segments of 10 rows by default (MSAU_ROWS_WAVES / tasks -> the minimum), MSAU_ROWS_SH as it is
PAIR8_SHAPES = (
    Shape(1, 1, 1, "W = 1, H = 1: exactly one task, one live lane column"),
    Shape(2, 2, 2, "W = 2, H = 2: both halo rows outside the image"),
    Shape(1, 10, 30, "exactly one task that fills its strip and its segment"),
    Shape(2, 11, 29, "W one short of a strip; default split 10 + 1: a one-row last segment"),
    Shape(2, 5, 30, "W = one full strip"),
    Shape(2, 3, 31, "W one column into the second strip"),
    Shape(3, 10, 61, "one column in the third strip; 9 tasks on 8 XCDs: idle waves (WG1: they wait at the slab reduction)"),
    Shape(2, 13, 31, "segments 6, 6, 1", ((SH, 6),)),
    Shape(2, 7, 61, "every row its own segment: each row's two halo rows belong to neighbours; 42 tasks (> 32)", ((SH, 1),)),
)
# pooled outputs (CPL = 2 at 8 and 16 channels, POOL at 16): 2x2 windows at odd ends and at seams
POOL8_SHAPES = (
    Shape(2, 1, 2, "H = 1, W >= 2: every window has no second row"),
    Shape(2, 2, 1, "W = 1, H >= 2: every window has no second column"),
    Shape(2, 11, 29, "odd H and W; default split 10 + 1"),
    Shape(2, 7, 31, "odd forced segment height below H: the ++SH branch of rowpair_split (4 + 3); odd W in the second strip", ((SH, 3),)),
    Shape(3, 10, 61, "9 tasks, odd W in the third strip"),
    Shape(2, 13, 61, "forced 5 -> 6: segments 6, 6, 1, the last window row alone in its segment", ((SH, 5),)),
    Shape(2, 7, 61, "forced 1 -> 2: a window per segment, 24 tasks", ((SH, 1),)),
)
# C16 pair: strips of 14 columns; MSAU_ROWS_SH16 = 16 by default
PAIR16_SHAPES = (
    Shape(1, 1, 1, "W = 1, H = 1: exactly one task"),
    Shape(2, 1, 13, "H = 1; W one short of a strip"),
    Shape(2, 17, 14, "W = one full strip; default split 16 + 1"),
    Shape(2, 17, 15, "one column in the second strip; 16 + 1"),
    Shape(3, 2, 29, "one column in the third strip, 9 tasks"),
    Shape(2, 9, 29, "forced small segments 4, 4, 1", ((SH, 4),)),
    Shape(2, 17, 13, "MSAU_ROWS_SH16 = 5: segments 5, 5, 5, 2", (("MSAU_ROWS_SH16", 5),)),
)
POOL16_SHAPES = (
    Shape(2, 1, 2, "H = 1, W >= 2"),
    Shape(2, 2, 1, "W = 1, H >= 2"),
    Shape(2, 17, 15, "odd H and W; default split 16 + 1: the last window row alone; odd W in the second strip"),
    Shape(2, 7, 29, "odd forced segment height below H: ++SH (4 + 3)", ((SH, 3),)),
    Shape(3, 5, 13, "odd H and W inside one strip"),
)
# rowconv8: strips of 32 output columns; segments of at least 8 rows rounded up to the loop's trip (3x3: 6, 1x1: 4, 4x4: 8), clamped to H
CONV8_SHAPES = (
    Shape(2, 1, 1, "W = 1, H = 1"),
    Shape(2, 8, 31, "W one short of a strip; H = the minimum segment"),
    Shape(2, 9, 32, "W = one full strip; H = 9: 4x4 / 1x1 split 8 + 1"),
    Shape(2, 13, 33, "one column in the second strip; H = 13: 3x3 splits 12 + 1, the others 8 + 5"),
    Shape(2, 25, 65, "one column in the third strip; H = 25: 12 + 12 + 1 / 8 + 8 + 8 + 1"),
    Shape(3, 1, 65, "H = 1 over three strips"),
    Shape(2, 13, 1, "W = 1 over two segments"),
    Shape(2, 9, 33, "MSAU_ROWS_SH = 1: raised to the minimum, rounded to the trip", ((SH, 1),)),
)
# transposed convs: strips of 16 input columns, segments of 8 output rows, the last one bounded by the kernel; (H, W) = the input's
DECONV_SHAPES = (
    Shape(2, 1, 1, "one input pixel -> 2 x 2"),
    Shape(2, 1, 16, "one input row -> ONE output row of 31", odd=(1, 1)),
    Shape(2, 4, 15, "7 x 29: one short of a strip, odd in both directions", odd=(1, 1)),
    Shape(2, 5, 16, "10 x 31: a full strip whose last output column is missing; segments 8 + 2", odd=(0, 1)),
    Shape(2, 9, 17, "17 x 34: one input column in the second strip; segments 8 + 8 + 1", odd=(1, 0)),
    Shape(2, 4, 33, "8 x 66: one input column in the third strip; exactly one segment"),
    Shape(3, 5, 17, "9 x 33: a one-row last segment, 12 tasks", odd=(1, 1)),
)


@dataclasses.dataclass(frozen=True)
class PairCase:
    """X(C16, BWD, BITS, LRNB, WG1, CPL, POOL) of ROWPAIR_TABLE: C16 = 16 channels; BWD = the data-gradient flag set; BITS = ballot planes
    written (forward) / read (backward); LRNB = MSAU_PAIR_LRN_BWD; WG1 = MSAU_PAIR_WGRAD1; CPL = 0 none, 1 the coupling conv, 2 also its
    pooled output; POOL = MSAU_CONV_POOL on y"""
    name: str
    c16: bool
    bwd: bool
    bits: bool
    lrnb: bool = False
    wg1: bool = False
    cpl: int = 0
    pool: bool = False

    @property
    def C(self):
        return 16 if self.c16 else 8

    @property
    def pooled(self):
        return self.pool or self.cpl == 2

    @property
    def shapes(self):
        if self.pooled:
            return POOL16_SHAPES if self.c16 else POOL8_SHAPES
        return PAIR16_SHAPES if self.c16 else PAIR8_SHAPES

    @property
    def flag_set(self):
        f1 = L.PAIR_MASK_MID if self.bwd else L.PAIR_RELU_IN | L.PAIR_RELU_MID
        f1 |= (L.PAIR_LRN_BWD if self.lrnb else 0) | (L.PAIR_WGRAD1 if self.wg1 else 0) | (L.PAIR_COUPLE if self.cpl else 0)
        f2 = (L.CONV_MASK_A | L.CONV_ADD) if self.bwd else (L.CONV_ADD | L.CONV_RELU_OUT | (L.CONV_POOL if self.pool else 0))
        return (self.C, f1, f2, self.bits, self.cpl == 2)


def _fwd(c16, cpl, pool, tag):
    p = "c16" if c16 else "c8"
    return [PairCase(f"{p}-fwd-{tag}", c16, False, False, cpl=cpl, pool=pool), PairCase(f"{p}-fwd-{tag}-bits", c16, False, True, cpl=cpl, pool=pool)]


# ROWPAIR_TABLE, row by row
PAIR_CASES = tuple(
    _fwd(False, 0, False, "plain") + _fwd(False, 1, False, "cpl") + _fwd(False, 2, False, "cplpool")
    + [PairCase("c8-bwd-plain", False, True, True), PairCase("c8-bwd-lrnb", False, True, True, lrnb=True),
       PairCase("c8-bwd-wg1", False, True, True, wg1=True), PairCase("c8-bwd-lrnb-wg1", False, True, True, lrnb=True, wg1=True)]
    + _fwd(True, 0, False, "plain") + _fwd(True, 1, False, "cpl") + _fwd(True, 2, False, "cplpool") + _fwd(True, 0, True, "pool")
    + [PairCase("c16-bwd-plain", True, True, True), PairCase("c16-bwd-lrnb", True, True, True, lrnb=True)])


@dataclasses.dataclass(frozen=True)
class ConvCase:
    """X(KIND, NS, KH, KW, EPI, EPI2, WG) of ROWCONV_TABLE: KIND = rowconv8 / rowdeconv8 / rowdeconv16; NS = sources (concat(x1, x2));
    EPI = flags without MSAU_CONV_WGRAD; EPI2 = flags2 (the second output of MSAU_CONV_DOUT); WG = the coupling conv's weight-gradient rider"""
    name: str
    kind: str                      # "conv8" | "deconv8" | "deconv16"
    ns: int
    k: int
    epi: int = 0
    epi2: int = 0
    wg: bool = False

    @property
    def dout(self):
        return bool(self.epi & L.CONV_DOUT)

    @property
    def cin(self):
        return {"conv8": 8, "deconv8": 16, "deconv16": 32}[self.kind]

    @property
    def cout(self):
        return {"conv8": 16 if self.dout else 8, "deconv8": 8, "deconv16": 16}[self.kind]

    @property
    def shapes(self):
        if self.kind != "conv8":
            return DECONV_SHAPES
        if self.k == 4:
            return tuple(dataclasses.replace(s, pad=p) for s in CONV8_SHAPES for p in (1, 2))
        return CONV8_SHAPES

    @property
    def flag_set(self):
        return (self.kind, self.ns, self.k, self.epi, self.epi2, self.wg)


# ROWCONV_TABLE, row by row
CONV_CASES = (
    ConvCase("k3-lrn", "conv8", 1, 3, L.CONV_LRN), ConvCase("k3-plain", "conv8", 1, 3), ConvCase("k3-accum", "conv8", 1, 3, L.CONV_ACCUM),
    ConvCase("k3-dual", "conv8", 2, 3), ConvCase("k1-dual-relu", "conv8", 2, 1, L.CONV_RELU_OUT),
    ConvCase("k4-plain", "conv8", 1, 4), ConvCase("k4-maskb", "conv8", 1, 4, L.CONV_MASK_B),
    ConvCase("k4-accum-maskb", "conv8", 1, 4, L.CONV_ACCUM | L.CONV_MASK_B),
    ConvCase("k3-dout", "conv8", 1, 3, L.CONV_DOUT), ConvCase("k3-dout-accum", "conv8", 1, 3, L.CONV_DOUT | L.CONV_ACCUM),
    ConvCase("k1-dout-maskb2", "conv8", 1, 1, L.CONV_DOUT, L.CONV_MASK_B), ConvCase("k1-dout-maskb2-wg", "conv8", 1, 1, L.CONV_DOUT, L.CONV_MASK_B, True),
    ConvCase("deconv8", "deconv8", 1, 3), ConvCase("deconv16", "deconv16", 1, 3))


def params(cases, pick=lambda c: True):
    """(case, shape, kind) of every case's own shape list"""
    import pytest
    return [pytest.param(c, s, k, id=f"{c.name}-{s.id}-{k}") for c in cases if pick(c) for s in c.shapes for k in KINDS]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
_INT = torch.tensor([-2.0, -1.0, 0.0, 0.0, 1.0, 2.0], dtype=torch.float64)
_W = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
_B = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0], dtype=torch.float64)


def draw(kind, what, shape, gen):
    """what = "act" (activations, gradients), "w", "b".  int: integers in [-2, 2], a third of them zero / weights in {-1, 0, 1} / biases
    integers in [-2, 2]; sparse: the same with 7 of 8 zero; rand: 0.5 randn and weights 0.2 randn rounded to bf16, biases 0.1 randn (fp32)"""
    if kind == "rand":
        v = torch.randn(shape, generator=gen, dtype=torch.float64) * {"act": 0.5, "w": 0.2, "b": 0.1}[what]
        return v.float().double() if what == "b" else E.bf16_round(v)
    table = {"act": _INT, "w": _W, "b": _B}[what]
    v = table[torch.randint(0, len(table), shape, generator=gen)]
    if kind == "sparse":
        v = v * (torch.randint(0, 8, shape, generator=gen) == 0)
    return v


def _gen(kind, *key):
    return torch.Generator().manual_seed(hash((KINDS.index(kind),) + tuple(int(k) for k in key)) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def pair_inputs(Cc, B, H, W, kind):
    """everything a residual block's forward and backward read: x (the block's input; the backward's x0), the forward weights w1, w2
    and biases, the coupling conv's prev / wc / bc, the backward's incoming gradient g and the LRN's input lrn_a.  Shared, never written."""
    gen = _gen(kind, Cc, B, H, W)
    act = lambda *s: draw(kind, "act", s, gen)
    return {"x": act(B, H, W, Cc), "prev": act(B, H, W, Cc), "g": act(B, H, W, Cc), "lrn_a": act(B, H, W, Cc),
            "w1": draw(kind, "w", (Cc, Cc, 3, 3), gen), "b1": draw(kind, "b", (Cc,), gen),
            "w2": draw(kind, "w", (Cc, Cc, 3, 3), gen), "b2": draw(kind, "b", (Cc,), gen),
            "wc": draw(kind, "w", (Cc, 2 * Cc, 1, 1), gen), "bc": draw(kind, "b", (Cc,), gen)}


@functools.lru_cache(maxsize=None)
def conv_inputs(case, B, H, W, kind):
    """x1, x2, w (OIHW of the launch's conv, both outputs' rows for DOUT), bias and, where the case reads them, y_old, mask_b, mask_b2, wg_x1"""
    gen = _gen(kind, CONV_CASES.index(case), B, H, W)
    act = lambda c: draw(kind, "act", (B, H, W, c), gen)
    inp = {"x1": act(case.cin), "x2": act(8) if case.ns == 2 else None,
           "w": draw(kind, "w", (case.cout, case.cin * case.ns, case.k, case.k), gen),
           "b": None if case.dout else draw(kind, "b", (case.cout,), gen)}
    # only what the case reads
    if case.epi & L.CONV_ACCUM:
        inp["y_old"] = act(8)
    if case.epi & L.CONV_MASK_B:
        inp["mask_b"] = act(8)
    if case.epi2 & L.CONV_MASK_B:
        inp["mask_b2"] = act(8)
    if case.wg:
        inp["wg_x1"] = act(8)
    return inp


# ---- the device model: the stages of a launch in turn, each stored in bf16 (tests/test_rows_cpu.py) ------------------------------
def lrn_consts(Cc):
    n = lrn_n(Cc)
    return n, LRN_ALPHA, LRN_BETA, LRN_K


def model_pair_fwd(case, inp, mut=EXACT, order=None):
    o1 = None if order is None else order[0]
    oc = None if order is None else order[1]
    got = {}
    got["mid"] = store(relu(conv(relu(inp["x"]), inp["w1"], inp["b1"], (1, 1), mut, o1)), mut)
    got["y"] = store(relu(residual(conv(got["mid"], inp["w2"], inp["b2"], (1, 1), mut, o1), inp["x"], mut)), mut)
    src = got["y"]
    if case.cpl:
        got["z"] = store(relu(conv(torch.cat([inp["prev"], got["y"]], -1), inp["wc"], inp["bc"], (0, 0), mut, oc)), mut)
        src = got["z"]
    if case.pooled:
        got["pool"], got["pool_idx"] = pool(src, mut)
    if case.bits:
        got["mask_mid"], got["mask_a"] = mask(got["mid"], mut), mask(inp["x"], mut)
    return got


def model_pair_bwd(case, inp, fwd, mut=EXACT, order=None):
    """`fwd`: the forward's outputs (mask_mid, mask_a: what the planes carry)"""
    o1 = None if order is None else order[0]
    got = {}
    wb1, wb2 = dgrad_weight(inp["w2"]), dgrad_weight(inp["w1"])
    got["mid"] = store(conv(inp["g"], wb1, None, (1, 1), mut, o1) * fwd["mask_mid"], mut)
    got["y"] = store(residual(conv(got["mid"], wb2, None, (1, 1), mut, o1) * fwd["mask_a"], inp["g"], mut), mut)
    if case.lrnb:
        n, al, be, k = lrn_consts(case.C)
        got["lrn_da"] = store(E.lrn_bwd(inp["lrn_a"], got["y"], n, al, be, k), mut)
    return got


def model_conv(case, shp, inp, mut=EXACT, order=None):
    pad = (shp.pad,) * 2 if case.k == 4 else (case.k // 2,) * 2
    if case.kind != "conv8":
        return {"y": store(deconv(inp["x1"], inp["w"], inp["b"], *shp.out_hw, mut, order), mut)}
    x = inp["x1"] if case.ns == 1 else torch.cat([inp["x1"], inp["x2"]], -1)
    v = conv(x, inp["w"], inp["b"], pad, mut, order)
    got = {}
    if case.dout:
        v1, v2 = v[..., :8], v[..., 8:]
        if case.epi & L.CONV_ACCUM:
            v1 = v1 + inp["y_old"]
        if case.epi2 & L.CONV_MASK_B:
            v2 = v2 * mask(inp["mask_b2"], mut)
        got["y"], got["y2"] = store(v1, mut), store(v2, mut)
        return got
    if case.epi & L.CONV_ACCUM:
        v = v + inp["y_old"]
    if case.epi & L.CONV_RELU_OUT:
        v = relu(v)
    if case.epi & L.CONV_MASK_B:
        v = v * mask(inp["mask_b"], mut)
    got["y"] = store(v, mut)
    if case.epi & L.CONV_LRN:
        n, al, be, k = lrn_consts(8)
        got["y2"] = store(E.lrn_fwd(got["y"], n, al, be, k), mut)
    return got


# ---- the comparisons (the GPU tests and the CPU tests call the same functions) ----------------------------------------------------
class Report:
    """the worst error / bound per group of a test; printed as RATIO lines"""
    def __init__(self, kind):
        self.kind, self.worst = kind, {}

    def add(self, group, ratio):
        self.worst[group] = max(self.worst.get(group, 0.0), ratio)

    def show(self, prefix):
        for g, r in self.worst.items():
            exact = self.kind != "rand" and not g.startswith("lrn")
            print(f"RATIO {prefix}-{g} {self.kind} {'equal' if exact else format(r, '.4f')}")

    def max(self):
        return max(self.worst.values(), default=0.0)


def hold(rep, group, got, ref, S, what):
    """int / sparse: bit for bit the bf16 rounding of the exact value.  rand: assert_rounded with ACC * S."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if rep.kind != "rand":
        assert float(S.max()) < 2 ** 24, f"{what}: the integer inputs are not exact in fp32"
        want = E.bf16_round(ref)
        bad = got != want
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the rounded exact value, first (b, y, x, c) {i}: "
                                 f"got {float(got[i])!r} want {float(want[i])!r}; rows {sorted(set(bad.nonzero()[:, 1].tolist()))[:8]} "
                                 f"columns {sorted(set(bad.nonzero()[:, 2].tolist()))[:8]} channels {sorted(set(bad.nonzero()[:, 3].tolist()))}")
        rep.add(group, 0.0)
        return
    rep.add(group, E.worst_ratio(got, ref, ACC * S, True))
    assert_rounded(got, ref, ACC * S, what)


def hold_lrn(rep, group, got, ref, bound, what):
    """LRN outputs: the fp32 bound of elementwise_util (fast form) and half a bf16 ulp, in every kind"""
    rep.add(group, E.worst_ratio(got, ref, bound, True))
    assert_rounded(got, ref, bound, what)


def verify_pair_fwd(case, inp, got, kind):
    """every output of a forward launch against float64 on the stage's own stored input"""
    rep = Report(kind)
    x, w1, w2 = inp["x"], inp["w1"], inp["w2"]
    hold(rep, "mid", got["mid"], relu(conv(relu(x), w1, inp["b1"])), conv_mag(relu(x), w1, inp["b1"]), "mid")
    hold(rep, "y", got["y"], relu(conv(got["mid"], w2, inp["b2"]) + x), conv_mag(got["mid"], w2, inp["b2"]) + x.abs(), "y")
    src = got["y"]
    if case.cpl:
        cat = torch.cat([inp["prev"], got["y"]], -1)
        hold(rep, "z", got["z"], relu(conv(cat, inp["wc"], inp["bc"], (0, 0))), conv_mag(cat, inp["wc"], inp["bc"], (0, 0)), "z")
        src = got["z"]
    if case.pooled:
        py, pi = E.pool_fwd(src)
        assert torch.equal(got["pool"], py), "pooled output: not the maximum of the stored tensor's zero-padded windows"
        if got.get("pool_idx") is not None:
            assert torch.equal(got["pool_idx"], pi), "pool positions: not the first maximum in row-major order"
        rep.add("pool", 0.0)
    return rep


def verify_pair_bwd(case, inp, got, fwd_mid, kind, dy=None, mid=None):
    """a data-gradient launch.  The masks are (the forward's stored mid > 0) and (x0 > 0): the planes are checked through what they do.
    `dy` (LRNB): the y the plain instance stored; `mid` (WG1): the intermediate gradient the plain instance stored."""
    rep = Report(kind)
    g, wb1, wb2 = inp["g"], dgrad_weight(inp["w2"]), dgrad_weight(inp["w1"])
    mm, ma = mask(fwd_mid), mask(inp["x"])
    if not case.wg1:
        hold(rep, "mid", got["mid"], conv(g, wb1) * mm, conv_mag(g, wb1) * mm, "gradient of mid")
        mid = got["mid"]
    if not case.lrnb:
        hold(rep, "y", got["y"], conv(mid, wb2) * ma + g, conv_mag(mid, wb2) * ma + g.abs(), "gradient of x")
    else:
        n, al, be, k = lrn_consts(case.C)
        hold_lrn(rep, "lrn_da", got["lrn_da"], E.lrn_bwd(inp["lrn_a"], dy, n, al, be, k),
                 E.lrn_bwd_bound(inp["lrn_a"], dy, n, al, be, k, True), "lrn_da")
    return rep


def plain_bwd(Cc):
    """the plain data-gradient case of the channel count"""
    return next(c for c in PAIR_CASES if c.C == Cc and c.bwd and not c.lrnb and not c.wg1)


def verify_planes(rep, case, inp, fwd_mid, bgot, kind):
    """The ballot planes of a forward launch are outputs of that instance, with a private layout: they are checked through what they
    do.  `bgot` = the plain data-gradient launch run on THESE planes; it must give the gradients masked by (stored mid > 0) and
    (x > 0).  Added to `rep` as groups planes-mid, planes-y."""
    for g, r in verify_pair_bwd(plain_bwd(case.C), inp, bgot, fwd_mid, kind).worst.items():
        rep.add("planes-" + g, r)


def verify_conv(case, shp, inp, got, kind):
    rep = Report(kind)
    if case.kind != "conv8":
        Ho, Wo = shp.out_hw
        s = stuffed(inp["x1"], Ho, Wo)
        hold(rep, "y", got["y"], conv(s, inp["w"], inp["b"]), conv_mag(s, inp["w"], inp["b"]), "y")
        return rep
    pad = (shp.pad,) * 2 if case.k == 4 else (case.k // 2,) * 2
    x = inp["x1"] if case.ns == 1 else torch.cat([inp["x1"], inp["x2"]], -1)
    v, S = conv(x, inp["w"], inp["b"], pad), conv_mag(x, inp["w"], inp["b"], pad)
    if case.dout:
        v1, S1, v2, S2 = v[..., :8], S[..., :8], v[..., 8:], S[..., 8:]
        if case.epi & L.CONV_ACCUM:
            v1, S1 = v1 + inp["y_old"], S1 + inp["y_old"].abs()
        if case.epi2 & L.CONV_MASK_B:
            v2, S2 = v2 * mask(inp["mask_b2"]), S2 * mask(inp["mask_b2"])
        hold(rep, "y", got["y"], v1, S1, "y")
        hold(rep, "y2", got["y2"], v2, S2, "y2")
        return rep
    if case.epi & L.CONV_ACCUM:
        v, S = v + inp["y_old"], S + inp["y_old"].abs()
    if case.epi & L.CONV_RELU_OUT:
        v = relu(v)
    if case.epi & L.CONV_MASK_B:
        v, S = v * mask(inp["mask_b"]), S * mask(inp["mask_b"])
    hold(rep, "y", got["y"], v, S, "y")
    if case.epi & L.CONV_LRN:
        n, al, be, k = lrn_consts(8)
        hold_lrn(rep, "lrn", got["y2"], E.lrn_fwd(got["y"], n, al, be, k), E.lrn_fwd_bound(got["y"], n, al, be, k, True), "LRN second output")
    return rep


# ---- slabs of the two weight-gradient riders ---------------------------------------------------------------------------------------
def wg1_reference(x0, gmid):
    """MSAU_PAIR_WGRAD1: the slab [1][8][80] of the block's first conv (3x3, ReLU on load), its S and the mask of its real columns"""
    B, H, W, _ = x0.shape
    c = WU.Case("wg1", L.BF16, WU.ROWS, 8, 8, 3, B=B, hw=(H, W), flags=L.CONV_RELU_IN)
    ref, m = WU.reference(c, relu(x0), gmid, 8, 1, 80)
    S, _ = WU.reference(c, relu(x0).abs(), gmid.abs(), 8, 1, 80)
    return ref, S, m


def rider_reference(prev, cur, g):
    """MSAU_CONV_WGRAD: the slab [2][8][16] of the 1x1 coupling conv over concat(prev, cur): column c of chunk s = sum g[co] src_s[c],
    the ones column 8 in chunk 0 ONLY (chunk 1 holds a zero there)"""
    B, H, W, _ = g.shape
    c = WU.Case("cplwg", L.BF16, WU.ROWS, 8, 8, 1, C2=8, B=B, hw=(H, W))
    xt = torch.cat([prev, cur], -1)
    ref, _ = WU.reference(c, xt, g, 8, 2, 16)
    S, _ = WU.reference(c, xt.abs(), g.abs(), 8, 2, 16)
    ref[1, :, 8] = 0
    S[1, :, 8] = 0
    return ref, S


def check_rider_slabs(buf, nslabs, ref, S, kind, what):
    """wgrad_util.check_slabs chunk by chunk (the ones column is real in chunk 0 and padding in chunk 1)"""
    n = nslabs * 2 * 8 * 16
    slabs, guard = buf[:n].view(nslabs, 2, 8 * 16), buf[n:]
    worst = 0.0
    for ch in range(2):
        m = torch.zeros(16, dtype=torch.bool, device=buf.device)
        m[:9 - ch] = True
        sub = torch.cat([slabs[:, ch].reshape(-1), guard])
        worst = max(worst, WU.check_slabs(sub, nslabs, ref[ch:ch + 1].to(buf.device), S[ch:ch + 1].to(buf.device), m, kind, f"{what} chunk {ch}"))
    return worst


def slab_kind(kind):
    return "rand" if kind == "rand" else "int"


# ---- the packed weight image, as msau_pack_params writes it ------------------------------------------------------------------------
def pack_image(w, C1, C2, ups=1):
    """OIHW [Cout][C1 + C2][KH][KW] -> the packed bf16 image [chunk][row][k = tap * cch + c] with the geometry msau_conv_pack_geometry
    gives (asserted: the kernels of conv_rows.hip index exactly this), zero in the k padding and in the rows beyond Cout; on the CPU"""
    Co, Ci, KH, KW = w.shape
    assert Ci == C1 + C2
    g = L.ConvPackGeom()
    assert L.load().msau_conv_pack_geometry(L.BF16, C1, C2, Co, KH, KW, 1, 1, ups, C.byref(g)) == 0
    taps = KH * KW
    assert g.cch * g.nchunks == Ci and g.cch % 8 == 0, (g.cch, g.nchunks)
    assert g.rows == 16 and Co <= 16, g.rows                        # (16 rows: the row permutation of the tile kernels' epilogue is the identity)
    assert g.kchunk == -(-taps * g.cch // 32) * 32, (g.kchunk, taps, g.cch)
    assert g.bytes == g.nchunks * g.rows * g.kchunk * 2, g.bytes
    img = torch.zeros(g.nchunks, g.rows, g.kchunk, dtype=torch.float64)
    for ch in range(g.nchunks):
        img[ch, :Co, :taps * g.cch] = w[:, ch * g.cch:(ch + 1) * g.cch].permute(0, 2, 3, 1).reshape(Co, taps * g.cch)
    out = img.to(torch.bfloat16)
    assert torch.equal(out.double(), img), "the weights are not exact in bf16"
    return out.reshape(-1), g


# ---- descriptors and routes --------------------------------------------------------------------------------------------------------
def conv_desc(case, shp, **ptr):
    d = L.ConvDesc()
    d.B, d.Hin, d.Win = shp.B, shp.H, shp.W
    d.Hout, d.Wout = shp.out_hw if case.kind != "conv8" else (shp.H, shp.W)
    d.C1, d.C2, d.Cout = case.cin, (8 if case.ns == 2 else 0), case.cout
    d.KH = d.KW = case.k
    d.dil, d.stride, d.ups = 1, 1, (1 if case.kind == "conv8" else 2)
    d.pad_t = d.pad_l = shp.pad if case.k == 4 else case.k // 2
    d.flags, d.flags2 = case.epi | (L.CONV_WGRAD if case.wg else 0), case.epi2
    d.lrn_alpha_over_n, d.lrn_beta, d.lrn_k = LRN_ALPHA / lrn_n(8), LRN_BETA, LRN_K
    for k, v in ptr.items():
        setattr(d, k, v)
    return d


def pair_desc(case, shp, **ptr):
    d = L.ConvPairDesc()
    d.B, d.H, d.W, d.C = shp.B, shp.H, shp.W, case.C
    _, d.flags1, d.flags2, _, _ = case.flag_set
    d.lrn_alpha_over_n, d.lrn_beta, d.lrn_k = LRN_ALPHA / lrn_n(case.C), LRN_BETA, LRN_K
    for k, v in ptr.items():
        setattr(d, k, v)
    return d


def conv_route(d):
    info = (L.i32 * 8)()
    rc = L.load().msau_conv2d_launch_info(L.BF16, C.byref(d), info)
    return rc, list(info)


def pair_route(d):
    return L.load().msau_conv_pair_instance(L.BF16, C.byref(d))


_KEEP = (C.c_char * 64)()


def fake_pointers(case, d):
    """every operand the route of `case` asks for set to a host address (the queries read no operand)"""
    p = C.addressof(_KEEP)
    if isinstance(case, PairCase):
        for n in ("x", "add", "w1", "b1", "mid", "w2", "b2", "y"):
            setattr(d, n, p)
        if case.bits:
            d.bits_mid = d.bits_a = p
        if case.lrnb:
            d.lrn_a = d.lrn_da = p
        if case.wg1:
            d.wg1_x = d.wg1_slabs = p
        if case.cpl:
            d.cpl_prev = d.cpl_w = d.cpl_b = d.cpl_y = p
        if case.cpl == 2:
            d.cpl_pool_y = d.cpl_pool_idx = p
        if case.pool:
            d.pool_y = d.pool_idx = p
    else:
        for n in ("x1", "wpack", "bias", "y"):
            setattr(d, n, p)
        if case.ns == 2:
            d.x2 = p
        if case.dout or case.epi & L.CONV_LRN:
            d.y2 = p
        if case.epi & L.CONV_MASK_B:
            d.mask_b = p
        if case.epi2 & L.CONV_MASK_B:
            d.mask_b2 = p
        if case.wg:
            d.wg_x1 = d.wg_slabs = p
    return d


def conv_geometry(case):
    """(kchunk, rows) of the image msau_conv2d expects for the case"""
    g = L.ConvPackGeom()
    assert L.load().msau_conv_pack_geometry(L.BF16, case.cin, 8 if case.ns == 2 else 0, case.cout, case.k, case.k, 1, 1,
                                            1 if case.kind == "conv8" else 2, C.byref(g)) == 0
    return g


# ---- the layout of a launch's tensors on the device ----------------------------------------------------------------------------------
POISON_U8 = 0xA5
PLANE_GUARD = 1024


def dev_in(t, dtype=torch.bfloat16):
    """[B][...] host -> [B + 2][...] on the device, the first and the last image NaN: a read that strays shows in the values"""
    full = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), dtype=torch.float64)
    full[1:-1] = t
    out = full.to(dtype).cuda()
    assert torch.equal(out[1:-1].double().cpu(), t), "the input is not exact in its storage type"
    return out


def dev_out(B, rest, dtype=torch.bfloat16, init=None):
    """an output with one guard image before and after it, everything poison (NaN / 0xA5) unless `init` (what ACCUM adds to)"""
    if dtype == torch.uint8:
        return torch.full((B + 2,) + tuple(rest), POISON_U8, dtype=dtype, device="cuda")
    full = torch.full((B + 2,) + tuple(rest), float("nan"), dtype=torch.float64)
    if init is not None:
        full[1:-1] = init
    return full.to(dtype).cuda()


def ptr(full):
    return full[1:].data_ptr()


def _poison(t):
    return (t == POISON_U8) if t.dtype == torch.uint8 else torch.isnan(t)


def take(full, what):
    """guards untouched, every element inside written -> the inside on the host (float64, positions uint8).  An output that starts as
    `init` (MSAU_CONV_ACCUM: y_old) holds no poison inside, so for it "written" is only what the values show: an element the launch
    skipped keeps y_old and is caught by `hold` unless the conv term there is exactly 0."""
    assert bool(_poison(full[0]).all()) and bool(_poison(full[-1]).all()), f"{what}: a guard image was written"
    inner = full[1:-1]
    bad = _poison(inner)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements not written, first {tuple(bad.nonzero()[0].tolist())}"
    return inner.cpu() if full.dtype == torch.uint8 else inner.double().cpu()


def untouched(full, what):
    assert bool(_poison(full).all()), f"{what}: written by an instance that must leave it alone"


def plane_buffer(nbytes, fill):
    return torch.full((PLANE_GUARD + nbytes + PLANE_GUARD,), fill, dtype=torch.uint8, device="cuda")


def plane_ptr(buf):
    return buf[PLANE_GUARD:].data_ptr()


def plane_take(buf, fill, what):
    assert bool((buf[:PLANE_GUARD] == fill).all()) and bool((buf[-PLANE_GUARD:] == fill).all()), f"{what}: a guard band of the plane was written"
    return buf[PLANE_GUARD:-PLANE_GUARD]


def slab_buffer(nslabs, slab_elems):
    """NaN everywhere, wgrad_util.GUARD floats before and behind the slabs -> (whole buffer, the part check_slabs takes)"""
    full = torch.full((WU.GUARD + nslabs * slab_elems + WU.GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return full, full[WU.GUARD:]
