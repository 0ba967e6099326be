"""Box convolution (msau_amd/csrc/boxconv.hip): a float64 reference written from the definition in that file's header comment, the
bounds the GPU tests hold the kernels to, input generators and the buffer plumbing.  Nothing here goes through msau_amd/plan.py or
oracle/box_oracle.py: tests/test_box_cpu.py checks this file against the oracle, autograd and finite differences,
tests/test_box_ops_gpu.py checks the kernels against this file.

Definition (pixels are unit squares, the image is zero outside; boxes (hmin, hmax, wmin, wmax)[c][f] in PIXELS; x_* are rows, y_*
are columns in the stored parameters):

    II[b,c,i,j]       = sum x~[b,c,0..i,0..j)          x~ = relu(x) under relu_in; row 0 and column 0 are zero
    out[b,c*F+f,y,x]  = 1/A * integral of x~[b,c] over rows [y+hmin, y+hmax+1) x columns [x+wmin, x+wmax+1)
                      = (Wy_f . x~ . Wx_f^T)[y,x] / A,   Wy[y,u] = |[u,u+1) n [y+hmin, y+hmax+1)|,   A = (hmax-hmin+1)(wmax-wmin+1)
    gin[b,c]          = sum_f  the same filter with the reflected box (-hmax, -hmin, -wmax, -wmin) applied to g[b,c*F+f]
    epilogue          v *= (mask_a > 0);  v += add;  v += old (accumulate);  v *= (mask_b > 0)

The kernels read the integral as the bilinear interpolation of the fp32 II at the four corners, the corner positions formed in fp32
as `fp32(y) + hmin` and `(fp32(y) + hmax) + 1`, clamped to [0, H]: two IEEE additions, which no contraction changes.  lerp_weights()
repeats exactly that, so a reference evaluated on the II a launch wrote (float64 arithmetic on the launch's own operand) differs
from the launch only by the fp32 rounding of the 16 taps, of 1/A and of the product.

Box-parameter gradient (pixel units, times the max-size factor).  With S the box integral and O = S / A:
    dO/dhmax = (dS/dhmax - O * ww) / A,   dO/dhmin = (dS/dhmin + O * ww) / A,   ww = wmax - wmin + 1   (hh for the columns)
    dS/dhmax = +(line integral of row floor(p) over the box columns),  p = y + hmax + 1,  WHEN 0 <= p < H, otherwise 0
    dS/dhmin = -(the same with p = y + hmin)                                                    (columns: 0 <= p < W)
ONE rule: the derivative towards +.  An edge at p moves into row floor(p) when it moves up; at p < 0 and at p >= H it moves through
nothing.  p == 0 is inside (row 0), p == H is not.  edge_weights() states it once.

Bounds (derived here, none tuned against the kernels):
  int inputs (integers in [-2, 2], boxes multiples of 1/8):
    II       every entry is an integer below 2^24: the fp32 II EQUALS the float64 one.
    filter   the tap weights have 3 fractional bits, every lerp product and sum at most 6, the values stay below 2^17: exact, fused or
             not.  1/A, the product with it, the sum over F and each epilogue addition round (<= 2^-24 each, relative to what they
             produce): |got - ref| <= 2^-21 * (sum_f |v_f| + |add| + |old|), room for a division that is not correctly rounded.
             bf16 storage adds half a bf16 ulp.
  rand inputs (0.5 * randn rounded to the storage type, arbitrary fp32 boxes):
    II       |ii - ref| <= (H + W) 2^-24 P[i,j], P the float64 II of |x~|: the worst case of a sequential fp32 sum of <= H + W terms.
    filter   against its OWN II: |got - ref| <= 2^-21 * (sum |weight * II| over the 16 taps) / A (+ the addends, + half a bf16 ulp).
  parameter gradient, both kinds: |got - ref| <= REL * S + ABS, the fp32-summation bound of tests/wgrad_util.py, S = the sum over the
    pixels of the per-pixel terms |g| (|dS| + |O| ww) / A (param_grad(mag="terms") on the II of |x~|).  int: ref from the exact II
    (the kernel's II arithmetic is exact there, only the sums round).  rand: ref from the device's own II.  There the kernel's taps
    also round at the size of II, which S does not contain: a bound over the tap magnitudes (mag="taps") would cover that in the
    worst case, but it cannot see a dropped edge term (tests/test_box_cpu.py), so the sharper S is the one asserted; the kernels use
    4 % of it at the test shapes (profiles/box_tests.md).
"""
import ctypes as C
import dataclasses

import numpy as np
import torch

from msau_amd import _lib as L

REL, ABS = 2e-5, 1e-12             # tests/wgrad_util.py: held by fp32 sums of 1.4 M terms
FILTER_REL = 2.0 ** -21
GUARD = 1024                       # elements behind every output buffer that no launch may touch
TNAME = {L.F32: "f32", L.BF16: "bf16"}
NAN = float("nan")


def torch_dtype(dtype):
    return torch.float32 if dtype == L.F32 else torch.bfloat16


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """one geometry; Cs: stored input channels (> C: padded), the stored output channels are C * F rounded up to 8"""
    name: str
    H: int = 9
    W: int = 23
    C: int = 8
    Cs: int = 8
    F: int = 3
    B: int = 2
    max_size: float = 28.0

    @property
    def CF(self):
        return self.C * self.F

    @property
    def Cs_out(self):
        return -(-self.CF // 8) * 8


# one base case per mechanism, the other axes small; then three mixed ones
CASES = ([Case("base")]
         + [Case(f"W{w}", W=w) for w in (63, 64, 65, 130)]                 # column tiles of 64; the row scan's 64-lane chunks of W + 1
         + [Case(f"H{h}", H=h) for h in (7, 32, 33, 70)]                   # 32-row segments; 8-row blocks of the parameter gradient
         + [Case("C5of8", C=5), Case("C16F2", C=16, Cs=16, F=2), Case("F1", F=1), Case("C3of8F1", C=3, F=1)]
         + [Case("mix-C5-33x65", H=33, W=65, C=5), Case("mix-C16F2-7x130", H=7, W=130, C=16, Cs=16, F=2),
            Case("mix-C3F1-70x64", H=70, W=64, C=3, F=1, B=1)])
LDS_CASE = Case("lds-C192-5x70", H=5, W=70, C=192, Cs=192, F=1, B=1)       # 192 * 129 * 4 bytes > 60 KiB: the opt-in LDS path
LARGEST = max(CASES, key=lambda c: c.H * c.W)
EPILOGUES = {"none": (), "mask_a": ("mask_a",), "add": ("add",), "accumulate": ("old",), "mask_b": ("mask_b",),
             "all": ("mask_a", "add", "old", "mask_b")}


def make_inputs(c: Case, kind, dtype, seed=0):
    """float64 NCHW tensors holding storage-type values: x [B][C], g [B][C*F] (output gradient), add / old / masks [B][C] for the
    summed form's epilogue; params fp32 [4][C*F] in pixels"""
    gen = torch.Generator().manual_seed(1000 * seed + (7 if kind == "int" else 11) + 13 * c.H + c.W)
    d = {"x": draw(kind, (c.B, c.C, c.H, c.W), gen, dtype), "g": draw(kind, (c.B, c.CF, c.H, c.W), gen, dtype)}
    for k in ("add", "old", "mask_a", "mask_b"):
        d[k] = draw(kind, (c.B, c.C, c.H, c.W), gen, dtype)
    d["params"] = make_boxes(kind, c.C, c.F, c.H, c.W, gen, rot=c.H + c.C)
    return d


# ---- inputs ----------------------------------------------------------------------------------------------------------------
_INT_VALUES = torch.tensor([-2.0, -1.0, 0.0, 0.0, 1.0, 2.0])


def draw(kind, shape, gen, dtype):
    """'int': integers in [-2, 2], a third of them zero; 'rand': 0.5 * randn; both rounded to the storage type; float64"""
    v = _INT_VALUES[torch.randint(0, 6, shape, generator=gen)] if kind == "int" else 0.5 * torch.randn(shape, generator=gen)
    return v.to(torch_dtype(dtype)).double()


def special_boxes(H, W):
    """(hmin, hmax, wmin, wmax) in pixels, multiples of 1/8: the boxes at which box kernels go wrong"""
    return [(0.375, 0.375, -0.625, -0.625),                   # one pixel (min == max) at a fractional offset
            (-1.0, 2.0, -2.0, 1.0),                           # integer edges: y + hmin == 0 for a whole row, x + wmin == 0 for a column
            (-H - 1.5, H + 0.5, -W - 2.5, W + 1.5),           # larger than the image on both sides, from every pixel
            (H + 1.0, H + 3.0, -1.0, 1.0),                    # wholly outside, below
            (-2.0, 1.0, -W - 4.0, -W - 2.0),                  # wholly outside, to the left
            (-6.25, 5.5, 0.25, 0.5),                          # tall and thin, off-centre: rows and columns cannot be swapped unseen
            (0.125, 0.375, -7.5, 6.25),                       # flat and wide
            (0.0, 0.0, 0.0, 0.0)]                             # the pixel itself: every edge on an integer, y + hmin == 0 at y == 0


def make_boxes(kind, Cn, F, H, W, gen, rot=0):
    """fp32 [4][Cn*F] in pixels.  The first min(Cn*F, 8) pairs are special_boxes() (starting at `rot`), the rest random with
    hmax >= hmin.  'int': multiples of 1/8, a third of the random ones integers; 'rand': arbitrary fp32 (the specials jittered)"""
    CF = Cn * F
    centre = (torch.rand(2, CF, generator=gen) - 0.5) * 8
    half = torch.rand(2, CF, generator=gen) * 4
    p = torch.stack([centre[0] - half[0], centre[0] + half[0], centre[1] - half[1], centre[1] + half[1]])
    sp = special_boxes(H, W)
    for k in range(min(CF, len(sp))):
        p[:, k] = torch.tensor(sp[(k + rot) % len(sp)])
    if kind == "int":
        p = torch.round(p * 8) / 8
        whole = torch.arange(CF) % 3 == 2
        whole[:min(CF, len(sp))] = False
        p[:, whole] = torch.round(p[:, whole])
    else:
        j = 0.02 * (torch.rand(2, CF, generator=gen) - 0.5)
        p = p + torch.stack([j[0], j[0] + 0.01, j[1], j[1] + 0.01])
    p = p.float()
    assert bool((p[1] >= p[0]).all() and (p[3] >= p[2]).all())
    return p.contiguous()


def reflected(params):
    return torch.stack([-params[1], -params[0], -params[3], -params[2]]).contiguous()


def to_nhwc(t, Cs, dtype, pad=0.0):
    """float64 [B][C][H][W] -> storage type [B][H][W][Cs]; the padded channels hold `pad`"""
    B, Cn, H, W = t.shape
    out = torch.full((B, H, W, Cs), pad, dtype=torch_dtype(dtype))
    out[..., :Cn] = t.permute(0, 2, 3, 1).to(torch_dtype(dtype))
    return out


def to_nchw(t, Cn):
    return t[..., :Cn].permute(0, 3, 1, 2).double().cpu().contiguous()


# ---- the reference ---------------------------------------------------------------------------------------------------------
def integral(xt):
    """float64 [B][C][H][W] -> [B][C][H+1][W+1]"""
    B, Cn, H, W = xt.shape
    ii = torch.zeros(B, Cn, H + 1, W + 1, dtype=torch.float64)
    ii[:, :, 1:, 1:] = xt.double().cumsum(2).cumsum(3)
    return ii


def edges(n, lo, hi):
    """the two edge positions of every output coordinate as the kernels form them: fp32 [P][n] each"""
    y = torch.arange(n, dtype=torch.float32)[None, :]
    return y + lo.float()[:, None], (y + hi.float()[:, None]) + 1.0


def lerp_weights(p, N):
    """float64 [P][n][N+1]: the weights of the two taps of the linear interpolation at clamp(p, 0, N)"""
    v = p.clamp(0.0, float(N))
    fl = v.floor()
    f, i = (v - fl).double(), fl.long()
    w = torch.zeros(*p.shape, N + 1, dtype=torch.float64)
    w.scatter_add_(2, i[..., None], (1 - f)[..., None])
    w.scatter_add_(2, (i + 1).clamp(max=N)[..., None], f[..., None])
    return w


def edge_weights(p, N):
    """float64 [P][n][N+1]: d/dp of the interpolation TOWARDS +: II[floor(p) + 1] - II[floor(p)] when 0 <= p < N, else nothing"""
    inside = ((p >= 0) & (p < N)).double()
    i = p.clamp(0.0, float(N - 1)).floor().long()
    w = torch.zeros(*p.shape, N + 1, dtype=torch.float64)
    w.scatter_add_(2, (i + 1)[..., None], inside[..., None])
    w.scatter_add_(2, i[..., None], -inside[..., None])
    return w


def areas(params):
    """float64 (hh, ww, A) per pair, from the fp32 boxes"""
    q = params.double()
    hh, ww = q[1] - q[0] + 1, q[3] - q[2] + 1
    return hh, ww, hh * ww


def filter_from_ii(ii, params, H, W, plane_of_pair):
    """the four-corner formula in float64 on the given II ([B][planes][H+1][W+1], pair p reads plane plane_of_pair[p]):
    -> (v, m) [B][P][H][W]: the normalised box integral of every pair and sum |weight * II| / A over its 16 taps"""
    r1, r2 = edges(H, params[0], params[1])
    c1, c2 = edges(W, params[2], params[3])
    R1, R2, C1, C2 = lerp_weights(r1, H), lerp_weights(r2, H), lerp_weights(c1, W), lerp_weights(c2, W)
    A = areas(params)[2][None, :, None, None]
    pl = ii.double()[:, plane_of_pair]
    v = torch.einsum("pyi,bpij,pxj->bpyx", R2 - R1, pl, C2 - C1) / A
    m = torch.einsum("pyi,bpij,pxj->bpyx", R2 + R1, pl.abs(), C2 + C1) / A
    return v, m


def overlap(n, lo, hi):
    """float64 [P][n][n]: |[u, u+1) n [y + lo, y + hi + 1)| for output y, input u -- restricted to the image by u's range"""
    y = torch.arange(n, dtype=torch.float64).view(1, n, 1)
    u = torch.arange(n, dtype=torch.float64).view(1, 1, n)
    a, b = y + lo.double().view(-1, 1, 1), y + hi.double().view(-1, 1, 1) + 1
    return (torch.minimum(u + 1, b) - torch.maximum(u, a)).clamp_min(0)


def filter_def(xt, params, plane_of_pair):
    """the definition, no integral image: xt float64 [B][planes][H][W] -> [B][P][H][W]"""
    H, W = xt.shape[2:]
    Wy, Wx = overlap(H, params[0], params[1]), overlap(W, params[2], params[3])
    return torch.einsum("pyu,bpuv,pxv->bpyx", Wy, xt.double()[:, plane_of_pair], Wx) / areas(params)[2][None, :, None, None]


def fwd_planes(Cn, F):
    return torch.arange(Cn * F) // F


def sum_filters(v, Cn, F):
    B, _, H, W = v.shape
    return v.view(B, Cn, F, H, W).sum(2)


def epilogue(v, S, mask_a=None, add=None, old=None, mask_b=None):
    """the documented order on the value and on its magnitude: mask_a, + add, + old, mask_b (all float64 NCHW)"""
    if mask_a is not None:
        v, S = v * (mask_a > 0), S * (mask_a > 0)
    for t in (add, old):
        if t is not None:
            v, S = v + t, S + t.abs()
    if mask_b is not None:
        v, S = v * (mask_b > 0), S * (mask_b > 0)
    return v, S


def param_grad(ii, params, g, max_h, max_w, mag=None, drop=None):
    """float64 [4][P]: the gradient of sum(g * out) w.r.t. the STORED (hmin, hmax, wmin, wmax), out the forward filter of the planes
    behind `ii` ([B][C][H+1][W+1]; g [B][P][H][W], pair p reads plane p // F).
    mag=None: the gradient.  Magnitudes of its terms, g = |g| and the edge and normalisation parts ADDED:
    mag="terms": `ii` is the II of |x~| -- per pixel |g| (|dS| + |O| ww) / A;  mag="taps": `ii` as read, |II| under |weights|."""
    B, P, H, W = g.shape
    F = P // ii.shape[1]
    r1, r2 = edges(H, params[0], params[1])
    c1, c2 = edges(W, params[2], params[3])
    R1, R2, C1, C2 = lerp_weights(r1, H), lerp_weights(r2, H), lerp_weights(c1, W), lerp_weights(c2, W)
    E = [edge_weights(r1, H), edge_weights(r2, H), edge_weights(c1, W), edge_weights(c2, W)]
    hh, ww, A = areas(params)
    pl = ii.double()[:, fwd_planes(P // F, F)]
    g = g.double()
    if mag == "taps":
        pl, Dy, Dx, E = pl.abs(), R2 + R1, C2 + C1, [e.abs() for e in E]
    else:
        Dy, Dx = R2 - R1, C2 - C1
    gi = torch.einsum("bpyx,pyi,bpij,pxj->p", g, Dy, pl, Dx)                  # sum g S
    edge = [torch.einsum("bpyx,pyi,bpij,pxj->p", g, E[0], pl, Dx), torch.einsum("bpyx,pyi,bpij,pxj->p", g, E[1], pl, Dx),
            torch.einsum("bpyx,pyi,bpij,pxj->p", g, Dy, pl, E[2]), torch.einsum("bpyx,pyi,bpij,pxj->p", g, Dy, pl, E[3])]
    if drop is not None:                                                      # (test_box_cpu.py: a kernel that loses one edge term)
        edge[drop[0]][drop[1]] = 0.0
    norm = [gi / A * ww, gi / A * ww, gi / A * hh, gi / A * hh]               # sum g O * (dA / d edge)
    scale = [max_h, max_h, max_w, max_w]
    if mag is not None:
        return torch.stack([(edge[k].abs() + norm[k].abs()) / A * scale[k] for k in range(4)])
    sign = [-1.0, 1.0, -1.0, 1.0]                                             # a min edge moving towards + SHRINKS the box
    return torch.stack([sign[k] * (edge[k] - norm[k]) / A * scale[k] for k in range(4)])


def box_params_ref(flat, offs, CF, rh, rw):
    """msau_box_params restated in float32: scale, clamp to the max size, max >= min; -> (fwd [4][CF], reflected [4][CF])"""
    v = [(flat[o:o + CF] * torch.tensor(r, dtype=torch.float32)).clamp(-r, r) for o, r in zip(offs, (rh, rh, rw, rw))]
    fwd = torch.stack([v[0], torch.maximum(v[1], v[0]), v[2], torch.maximum(v[3], v[2])])
    return fwd, reflected(fwd)


# ---- fp32 prefix sums in numpy (test_box_cpu.py: how much of ii_bound() real summation orders use) ------------------------------
def ii_fp32(x, order):
    """fp32 integral image [N][H+1][W+1] of x [N][H][W], every addition rounded to fp32.
    'kernel': boxconv.hip -- column sums in 32-row segments (each segment starts from the sequential sum of the earlier segments'
    totals), then every row scanned in 64-lane chunks of W + 1 (Hillis-Steele steps 1, 2, .. 32, plus the carry of the chunk before);
    'cols-rows' / 'rows-cols': plain sequential running sums, down the columns first / along the rows first"""
    x = np.asarray(x, dtype=np.float32)
    N, H, W = x.shape
    ii = np.zeros((N, H + 1, W + 1), dtype=np.float32)
    if order == "rows-cols":
        ii[:, 1:, 1:] = np.add.accumulate(np.add.accumulate(x, axis=2, dtype=np.float32), axis=1, dtype=np.float32)
        return ii
    if order == "cols-rows":
        ii[:, 1:, 1:] = np.add.accumulate(np.add.accumulate(x, axis=1, dtype=np.float32), axis=2, dtype=np.float32)
        return ii
    assert order == "kernel"
    seg_rows = 32
    totals = [np.add.accumulate(x[:, y0:y0 + seg_rows], axis=1, dtype=np.float32)[:, -1] for y0 in range(0, H, seg_rows)]
    for s, y0 in enumerate(range(0, H, seg_rows)):
        acc = np.zeros((N, W), dtype=np.float32)
        for t in totals[:s]:
            acc = acc + t
        for y in range(y0, min(H, y0 + seg_rows)):
            acc = acc + x[:, y]
            ii[:, y + 1, 1:] = acc
    carry = np.zeros((N, H + 1), dtype=np.float32)
    for x0 in range(0, W + 1, 64):
        v = np.zeros((N, H + 1, 64), dtype=np.float32)
        n = min(64, W + 1 - x0)
        v[..., :n] = ii[:, :, x0:x0 + n]
        o = 1
        while o < 64:
            v[..., o:] = v[..., o:] + v[..., :-o].copy()
            o *= 2
        v = v + carry[..., None]
        ii[:, :, x0:x0 + n] = v[..., :n]
        carry = v[..., 63]
    return ii


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120))) - 7)


def ii_bound(kind, P, H, W):
    """int: the fp32 II is exact (asserts that the sums stay below 2^24); rand: (H + W) 2^-24 P"""
    if kind == "int":
        assert float(P.max()) < 2 ** 24
        return torch.zeros_like(P)
    return (H + W) * 2.0 ** -24 * P


def filter_bound(S, got, ref, dtype):
    """2^-21 S, plus half a bf16 ulp of the stored value in bf16 storage"""
    b = FILTER_REL * S
    if dtype == L.BF16:
        b = b + 0.5 * ulp_bf16(torch.maximum(got.abs(), ref.abs())) * (1 + 1e-6)
    return b


def assert_int_filter_exact(ii):
    """every intermediate of the four lerps is a combination of at most four II values with at most 6 fractional bits"""
    assert 4 * float(ii.abs().max()) < 2 ** 17, "the integer case is too large for exact fp32 lerps"


def check(got, ref, bound, what):
    """|got - ref| <= bound element-wise (a zero bound means equality; NaN never passes); returns the worst error / bound"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        w = torch.where(bad, err - bound, torch.zeros_like(err))
        w = torch.where(torch.isnan(w), torch.full_like(w, float("inf")), w)
        i = int(w.flatten().argmax())
        idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst at {idx}: got "
                             f"{float(got.flatten()[i])!r} want {float(ref.flatten()[i])!r} bound {float(bound.flatten()[i]):.3g}; "
                             f"first {[tuple(r) for r in bad.nonzero()[:4].tolist()]}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


# ---- buffers ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """a device buffer of n elements, GUARD more behind it, all NaN (or `fill` in the first n)"""

    def __init__(self, n, dtype=torch.float32, fill=None, device="cuda"):
        self.n = n
        self.full = torch.full((n + GUARD,), NAN, dtype=dtype, device=device)
        if fill is not None:
            self.full[:n] = fill.reshape(-1).to(device=device, dtype=dtype)

    @property
    def data(self):
        return self.full[:self.n]

    def ptr(self):
        return self.full.data_ptr()

    def assert_guard(self, what):
        assert bool(torch.isnan(self.full[self.n:]).all()), f"{what}: the guard band behind the buffer was written"


WORST = {}                         # test group -> worst error / bound seen in this process (printed by the GPU tests)


def record(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    return ratio


def box_args(**kw):
    a = L.BoxArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def byref(a):
    return C.byref(a)
