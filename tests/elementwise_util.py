"""Float64 references, inputs and bounds for the kernels of msau_amd/csrc/elementwise.hip (layout conversion, cross-channel LRN,
2x2 max pool, extent copy, one-hot ids).  Plain torch / numpy on the CPU; imports no kernel.  tests/test_elementwise_cpu.py proves
what is stated here, tests/test_elementwise_gpu.py holds the kernels to it.

Tensors are channel-last, [..., C], as the kernels store them (`lrn_bwd_ref` takes the channel dimension as an argument: the
plan-level check of test_launch_ulp_gpu.py works in NCHW).

LRN (torch.nn.LocalResponseNorm):   d_c = k + (alpha / n) sum_{j in F(c)} x_j^2,   y_c = x_c d_c^-beta
    forward window  F(c) = [c - n/2, c + (n-1)/2]
    adjoint window  A(c) = [c - (n-1)/2, c + n/2]           (j in A(c)  <=>  c in F(j))
    da_c = dy_c d_c^-beta - 2 beta (alpha / n) x_c sum_{j in A(c)} dy_j x_j d_j^(-beta-1)

The fp32 term of the LRN bounds (`lrn_fwd_bound`, `lrn_bwd_bound`), in units of EPS = 2^-24 (half an fp32 ulp); a "one-ulp"
transcendental costs 2:
    C_D = 2          d = k + (alpha/n) win: one multiply, one add (one rounding when contracted)
    rsq / sqrt form (beta == 0.75):  r = rsq(d) [2],  r * sqrt(r): the error of r enters 1.5 times [3 in all], sqrt [2], the
                     multiply [1]  ->  C_RSQ = 6;   1/d = r * r  ->  2 * 2 + 1 = 5
    exp / log form:  exp2(-beta * log2e * (ln2 * log2(d))):  log2 [2], ln2 and its multiply [2], beta's multiply [1], log2e and its
                     multiply [2] are 7 relative to the ARGUMENT -beta ln d, i.e. 7 |beta ln d| relative to the result; exp2 [2]
                     ->  2 + 7 |beta ln d|;   1/d = rcp(d) -> 2  (the generic kernel divides: 1)
    c_sum            the additions on the longest path to a window sum: 8 + log2 G + 2 for the fast kernel (a product and 7
                     additions in the lane, log2 G scan steps, the exclusive prefix, the difference from the total), min(n, C) for
                     the generic kernel (a product and at most n - 1 additions)
    T                what the window sum's error is relative to: the sum of x^2 over ALL channels for the fast kernel (differences
                     of prefix sums), the window's own sum for the generic one
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

EPS = 2.0 ** -24
C_D, C_RSQ, C_EXP, C_ARG = 2.0, 6.0, 2.0, 7.0
C_INV_RSQ, C_INV_RCP, C_INV_DIV = 5.0, 2.0, 1.0

# (alpha as a multiple of n or None for the reference's 1e-4, beta, k, input scale)
SETTINGS = {"a": (None, 0.75, 1.0, 10.0), "b": (1.0, 0.75, 1.0, 1.0), "c": (2.0, 0.5, 2.0, 1.0)}
FAST_G = (1, 2, 4, 8, 16, 32)
GENERIC = ((5, 8, 5), (12, 16, 12), (24, 24, 24), (40, 40, 7), (40, 40, 4), (13, 16, 1), (100, 128, 100))      # (C, Cs, n)
NPIX = 37


def setting(name, n):
    """-> (alpha, beta, k, input scale)"""
    am, beta, k, scale = SETTINGS[name]
    return (1e-4 if am is None else am * n), beta, k, scale


def bf16_round(t):
    return t.float().bfloat16().double()


def ulp_bf16(v):
    a = v.abs().clamp_min(2.0 ** -120)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


# ---- the LRN in float64 --------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Mut:
    """a deliberately wrong LRN (test_elementwise_cpu.py: the bounds catch each of them)"""
    shift: int = 0                 # both windows moved by `shift` channels
    swap: bool = False             # forward and adjoint windows exchanged
    half: bool = False             # n/2 taken as (n-1)/2
    beta_scale: float = 1.0
    aon_is_alpha: bool = False     # alpha / n taken as alpha


EXACT = Mut()
MUTATIONS = {"shift": Mut(shift=1), "swap": Mut(swap=True), "half": Mut(half=True), "beta": Mut(beta_scale=1.01),
             "aon": Mut(aon_is_alpha=True)}


def mutation_is_identity(name, n):
    """odd n: n/2 == (n-1)/2, the two windows coincide; n == 1: alpha / n == alpha"""
    return (name in ("swap", "half") and n % 2 == 1) or (name == "aon" and n == 1)


def windows(C, n, adjoint=False, mut=EXACT):
    """-> (lo, hi): the window of channel c is [lo[c], hi[c]) after clipping to [0, C)"""
    c = torch.arange(C)
    before, after = n // 2, (n - 1) // 2
    if mut.half:
        before = after
    if adjoint != mut.swap:
        before, after = after, before
    s = -mut.shift if adjoint else mut.shift               # (the adjoint of a window moved up is moved down)
    return (c - before + s).clamp(0, C), (c + after + 1 + s).clamp(0, C)


def window_sum(v, lo, hi):
    cs = torch.cumsum(v, -1)
    cs = torch.cat([torch.zeros_like(cs[..., :1]), cs], -1)
    return cs[..., hi] - cs[..., lo]


def lrn_d(x, n, alpha, k, mut=EXACT):
    lo, hi = windows(x.shape[-1], n, False, mut)
    return k + (alpha if mut.aon_is_alpha else alpha / n) * window_sum(x * x, lo, hi)


def lrn_fwd(x, n, alpha, beta, k, mut=EXACT):
    return x * lrn_d(x, n, alpha, k, mut) ** (-beta * mut.beta_scale)


def lrn_bwd(x, dy, n, alpha, beta, k, mut=EXACT):
    d = lrn_d(x, n, alpha, k, mut)
    b = beta * mut.beta_scale
    lo, hi = windows(x.shape[-1], n, True, mut)
    adj = window_sum(dy * x * d ** (-b - 1), lo, hi)
    return dy * d ** -b - 2 * b * (alpha if mut.aon_is_alpha else alpha / n) * x * adj


def lrn_bwd_ref(a, dy, n=None, alpha=1e-4, beta=0.75, k=1.0, dim=1):
    """-> (da, sum of |terms|) with the channels in dimension `dim`: da_c = dy_c d_c^-b - a_c (2 alpha b / n) sum_{c' : c in
    window(c')} dy_c' a_c' d_c'^(-b-1).  The fast kernels take the window sums as differences of fp32 prefix sums over ALL channels,
    so the terms of the bound are those of the whole sum."""
    a, dy = a.movedim(dim, -1), dy.movedim(dim, -1)
    n = a.shape[-1] if n is None else n
    d = lrn_d(a, n, alpha, k)
    t1 = dy.abs() * d ** -beta
    t2 = a.abs() * (2 * alpha * beta / n) * (dy.abs() * a.abs() * d ** (-beta - 1)).sum(-1, keepdim=True)
    return lrn_bwd(a, dy, n, alpha, beta, k).movedim(-1, dim), (t1 + t2).movedim(-1, dim)


# ---- the fp32 term of the LRN bounds ---------------------------------------------------------------------------------------------
def c_sum(n, C, fast):
    return 8 + math.log2(C // 8) + 2 if fast else min(n, C)


def _rel_errors(x, d, n, alpha, beta, fast):
    """-> (rho, sigma, cs): the relative errors of the computed d^-beta and 1/d in units of EPS, and c_sum"""
    C = x.shape[-1]
    cs = c_sum(n, C, fast)
    aon = alpha / n
    T = (x * x).sum(-1, keepdim=True).expand_as(x) if fast else window_sum(x * x, *windows(C, n))
    wrel = aon * cs * T / d                                          # the window sum's error, relative to d
    if beta == 0.75:
        c_dnb, c_inv = C_RSQ, (C_INV_RSQ if fast else C_INV_DIV)
    else:
        c_dnb, c_inv = C_EXP + C_ARG * (beta * torch.log(d)).abs(), (C_INV_RCP if fast else C_INV_DIV)
    rho = c_dnb + beta * C_D + beta * wrel
    sigma = c_inv + C_D + wrel
    return rho, sigma, cs


def lrn_fwd_bound(x, n, alpha, beta, k, fast):
    """|computed y - exact y| in fp32 arithmetic:  |y| c_pow EPS + |x| beta d^(-beta-1) (alpha/n) c_sum EPS T"""
    d = lrn_d(x, n, alpha, k)
    rho, _, _ = _rel_errors(x, d, n, alpha, beta, fast)
    return (x * d ** -beta).abs() * (rho + 1) * EPS                  # (+1: the multiply with x)


def lrn_bwd_bound(x, dy, n, alpha, beta, k, fast):
    """the same form for every factor of dy_c d_c^-b - 2 b (alpha/n) x_c sum_j dy_j x_j d_j^(-b-1): the adjoint sum's terms in
    absolute value, over all channels for the fast kernel and over the adjoint window for the generic one"""
    C = x.shape[-1]
    d = lrn_d(x, n, alpha, k)
    rho, sigma, cs = _rel_errors(x, d, n, alpha, beta, fast)
    q = (dy * x).abs() * d ** (-beta - 1)
    qe = q * (rho + sigma + 3 + cs)                                  # dy x [1], d^-b [1], 1/d [1], the sum's additions
    if fast:
        S, Se = q.sum(-1, keepdim=True), qe.sum(-1, keepdim=True)
    else:
        lo, hi = windows(C, n, True)
        S, Se = window_sum(q, lo, hi), window_sum(qe, lo, hi)
    c2x = 2 * beta * (alpha / n) * x.abs()
    # first term: d^-b, its multiply with dy, the final subtraction; second: c2 [1], c2 x [1], its multiply with the sum [1], the
    # final subtraction [1]
    return (dy.abs() * d ** -beta * (rho + 2) + c2x * (Se + 4 * S)) * EPS


# ---- float32 restatements of the two kernel forms (numpy) ----------------------------------------------------------------------
def _pow32(d, beta):
    f = np.float32
    if beta == 0.75:
        r = (f(1) / np.sqrt(d)).astype(f)
        return (r * np.sqrt(r)).astype(f), (r * r).astype(f)
    return np.exp((f(-beta) * np.log(d)).astype(f)).astype(f), (f(1) / d).astype(f)


def _scan32(v):
    """[npix, G, 8] fp32 -> (exclusive prefix of the lane, inclusive prefix, total): a running sum in the lane, a Hillis-Steele
    scan over the G lanes"""
    f = np.float32
    G = v.shape[1]
    P = np.zeros_like(v)
    run = np.zeros(v.shape[:2], f)
    for j in range(8):
        run = (run + v[:, :, j]).astype(f)
        P[:, :, j] = run
    inc = run.copy()
    o = 1
    while o < G:
        nxt = inc.copy()
        nxt[:, o:] = (inc[:, o:] + inc[:, :-o]).astype(f)
        inc = nxt
        o *= 2
    E = (inc - run).astype(f)
    return E, P, inc[:, -1:]


def lrn_fast32(x, dy, alpha, beta, k):
    """the fast kernel's form in float32: [npix, C] float32 with C = n = 8 G -> y (dy None) or da"""
    f = np.float32
    npix, C = x.shape
    G = C // 8
    x = x.astype(f).reshape(npix, G, 8)
    aon, kk = f(f(alpha) / f(C)), f(k)
    lane = np.arange(G)
    low = (lane < G // 2)[None, :, None]

    def wins(v, inclusive):
        if G == 1:
            out = np.zeros_like(v)
            for j in range(8):
                s = np.zeros(npix, f)
                for c in range(8):
                    if (j - 3 <= c <= j + 4) if inclusive else (j - 4 <= c <= j + 3):
                        s = (s + v[:, 0, c]).astype(f)
                out[:, 0, j] = s
            return out
        E, P, tot = _scan32(v)
        if inclusive:
            X = (E[:, :, None] + P).astype(f)
        else:
            Pm = np.concatenate([np.zeros_like(P[:, :, :1]), P[:, :, :-1]], 2)
            X = (E[:, :, None] + Pm).astype(f)
        Xo = X[:, lane ^ (G // 2), :]
        return np.where(low, Xo, (tot[:, :, None] - Xo).astype(f))
    d = (kk + (aon * wins((x * x).astype(f), False)).astype(f)).astype(f)
    dnb, invd = _pow32(d, beta)
    if dy is None:
        return (x * dnb).astype(f).reshape(npix, C)
    g = dy.astype(f).reshape(npix, G, 8)
    q = ((((g * x).astype(f) * dnb).astype(f)) * invd).astype(f)
    adj = wins(q, True)
    c2 = f(f(2 * beta) * aon)
    return ((g * dnb).astype(f) - (((c2 * x).astype(f)) * adj).astype(f)).astype(f).reshape(npix, C)


def lrn_generic32(x, dy, n, alpha, beta, k):
    """the generic kernel's form in float32: direct sums over the windows, in channel order"""
    f = np.float32
    npix, C = x.shape
    x = x.astype(f)
    aon = f(f(alpha) / f(n))
    d = np.zeros_like(x)
    for c in range(C):
        s = np.zeros(npix, f)
        for cc in range(max(0, c - n // 2), min(C, c + (n - 1) // 2 + 1)):
            s = (s + (x[:, cc] * x[:, cc]).astype(f)).astype(f)
        d[:, c] = (f(k) + (aon * s).astype(f)).astype(f)
    dnb, _ = _pow32(d, beta)
    if dy is None:
        return (x * dnb).astype(f)
    g = dy.astype(f)
    q = ((((g * x).astype(f) * dnb).astype(f)) / d).astype(f)
    out = np.zeros_like(x)
    c2 = f(f(2 * beta) * aon)
    for c in range(C):
        s = np.zeros(npix, f)
        for cc in range(max(0, c - (n - 1) // 2), min(C, c + n // 2 + 1)):
            s = (s + q[:, cc]).astype(f)
        out[:, c] = ((g[:, c] * dnb[:, c]).astype(f) - ((c2 * x[:, c]).astype(f) * s).astype(f)).astype(f)
    return out


# ---- LRN inputs ------------------------------------------------------------------------------------------------------------------
def lrn_inputs(npix, C, scale, seed):
    """-> (x, dy) float64, bf16-exact: both storage types read the same numbers"""
    g = torch.Generator().manual_seed(seed)
    return bf16_round(scale * torch.randn(npix, C, generator=g)), bf16_round(torch.randn(npix, C, generator=g))


def energy_positions(n):
    return (0, n // 2 - 1, n // 2, n - 1)


def energy_inputs(npix, n, seed):
    """all of a pixel's energy in one channel (16: d = 257 where it is in the window, ~1 where it is not), placed in turn where
    the two window formulae change membership; the other channels hold small values so that their outputs show the window.
    -> (x, dy) of 4 * npix pixels"""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for pos in energy_positions(n):
        x = 2.0 ** -4 * torch.randn(npix, n, generator=g)
        x[:, pos] = 16.0 * (1 - 2 * (torch.arange(npix) % 2)).double()
        xs.append(x)
    x = bf16_round(torch.cat(xs))
    return x, bf16_round(torch.randn(x.shape, generator=g))


# ---- 2x2 max pool ----------------------------------------------------------------------------------------------------------------
POOL_HW = ((1, 1), (1, 6), (7, 5), (8, 8), (9, 2))
POOL_CS = (8, 24, 64)
# bf16-exact; ties are certain with so few values, +0 and -0 compare equal
POOL_VALUES = (-3.0, -1.5, -0.25, -0.0, 0.0, 0.25, 0.25, 1.5, 2.0, -1.5)


def pool_input(B, H, W, Cs, seed, negative=False):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([v for v in POOL_VALUES if v < 0] if negative else POOL_VALUES, dtype=torch.float32)
    return vals[torch.randint(len(vals), (B, H, W, Cs), generator=g)]


def pool_windows(x):
    """[B, H, W, C] -> [4, B, Ho, Wo, C]: the zero-padded windows, positions in row-major order"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    p = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=x.dtype)
    p[:, :H, :W] = x
    return torch.stack([p[:, pos // 2::2, pos % 2::2] for pos in range(4)])


def pool_fwd(x):
    """-> (y, idx): the first maximum in row-major order of the zero-padded window; y keeps the bits of the selected element"""
    v = pool_windows(x)
    best, idx = v[0].clone(), torch.zeros(v[0].shape, dtype=torch.uint8)
    for pos in range(1, 4):
        up = v[pos] > best
        best = torch.where(up, v[pos], best)
        idx = torch.where(up, torch.full_like(idx, pos), idx)
    return best, idx


def pool_scatter(g, idx, H, W):
    """[B, Ho, Wo, C] -> [B, H, W, C]: g where idx names the position, 0 elsewhere; positions in the padding are dropped"""
    B, Ho, Wo, C = g.shape
    full = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=g.dtype)
    for pos in range(4):
        full[:, pos // 2::2, pos % 2::2] = torch.where(idx == pos, g, torch.zeros_like(g))
    return full[:, :H, :W].contiguous()


def extent_mask(B, H, W, extent):
    """-> [B, H, W] bool: inside the sample's (h, w)"""
    e = torch.as_tensor(extent).reshape(B, 2)
    yy, xx = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    return (yy < e[:, 0].view(B, 1, 1)) & (xx < e[:, 1].view(B, 1, 1))


def pool_bwd(g, idx, old, mask, elu, extent, H, W):
    """The kernel's documented order in the dtype of `g`: (old + g at the named position), then the mask factor (ReLU output: 0
    where not mask > 0; ELU output: times mask + 1 there), then 0 outside the extent.  -> (dx, slack): `slack` is 2^-23 times the
    magnitude of each fp32 sum or product, for bf16 storage (in fp32 storage the same operations give the same bits)."""
    v = pool_scatter(g, idx, H, W)
    if old is not None:
        v = old + v
    slack = 2.0 ** -23 * v.abs()
    if mask is not None:
        off = ~(mask > 0)
        if elu:
            f = mask + 1
            slack = torch.where(off, 3 * slack * f.abs(), slack)
            v = torch.where(off, v * f, v)
        else:
            v = torch.where(off, torch.zeros_like(v), v)
            slack = torch.where(off, torch.zeros_like(slack), slack)
    if extent is not None:
        inside = extent_mask(v.shape[0], H, W, extent).unsqueeze(-1)
        v = torch.where(inside, v, torch.zeros_like(v))
        slack = torch.where(inside, slack, torch.zeros_like(slack))
    return v, slack


def pool_extents(B, H, W):
    """(0, 0), the full image and odd sizes inside it, in turn"""
    some = [(0, 0), (H, W), (min(H, (H // 2) | 1), min(W, (W // 2) | 1)), (H, min(W, 1)), (min(H, 1), W)]
    return torch.tensor([some[b % len(some)] for b in range(B)], dtype=torch.int32)


# ---- layout ----------------------------------------------------------------------------------------------------------------------
LAYOUT_CCS = ((13, 16), (64, 64), (100, 128), (5, 8))
LAYOUT_HW = ((1, 1), (5, 6), (7, 11))                 # HW = 1, 30, 77


def nhwc_to_nchw(src, C):
    """[B, HW, Cs] -> [B, C, HW]"""
    return src[..., :C].transpose(1, 2).contiguous()


def nchw_grad_to_nhwc(src, old, Cs):
    """[B, C, HW] (+ old [B, HW, Cs], its padded channels ignored) -> [B, HW, Cs] with zero padded channels"""
    B, C, HW = src.shape
    out = torch.zeros(B, HW, Cs, dtype=src.dtype)
    out[..., :C] = src.transpose(1, 2)
    if old is not None:
        out[..., :C] += old[..., :C]
    return out


# ---- extent copy, one-hot ids ----------------------------------------------------------------------------------------------------
SPECIAL_WORDS = (0x7FC00000, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001, 0xFFFFFFFF, 0x7FC07FC0, 0x80008000)


def extent_words(B, planes, H, W, words, seed):
    """int32 [B, planes, H, W, words]: random bit patterns with NaNs, infinities and -0.0 (fp32 and paired bf16) among them"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31, (B, planes, H, W, words), generator=g, dtype=torch.int64)
    sp = torch.tensor(SPECIAL_WORDS, dtype=torch.int64)
    sp = torch.where(sp >= 2 ** 31, sp - 2 ** 32, sp)
    pick = torch.randint(0, 3 * len(sp), w.shape, generator=g)
    w = torch.where(pick < len(sp), sp[pick.clamp_max(len(sp) - 1)], w)
    return w.to(torch.int32)


def extent_copy(words, extent):
    B, planes, H, W, _ = words.shape
    inside = extent_mask(B, H, W, extent).view(B, 1, H, W, 1)
    return torch.where(inside, words, torch.zeros_like(words))


def extent_cases(H, W):
    """(0, 0), the full image, (h, W), (H, w) and an interior one"""
    h, w = max(1, H // 2), max(1, W // 2)
    return ((0, 0), (H, W), (h, W), (H, w), (h, w))


def onehot_ids(B, H, W, C, Cs, seed):
    """int32 [B, H, W]: valid ids with -1, C - 1, C, Cs - 1 and large values of both signs among them"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64)
    sp = torch.tensor([-1, C - 1, C, Cs - 1, 2 ** 31 - 1, -2 ** 31, 0, Cs, 2 ** 16 + 1])
    pick = torch.randint(0, 2 * len(sp), ids.shape, generator=g)
    return torch.where(pick < len(sp), sp[pick.clamp_max(len(sp) - 1)], ids).to(torch.int32)


def onehot(ids, C, Cs, extent=None):
    """-> [B, H, W, Cs] float32: 1 at channel id where 0 <= id < C (and the pixel is inside the extent), 0 elsewhere"""
    B, H, W = ids.shape
    ok = (ids >= 0) & (ids < C)
    if extent is not None:
        ok &= extent_mask(B, H, W, extent)
    out = torch.zeros(B, H, W, Cs, dtype=torch.float32)
    out.scatter_(3, ids.long().clamp(0, Cs - 1).unsqueeze(-1), ok.float().unsqueeze(-1))
    return out


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, slack, bf16, mag=None):
    """-> max over the elements of |got - ref| / tolerance: fp32 storage, the fp32 term alone; bf16 storage, half a bf16 ulp of
    the larger of |got|, |ref| (and `mag`) on top of it -- the tolerance of test_launch_ulp_gpu.assert_rounded"""
    tol = slack + 1e-30
    if bf16:
        big = torch.maximum(got.abs(), ref.abs())
        if mag is not None:
            big = torch.maximum(big, mag)
        tol = tol + 0.5 * ulp_bf16(big) * (1 + 1e-6)
    return float(((got - ref).abs() / tol).max())
