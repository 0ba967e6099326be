"""Weight gradients (msau_conv2d_wgrad, msau_wgrad_reduce, msau_channel_sum): a float64 reference written from the definition,
the bounds the GPU tests hold the kernels to, input generators and the descriptor / route plumbing.  Nothing here goes through the
product's own helpers (plan.py, the oracle): tests/test_wgrad_cpu.py checks this file against autograd, tests/test_wgrad_gpu.py
checks the kernels against this file.

The slab a launch writes (include/msau_hip.h): [nslabs][nchunks][Cout][kext] fp32; per chunk of cch input channels column
tap * cch + c holds

    dW[co][chunk][tap][c] = sum_{b,oy,ox} g[b,oy,ox,co] * x~[b, oy*stride - pad_t + ky*dil, ox*stride - pad_l + kx*dil, chunk*cch + c]

(tap = ky * KW + kx; zero outside the image; x~ = relu(x) under MSAU_CONV_RELU_IN; x~ = x1 | x2 concatenated; under MSAU_CONV_IDS the
one-hot expansion of the id map, ids outside [0, 64) empty), column taps * cch holds sum g[..., co] in every chunk, the columns up to
kext are padding.

Bounds.  Integer inputs (values in [-2, 2], a third of them zero, exact in bf16 and fp32): every product and every partial sum in
any order is an integer below 2^24, so fp32 sums are exact whatever their order -- the sum of the slabs must EQUAL the reference.
Random inputs (0.5 * randn rounded to the storage type): |sum of slabs - exact| <= 2e-5 * S + 1e-12 per element, S = the sum of the
magnitudes of the terms (the same reference on |g|, |x~|).  2e-5 is the bound tests/test_launch_ulp_gpu.py holds every plan's weight
gradients to at 1.4 M terms; test_wgrad_cpu.py shows that fp32 sums of these terms in shuffled and slab-split orders use less than
half of it.
"""
import ctypes as C
import dataclasses

import numpy as np
import torch

from msau_amd import _lib as L

REL, ABS = 2e-5, 1e-12
GUARD = 1024                       # floats behind the last slab that no launch may touch
TILE, REFUSED, GENERIC, LEAN, SPECIAL, IN64, IN64_IDS, ROWS, OWNER = 16, 0, 1, 2, 3, 4, 5, 6, 7
FAMILY = {REFUSED: "refused", GENERIC: "generic", LEAN: "lean", SPECIAL: "special", IN64: "in64", IN64_IDS: "in64-ids", ROWS: "rows",
          OWNER: "owner"}
TNAME = {L.F32: "f32", L.BF16: "bf16"}
# WGRAD_TILE_TABLE of csrc/conv_wgrad.hip: the instantiations of wgrad_kernel<T, CTN, NKW>, per type (fp32 slices are 64 channels wide: CTN <= 4)
TILE_TABLE = {L.F32: [(ctn, nkw) for ctn in (1, 2, 4) for nkw in (1, 2, 3, 5, 10)]}
TILE_TABLE[L.BF16] = TILE_TABLE[L.F32] + [(8, nkw) for nkw in (1, 2, 3, 5)]
# WLEAN_TABLE of csrc/wgrad_lean.hip: (family, cch / 8, Cout / 8, k, dil, stride), per type
_LEAN_BOTH = [(LEAN, c8, co8, k, 1, 1) for k in (1, 3) for c8, co8 in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4), (8, 1), (4, 8), (8, 4))] + \
             [(LEAN, 8, 8, 1, 1, 1), (LEAN, 1, 1, 4, 1, 1), (SPECIAL, 1, 2, 3, 2, 1), (SPECIAL, 2, 4, 3, 4, 1), (SPECIAL, 1, 2, 3, 1, 2), (SPECIAL, 2, 4, 3, 1, 2)]
LEAN_TABLE = {L.F32: _LEAN_BOTH,
              L.BF16: _LEAN_BOTH + [(LEAN, 8, 8, 3, 1, 1), (SPECIAL, 4, 8, 3, 8, 1), (SPECIAL, 4, 8, 3, 1, 2), (IN64, 8, 1, 3, 1, 1)]}


def torch_dtype(dtype):
    return torch.float32 if dtype == L.F32 else torch.bfloat16


@dataclasses.dataclass(frozen=True)
class Case:
    """one descriptor of msau_conv2d_wgrad and what the test expects of it"""
    name: str
    dtype: int
    family: int
    C1: int
    Cout: int
    k: int
    C2: int = 0
    dil: int = 1
    stride: int = 1
    pad: tuple = None              # (pad_t, pad_l); None: centred -- dil * (k - 1) // 2, stride 2: k // 2
    B: int = 2
    hw: tuple = (19, 35)           # Hout, Wout: 2 x 3 tiles, partial in both directions
    hw_in: tuple = None            # None: hw (stride 1), 2 * hw (stride 2)
    flags: int = 0
    nslabs: tuple = (1, 5, 12)     # one workgroup walks everything; a count that does not divide the tiles; one tile each
    env: tuple = ()                # MSAU_* switches the case needs, ((name, value), ...)
    tup: tuple = None              # generic kernel: (CTN, NKW, compact, sliced) the case was chosen for

    @property
    def pads(self):
        if self.pad is not None:
            return self.pad
        p = self.k // 2 if self.stride == 2 else self.dil * (self.k - 1) // 2
        return (p, p)

    @property
    def in_hw(self):
        return self.hw_in or (self.hw if self.stride == 1 else (2 * self.hw[0], 2 * self.hw[1]))

    @property
    def ntiles(self):
        return self.B * -(-self.hw[0] // TILE) * -(-self.hw[1] // TILE)

    @property
    def id(self):
        return f"{TNAME[self.dtype]}-{self.name}"


def descriptor(c: Case, nslabs=1, x1=None, x2=None, g=None, slabs=None):
    d = L.WgradDesc()
    d.B, (d.Hin, d.Win), (d.Hout, d.Wout) = c.B, c.in_hw, c.hw
    d.C1, d.C2, d.Cout, d.KH, d.KW = c.C1, c.C2, c.Cout, c.k, c.k
    d.dil, (d.pad_t, d.pad_l), d.stride, d.flags = c.dil, c.pads, c.stride, c.flags
    d.x1, d.x2, d.g, d.slabs, d.nslabs = x1, x2, g, slabs, nslabs
    return d


def route(dtype, d):
    """(status, info[8]) of msau_wgrad_route"""
    info = (C.c_int32 * 8)()
    rc = L.load().msau_wgrad_route(dtype, C.byref(d), info)
    return rc, list(info)


def route_tuple(dtype, info):
    """what the coverage is counted in: (dtype, family, CTN, NKW, compact, more than one slice)"""
    return (dtype, info[0], info[1], info[2], info[3], int(info[4] > 1))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
_INT_VALUES = torch.tensor([-2.0, -1.0, 0.0, 0.0, 1.0, 2.0])


def draw(kind, shape, gen, dtype):
    """'int': integers in [-2, 2], a third of them zero; 'rand': 0.5 * randn; both rounded to the storage type"""
    if kind == "int":
        v = _INT_VALUES[torch.randint(0, 6, shape, generator=gen)]
    else:
        v = 0.5 * torch.randn(shape, generator=gen)
    return v.to(torch_dtype(dtype))


def make_inputs(c: Case, kind, seed=0):
    """{x1, x2 | None, g} in the storage type (NHWC, on the CPU); under MSAU_CONV_IDS x1 is the int32 id map, with -1, 64 and an
    all-empty first sample in it"""
    gen = torch.Generator().manual_seed(1000 * seed + (7 if kind == "int" else 11))
    (Hi, Wi), (Ho, Wo) = c.in_hw, c.hw
    if c.flags & L.CONV_IDS:
        ids = torch.randint(-1, 65, (c.B, Hi, Wi), generator=gen, dtype=torch.int32)
        ids[0] = -1
        ids[-1].view(-1)[:2] = torch.tensor([-1, 64], dtype=torch.int32)
        x1 = ids
    else:
        x1 = draw(kind, (c.B, Hi, Wi, c.C1), gen, c.dtype)
    x2 = draw(kind, (c.B, Hi, Wi, c.C2), gen, c.dtype) if c.C2 else None
    return {"x1": x1, "x2": x2, "g": draw(kind, (c.B, Ho, Wo, c.Cout), gen, c.dtype)}


def onehot(ids):
    """[B][H][W] int ids -> [B][H][W][64] float64, ids outside [0, 64) empty"""
    return (ids.long()[..., None] == torch.arange(64, device=ids.device)).double()


def x_tilde(c: Case, x1, x2):
    """the tensor the weight gradient is taken against, float64"""
    x = onehot(x1) if c.flags & L.CONV_IDS else x1.double()
    if x2 is not None:
        x = torch.cat([x, x2.double()], dim=-1)
    return torch.relu(x) if c.flags & L.CONV_RELU_IN else x


# ---- the reference ---------------------------------------------------------------------------------------------------------
def shifted(c: Case, x, ky, kx):
    """x[b, oy*stride - pad_t + ky*dil, ox*stride - pad_l + kx*dil, :] for every output pixel, zero outside the image"""
    (Hi, Wi), (Ho, Wo), (pt, pl) = c.in_hw, c.hw, c.pads
    iy = torch.arange(Ho, device=x.device) * c.stride - pt + ky * c.dil
    ix = torch.arange(Wo, device=x.device) * c.stride - pl + kx * c.dil
    oky, okx = (iy >= 0) & (iy < Hi), (ix >= 0) & (ix < Wi)
    xs = x[:, iy.clamp(0, Hi - 1)][:, :, ix.clamp(0, Wi - 1)]
    return xs * (oky[:, None] & okx[None, :])[None, :, :, None].to(x.dtype)


def reference(c: Case, xt, g, cch, nchunks, kext):
    """float64 slab [nchunks][Cout][kext] of the whole launch and the mask [kext] of its real columns (the rest is padding).
    xt = x_tilde(), g float64.  Called with |xt|, |g| it gives S, the sum of the magnitudes of the terms."""
    taps = c.k * c.k
    assert xt.shape[-1] == cch * nchunks == c.C1 + c.C2 and kext >= taps * cch + 1
    ref = torch.zeros(nchunks, c.Cout, kext, dtype=torch.float64, device=g.device)
    gm = g.reshape(-1, c.Cout)
    for ky in range(c.k):
        for kx in range(c.k):
            dw = gm.T @ shifted(c, xt, ky, kx).reshape(-1, xt.shape[-1])            # [Cout][Cin]: the sum over the pixels
            tap = ky * c.k + kx
            ref[:, :, tap * cch:(tap + 1) * cch] = dw.view(c.Cout, nchunks, cch).permute(1, 0, 2)
    ref[:, :, taps * cch] = gm.sum(0)[None, :]
    mask = torch.zeros(kext, dtype=torch.bool, device=g.device)
    mask[:taps * cch + 1] = True
    return ref, mask


def terms(c: Case, xt, g, elems, cch):
    """the terms of slab elements (chunk, co, column) one by one: float64 [B * Hout * Wout][len(elems)], pixels in (b, oy, ox) order"""
    taps, cols = c.k * c.k, []
    for chunk, co, col in elems:
        if col == taps * cch:
            cols.append(g[..., co].reshape(-1))
        else:
            tap, ch = col // cch, chunk * cch + col % cch
            cols.append((g[..., co] * shifted(c, xt, tap // c.k, tap % c.k)[..., ch]).reshape(-1))
    return torch.stack(cols, dim=1)


def slab_of_pixel(c: Case, nslabs):
    """the slab that takes each output pixel, (b, oy, ox) order: 16 x 16 tiles numbered x fastest, tile t -> workgroup t % nslabs"""
    Ho, Wo = c.hw
    ty, tx = -(-Ho // TILE), -(-Wo // TILE)
    b, oy, ox = np.meshgrid(np.arange(c.B), np.arange(Ho), np.arange(Wo), indexing="ij")
    return (((b * ty + oy // TILE) * tx + ox // TILE) % nslabs).reshape(-1)


def fp32_orders(t64, slab_ids, nslabs, seed=0):
    """fp32 sums of the columns of t64 (float64 terms, exactly representable products are NOT assumed: each term is rounded to
    fp32 first, as a kernel's fp32 accumulator sees it at best) in three shuffled orders and split into nslabs partial sums that
    are then added slab by slab: [4][n] float64"""
    t = np.asarray(t64, dtype=np.float64).astype(np.float32)
    rng = np.random.default_rng(seed)
    out = [np.add.accumulate(t[rng.permutation(len(t))], axis=0, dtype=np.float32)[-1] for _ in range(3)]
    parts = np.zeros((nslabs, t.shape[1]), dtype=np.float32)
    for s in range(nslabs):
        rows = t[slab_ids == s]
        if len(rows):
            parts[s] = np.add.accumulate(rows, axis=0, dtype=np.float32)[-1]
    out.append(np.add.accumulate(parts, axis=0, dtype=np.float32)[-1])
    return np.stack(out).astype(np.float64)


# ---- what a launch must leave behind -----------------------------------------------------------------------------------------
def slab_buffer(nslabs, slab_elems, device):
    """NaN everywhere, GUARD floats behind the slabs"""
    return torch.full((nslabs * slab_elems + GUARD,), float("nan"), dtype=torch.float32, device=device)


def check_slabs(buf, nslabs, ref, S, mask, kind, what):
    """sentinels, then the sum of the slabs against the reference: bit-exact ('int') or within REL * S + ABS ('rand').
    Returns the worst error / bound."""
    nchunks, cout, kext = ref.shape
    n = nslabs * nchunks * cout * kext
    slabs = buf[:n].view(nslabs, nchunks, cout, kext)
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: the guard band behind the slabs was written"
    real, pad = slabs[..., mask], slabs[..., ~mask]
    bad = ~torch.isfinite(real)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} real slab elements not written or not finite, first (slab, chunk, co, k) " \
                                f"{tuple(bad.nonzero()[0].tolist())} (an idle workgroup writes zeros)"
    assert bool((torch.isnan(pad) | (pad == 0)).all()), f"{what}: a padding column holds something other than 0"
    tot = real.double().sum(0)
    want, s = ref[..., mask], S[..., mask]
    err = (tot - want).abs()
    if kind == "int":
        assert float(S.max()) < 2 ** 24, f"{what}: the integer inputs are not exact in fp32"
        bound = torch.zeros_like(s)
    else:
        bound = REL * s + ABS
    over = err > bound
    if bool(over.any()):
        idx = np.unravel_index(int(((err - bound) * over).flatten().argmax()), tuple(err.shape))
        raise AssertionError(f"{what}: {int(over.sum())} of {over.numel()} elements off, worst (chunk, co, k) {tuple(int(v) for v in idx)}: "
                             f"got {float(tot[idx]):.9g} want {float(want[idx]):.9g} bound {float(bound[idx]):.3g}; "
                             f"chunks {sorted(set(over.nonzero()[:, 0].tolist()))} rows {sorted(set(over.nonzero()[:, 1].tolist()))[:8]} "
                             f"columns {sorted(set(over.nonzero()[:, 2].tolist()))[:8]}")
    return float((err / (REL * s + ABS)).max())


# ---- the route sweep (tests/test_wgrad_cpu.py: coverage; tests/test_wgrad_gpu.py: representatives of the generic kernel) ------
def sweep(cins, couts, ks, dils, strides, dtypes=(L.F32, L.BF16), hw=(33, 61), split=True):
    """msau_wgrad_route over the grid; per row the geometries 'same' (Hin = Hout, centred pad; stride 2: Hin = 2 Hout) and, at
    stride 1, 'valid' (Hin = Hout + (k - 1) dil, no pad: lean-shaped channel counts land on the generic kernel).  Yields
    (Case, status, info)."""
    for cin in cins:
        splits = [(cin, 0)]
        if split and cin >= 16:
            splits.append((cin - 8, 8))
            if cin % 16 == 0:
                splits.append((cin // 2, cin // 2))
        for (c1, c2) in splits:
            for cout in couts:
                for k in ks:
                    for dil in dils:
                        for stride in strides:
                            for geo in (("same", "valid") if stride == 1 and k > 1 else ("same",)):
                                hw_in = (hw[0] + (k - 1) * dil, hw[1] + (k - 1) * dil) if geo == "valid" else None
                                for dtype in dtypes:
                                    c = Case(f"{c1}+{c2}to{cout}-k{k}-d{dil}-s{stride}-{geo}", dtype, -1, c1, cout, k, C2=c2, dil=dil,
                                             stride=stride, pad=(0, 0) if geo == "valid" else None, hw=hw, hw_in=hw_in)
                                    rc, info = route(dtype, descriptor(c))
                                    yield c, rc, info
