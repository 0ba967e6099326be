"""CPU: what tests/test_wgrad_gpu.py rests on.  The float64 reference of tests/wgrad_util.py against float64 autograd (F.conv2d, and
the transposed conv of oracle/msau_oracle.py with the roles swapped as plan.py builds the descriptor); the 2e-5 bound against fp32
sums of the very terms of every random GPU case in shuffled and slab-split orders; msau_wgrad_route swept over the descriptors the
nets can produce -- the GPU case table must hold a case for everything the sweep reaches -- and msau_wgrad_geometry /
msau_conv2d_wgrad_groupable / the refusals of msau_conv2d_wgrad against the route."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from oracle import msau_oracle as O
from tests import wgrad_util as U
from tests.wgrad_util import Case
from tests import test_wgrad_gpu as G

F64 = torch.float64
CINS = list(range(8, 129, 8)) + [192, 768]
COUTS = list(range(8, 137, 8)) + [192, 256]
KS, DILS, STRIDES = (1, 3, 4, 5, 7), (1, 2, 4, 8, 16, 32), (1, 2)
# every instantiation of wgrad_kernel<T, CTN, NKW> (WGRAD_TILE_TABLE in csrc/conv_wgrad.hip), per type
INSTANTIATED = U.TILE_TABLE


@pytest.fixture
def wenv(monkeypatch):
    lib = L.load()

    names = set()

    def set_env(pairs):
        for k in names:
            monkeypatch.delenv(k, raising=False)
        for k, v in pairs:
            monkeypatch.setenv(k, v)
            names.add(k)
        lib.msau_reload_env()
    yield set_env
    monkeypatch.undo()
    lib.msau_reload_env()


# ---- the reference against autograd ------------------------------------------------------------------------------------------
def _conv_cases():
    for k, dil, stride in itertools.product((1, 3, 4), (1, 2, 16), (1, 2)):
        hw = (6, 9) if dil < 16 else (20, 37)
        pads = list(itertools.product(range(k), range(k))) if dil == 1 else [(0, 0), (dil * (k - 1) // 2,) * 2, (dil, 0)]
        for pad in pads:
            for flags in (0, L.CONV_RELU_IN):
                if flags and pad[0] == pad[1] and k > 1:
                    continue
                hin = tuple(stride * s - (1 if flags else 0) for s in hw)                # (odd input sizes under stride 2 ride along)
                yield Case(f"k{k}d{dil}s{stride}p{pad}f{flags}", L.F32, -1, 8, 8, k, C2=8, dil=dil, stride=stride, pad=pad, hw=hw,
                           hw_in=hin if stride == 2 else None, flags=flags)


@pytest.mark.parametrize("c", list(_conv_cases()), ids=lambda c: c.name)
def test_reference_is_autograd_of_conv2d(c):
    gen = torch.Generator().manual_seed(1)
    (Hi, Wi), (Ho, Wo), (pt, pl) = c.in_hw, c.hw, c.pads
    x1, x2 = (torch.randn(c.B, Hi, Wi, 8, generator=gen, dtype=F64) for _ in range(2))
    g = torch.randn(c.B, Ho, Wo, c.Cout, generator=gen, dtype=F64)
    cch, nchunks, kext = 8, 2, -(-(c.k * c.k * 8 + 8) // 16) * 16
    ref, mask = U.reference(c, U.x_tilde(c, x1, x2), g, cch, nchunks, kext)
    # autograd: the same conv on an explicitly padded (or cropped) input
    xin = torch.cat([x1, x2], -1).permute(0, 3, 1, 2)
    if c.flags & L.CONV_RELU_IN:
        xin = torch.relu(xin)
    pb = (Ho - 1) * c.stride + c.dil * (c.k - 1) + 1 - Hi - pt
    pr = (Wo - 1) * c.stride + c.dil * (c.k - 1) + 1 - Wi - pl
    w = torch.zeros(c.Cout, 16, c.k, c.k, dtype=F64, requires_grad=True)
    b = torch.zeros(c.Cout, dtype=F64, requires_grad=True)
    y = F.conv2d(F.pad(xin, (pl, pr, pt, pb)), w, b, stride=c.stride, dilation=c.dil)
    assert y.shape[2:] == (Ho, Wo)
    y.backward(g.permute(0, 3, 1, 2))
    taps = c.k * c.k
    got = ref[:, :, :taps * cch].view(nchunks, c.Cout, taps, cch).permute(1, 0, 3, 2).reshape(c.Cout, 16, c.k, c.k)
    assert float((got - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max() + 1)
    for chunk in range(nchunks):
        assert float((ref[chunk, :, taps * cch] - b.grad).abs().max()) <= 1e-12 * float(b.grad.abs().max())
    assert int(mask.sum()) == taps * cch + 1 and float(ref[..., ~mask].abs().max()) == 0.0


@pytest.mark.parametrize("odd", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_reference_is_autograd_of_the_transposed_conv_with_roles_swapped(odd):
    """plan.py: the weight gradient of ConvTranspose2d is the stride-2 weight gradient with x1 = the gradient of its OUTPUT, g = its
    INPUT; slab rows = its input channels (dim 0 of the IOHW weight)"""
    gen = torch.Generator().manual_seed(2)
    B, Ci, Co, h, w_ = 2, 16, 8, 5, 7
    out_hw = (2 * h - odd[0], 2 * w_ - odd[1])
    x = torch.randn(B, Ci, h, w_, generator=gen, dtype=F64)
    dy = torch.randn(B, Co, *out_hw, generator=gen, dtype=F64)
    w = torch.randn(Ci, Co, 3, 3, generator=gen, dtype=F64).requires_grad_(True)
    O.deconv(x, w, torch.zeros(Co, dtype=F64), out_hw).backward(dy)
    c = Case("deconv", L.F32, -1, Co, Ci, 3, stride=2, B=B, hw=(h, w_), hw_in=out_hw)
    assert c.pads == (1, 1)
    ref, _ = U.reference(c, dy.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), Co, 1, 80)
    got = ref[0, :, :72].view(Ci, 3, 3, Co).permute(0, 3, 1, 2)
    assert float((got - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())


def test_reference_of_an_id_map_is_the_reference_of_its_one_hot_expansion():
    c = Case("ids", L.BF16, U.IN64_IDS, 64, 8, 3, flags=L.CONV_IDS)
    ins = U.make_inputs(c, "rand")
    ids = ins["x1"]
    assert ids.dtype == torch.int32 and int(ids.min()) == -1 and int(ids.max()) == 64 and bool((ids[0] == -1).all())
    xt = U.x_tilde(c, ids, None)
    assert xt.shape[-1] == 64 and bool((xt.sum(-1) == ((ids >= 0) & (ids < 64)).double()).all())
    hot = xt.argmax(-1)[(ids >= 0) & (ids < 64)]
    assert torch.equal(hot, ids[(ids >= 0) & (ids < 64)].long())


# ---- the bounds without a GPU ---------------------------------------------------------------------------------------------------
ALL = G.CASES + G.GROUPED
NSAMPLE = 24                       # slab elements per case whose terms are summed one by one (the ones column among them)


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_fp32_sums_of_the_random_terms_use_half_of_the_bound(c):
    """three shuffled orders and the split into nslabs partial sums by 16 x 16 tiles, for NSAMPLE elements of every random case"""
    rc, info = U.route(c.dtype, U.descriptor(c))
    cch, nchunks = info[5], info[6]
    ins = U.make_inputs(c, "rand")
    xt, g = U.x_tilde(c, ins["x1"], ins["x2"]), ins["g"].double()
    rng = np.random.default_rng(5)
    taps = c.k * c.k
    elems = [(int(rng.integers(nchunks)), int(rng.integers(c.Cout)), int(rng.integers(taps * cch))) for _ in range(NSAMPLE - 2)]
    elems += [(0, 0, taps * cch), (nchunks - 1, c.Cout - 1, taps * cch)]
    t = U.terms(c, xt, g, elems, cch).numpy()
    exact, S = t.sum(0), np.abs(t).sum(0)
    for nslabs in c.nslabs:
        sums = U.fp32_orders(t, U.slab_of_pixel(c, nslabs), nslabs)
        assert (np.abs(sums - exact[None]) <= 0.5 * (U.REL * S + U.ABS)[None]).all(), float((np.abs(sums - exact[None]) / (U.REL * S + U.ABS)).max())


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_integer_inputs_are_exact_in_fp32(c):
    """S = sum of the magnitudes of the terms stays below 2^24: every partial sum of the integer run, in any order, is an fp32 integer;
    and the term-by-term sums agree with the reference at the sampled elements"""
    rc, info = U.route(c.dtype, U.descriptor(c))
    ins = U.make_inputs(c, "int")
    for v in (ins["g"],) + (() if c.flags & L.CONV_IDS else (ins["x1"],)):
        vals, counts = torch.unique(v.double(), return_counts=True)
        assert vals.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0] or v.numel() < 200
        assert 0.25 < float((v == 0).double().mean()) < 0.42 or v.numel() < 2000
    xt, g = U.x_tilde(c, ins["x1"], ins["x2"]), ins["g"].double()
    S, mask = U.reference(c, xt.abs(), g.abs(), info[5], info[6], info[7])
    assert float(S.max()) < 2 ** 24
    ref, _ = U.reference(c, xt, g, info[5], info[6], info[7])
    taps = c.k * c.k
    elems = [(info[6] - 1, c.Cout - 1, taps * info[5] - 1), (0, 0, 0), (info[6] - 1, 1, taps * info[5])]
    t = U.terms(c, xt, g, elems, info[5])
    for j, (chunk, co, col) in enumerate(elems):
        assert float(t[:, j].sum()) == float(ref[chunk, co, col]) and float(t[:, j].abs().sum()) == float(S[chunk, co, col])


# ---- the route: coverage and consistency --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swept():
    """every row of the sweep with its route, msau_wgrad_geometry and msau_conv2d_wgrad_groupable(a, a)"""
    lib = L.load()
    rows = []
    geom = L.WgradGeom()
    for c, rc, info in U.sweep(CINS, COUTS, KS, DILS, STRIDES):
        d = U.descriptor(c)
        grc = lib.msau_wgrad_geometry(c.dtype, C.byref(d), C.byref(geom))
        rows.append((c, rc, info, grc, (geom.lean, geom.cch, geom.nchunks, geom.kext), lib.msau_conv2d_wgrad_groupable(c.dtype, C.byref(d), C.byref(d))))
    return rows


def _shape_key(c, info):
    """a lean-family instance: (dtype, family, k, dil, stride, cch, Cout)"""
    return (c.dtype, info[0], c.k, c.dil, c.stride, info[5], c.Cout)


def test_the_gpu_table_reaches_every_instance_the_route_can_name(swept, wenv):
    reach, shapes = {}, {}
    for c, rc, info, *_ in swept:
        if rc == 0:
            reach.setdefault(U.route_tuple(c.dtype, info), c.name)
            if info[0] in (U.LEAN, U.SPECIAL, U.IN64):
                shapes.setdefault(_shape_key(c, info), c.name)
    assert {k[1] for k in reach} == {U.GENERIC, U.LEAN, U.SPECIAL, U.IN64, U.ROWS}
    have, have_shapes = set(), set()
    for c in G.CASES:
        wenv(c.env)
        rc, info = U.route(c.dtype, U.descriptor(c))
        assert rc == 0 and info[0] == c.family, (c.id, info)
        have.add(U.route_tuple(c.dtype, info))
        have_shapes.add(_shape_key(c, info))
    missing = {k: v for k, v in reach.items() if k not in have}
    assert not missing, f"(dtype, family, CTN, NKW, compact, sliced) the sweep reaches and no GPU case runs: {missing}"
    missing = {k: v for k, v in shapes.items() if k not in have_shapes}
    assert not missing, f"lean instances (dtype, family, k, dil, stride, cch, Cout) the sweep reaches and no GPU case runs: {missing}"
    assert {U.IN64_IDS, U.ROWS} <= {k[1] for k in have}
    # nothing is instantiated that no descriptor of the sweep reaches
    for dtype in (L.F32, L.BF16):
        dead = [p for p in INSTANTIATED[dtype] if not any(k[0] == dtype and k[1] == U.GENERIC and (k[2], k[3]) == p for k in reach)]
        print(f"\nwgrad_kernel<{U.TNAME[dtype]}, CTN, NKW> instantiated and unreachable: {dead}")
        assert dead == []
        assert all((k[2], k[3]) in INSTANTIATED[dtype] for k in reach if k[0] == dtype and k[1] == U.GENERIC)


def test_geometry_and_groupable_take_the_routes_decision(swept):
    n = 0
    for c, rc, info, grc, (lean, cch, nchunks, kext), groupable in swept:
        if info[7] == 0:                                                   # no geometry at all (no chunk fits the LDS)
            assert rc != 0 and grc != 0 and groupable == 0
            continue
        assert grc == 0 and (cch, nchunks, kext) == tuple(info[5:8]), (c.name, info)
        fam = info[0]
        assert lean == (2 if fam == U.ROWS else 1 if fam in (U.LEAN, U.SPECIAL, U.IN64, U.IN64_IDS) else 0), (c.name, info, lean)
        assert groupable == (1 if fam in (U.LEAN, U.SPECIAL) else 0), (c.name, info, groupable)
        assert kext == -(-(c.k * c.k * cch + 8) // 16) * 16 and cch * nchunks == c.C1 + c.C2 and (c.C2 == 0 or c.C1 % cch == 0)
        n += fam != 0
    assert n > 100000


def test_conv2d_wgrad_refuses_what_the_route_refuses_before_any_launch(swept):
    """no device here: a launch would be a HIP error, not the route's status"""
    lib = L.load()
    refused = [(c, rc) for c, rc, info, *_ in swept if rc != 0]
    assert len(refused) > 100
    for c, rc in refused[::max(1, len(refused) // 300)]:
        d = U.descriptor(c, 1, 64, 64, 64, 64)
        assert lib.msau_conv2d_wgrad(None, c.dtype, C.byref(d)) == rc, c.name
    # MSAU_CONV_IDS belongs to the bf16 64 -> 8 3x3 instance with ONE chunk: anything else is refused, lean-shaped or not
    for c in (Case("ids-f32", L.F32, 0, 64, 8, 3, flags=L.CONV_IDS), Case("ids-16to16", L.BF16, 0, 16, 16, 3, flags=L.CONV_IDS),
              Case("ids-128", L.BF16, 0, 128, 8, 3, flags=L.CONV_IDS), Case("ids-k1", L.BF16, 0, 64, 8, 1, flags=L.CONV_IDS),
              Case("ids-24to40", L.BF16, 0, 24, 40, 3, flags=L.CONV_IDS)):
        rc, info = U.route(c.dtype, U.descriptor(c))
        assert rc == -1 and info[0] == 0 and info[4] == 0 and b"MSAU_CONV_IDS" in lib.msau_last_error(), (c.name, info)
        assert lib.msau_conv2d_wgrad(None, c.dtype, C.byref(U.descriptor(c, 1, 64, None, 64, 64))) == -1
    rc, info = U.route(L.BF16, U.descriptor(Case("owner", L.BF16, U.OWNER, 64, 8, 3, flags=L.CONV_OWNER)))
    assert rc == 0 and info[0] == U.OWNER
