"""GPU: every kernel family of the attention core (msau_selfattn_{fwd,bwd}[_ext]) against the float64 reference of
tests/attention_util.py -- ELEMENT BY ELEMENT, every output (statistics, y, dh, delta, dg, df), at the sizes that cross each tiling
edge of its family (the 16 x 32 MFMA step, the 512 / 256-row chunk, the 64-row own block, the 128-row stage, the 256-column
statistics tile, the MFMA / VALU switch), with inputs that make the softmax peaked or shift whole rows to -+128, and with extents.
Every case asserts the family it means to test (msau_selfattn_route), that every output element was written, and that nothing
beside the outputs was.  The bounds and their constants: tests/attention_util.py.

What this found: on the MFMA backward without extents, a swept row j >= N (staged as zeros, score 0) got P = exp2(0 - lse2) in the
own-i sweeps (dh, dg); for a row i whose scores are all below about -89 that is +inf, and inf * 0 in the second product made dh[i],
delta[i], dg[i] and then every df NaN (generator shift_neg, any N that is no multiple of 32).  The sweeps now give those rows P = 0.

Worst error / bound per family and output over all cases of this module (MI355X; `pytest -s` prints them per case and per module):
    family      m       ln Z    m+ln Z  y       dh      delta   dg      df
    f32         0.0042  0.0091  0.0091  0.092   0.13    0.019   0.020   0.031
    bf16_valu   0.0044  0.045   0.045   0.99    0.99    0.019   0.97    0.98      (y, dh, dg, df: the half ulp of the store)
    mfma        0.0028  0.0034  0.0032  0.99    0.93    0.83    0.59    0.61      (delta: against K_DELTA_MFMA, see attention_util)
"""
import pytest
import torch

from msau_amd import _lib as L
from tests import attention_util as AU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 24576.0                  # representable in bf16; no output of these inputs comes near it
GUARD = 2048                        # elements on either side of every output
RATIOS = {}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in ("f32", "bf16_valu", "mfma"):
        if any(k[0] == fam for k in RATIOS):
            print(f"\nworst err/bound {fam:10s}" + " ".join(f"{k}={RATIOS.get((fam, k), 0.0):.3g}" for k in AU.OUTPUTS))


def _guarded(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def _untouched(whole, what):
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), f"{what}: written outside the tensor"


def run_core(dtype, ins, ext=None, W=0):
    """the C ABI on sentinel-filled, guarded outputs -> what the kernels stored (m, Z, y, dh, delta, dg, df)"""
    td = torch.float32 if dtype == L.F32 else torch.bfloat16
    f, g, h, x, dy = (t.to(DEV).to(td).contiguous() for t in ins)
    B, N, D = f.shape
    C = h.shape[-1]
    bufs = {"y": _guarded((B, N, C), td), "df": _guarded((B, N, D), td), "dg": _guarded((B, N, D), td), "dh": _guarded((B, N, C), td),
            "stats": _guarded((B, N, 2), torch.float32), "ws": _guarded((B * N * (C + 4),), torch.float32)}
    p = {k: v[0].data_ptr() for k, v in bufs.items()}
    s = torch.cuda.current_stream().cuda_stream
    if ext is None:
        L.call("msau_selfattn_fwd", s, dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), x.data_ptr(), p["y"], p["stats"], B, N, D, C)
        L.call("msau_selfattn_bwd", s, dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), dy.data_ptr(), p["stats"], p["df"], p["dg"],
               p["dh"], p["ws"], B, N, D, C)
    else:
        e = ext.to(DEV).contiguous()
        L.call("msau_selfattn_fwd_ext", s, dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), x.data_ptr(), p["y"], p["stats"], B, N, D, C,
               e.data_ptr(), W)
        L.call("msau_selfattn_bwd_ext", s, dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), dy.data_ptr(), p["stats"], p["df"], p["dg"],
               p["dh"], p["ws"], B, N, D, C, e.data_ptr(), W)
    torch.cuda.synchronize()
    for k, (view, whole) in bufs.items():
        _untouched(whole, k)
        written = view[:B * N] if k == "ws" else view
        assert bool((written != SENTINEL).all()), f"{k}: {int((written == SENTINEL).sum())} elements never written"
    stats = bufs["stats"][0]
    return {"m": stats[..., 0], "Z": stats[..., 1], "y": bufs["y"][0], "dh": bufs["dh"][0], "delta": bufs["ws"][0][:B * N].view(B, N),
            "dg": bufs["dg"][0], "df": bufs["df"][0]}


def _reference(gen, B, N, D, C):
    """inputs and their float64 reference (on the device), computed once per (generator, shape) and shared between the dtypes"""
    key = (gen, B, N, D, C)
    if key not in _REFS:
        ins = AU.make_inputs(gen, B, N, D, C)
        val = (ins, AU.attn_ref(*ins, device=DEV))
        if N > 2048:
            return val
        _REFS[key] = val
    return _REFS[key]


def _case(dtype, family, route, gen, N, D, C, B=2):
    assert L.load().msau_selfattn_route(dtype, N, D, C) == route, "the case does not run the family it is meant for"
    ins, ref = _reference(gen, B, N, D, C)
    AU.check(run_core(dtype, ins), ref, family, f"{gen} N={N} ({D},{C})", RATIOS)


ALL, TWO = AU.GENERATORS, ("normal", "shift_neg")
MFMA_N = [5, 16, 31, 48, 77, 120, 512, 513, 1024, 1344]
VALU_N = [5, 64, 65, 129, 257]


def _grid(instances, sizes):
    return [pytest.param(D, C, gen, N, id=f"{D}x{C}-{gen}-N{N}") for (D, C), gens in instances for gen in gens for N in sizes]


@pytest.mark.parametrize("D,C,gen,N", _grid([((8, 32), ALL), ((8, 64), TWO)], MFMA_N) + _grid([((16, 128), ALL)], [31, 256, 257, 520]))
def test_mfma_sweeps(D, C, gen, N):
    _case(L.BF16, "mfma", 2, gen, N, D, C)


@pytest.mark.parametrize("D,C,gen,N", _grid([((8, 8), ALL), ((8, 16), TWO), ((8, 32), TWO), ((8, 64), TWO), ((16, 128), TWO)], VALU_N))
def test_valu_instances_fp32(D, C, gen, N):
    _case(L.F32, "f32", 0, gen, N, D, C)


@pytest.mark.parametrize("D,C,gen,N", _grid([((8, 8), ALL), ((8, 16), TWO)], VALU_N))
def test_valu_instances_bf16(D, C, gen, N):
    _case(L.BF16, "bf16_valu", 0, gen, N, D, C)


@pytest.mark.parametrize("dtype,family", [pytest.param(L.F32, "f32", id="f32"), pytest.param(L.BF16, "bf16_valu", id="bf16")])
@pytest.mark.parametrize("D,C,gen,N", _grid([((24, 40), ALL), ((32, 256), TWO)], [5, 30, 257]))
def test_any_width_kernels(D, C, gen, N, dtype, family):
    _case(dtype, family, 1, gen, N, D, C)


@pytest.mark.parametrize("D,C,N,route", [(8, 64, 9552, 2), (8, 64, 9553, 0), (16, 128, 4768, 2), (16, 128, 4769, 0)])
def test_the_switch_between_mfma_and_valu(D, C, N, route):
    """the largest N whose f fits the MFMA statistics kernel's LDS ((ceil(N / 16) 16) Ds 2 + 768 <= 150 KiB) and the first that
    takes the bf16 VALU instance"""
    route_of = L.load().msau_selfattn_route
    assert route_of(L.BF16, N, D, C) == route and route_of(L.BF16, N - 1 if route == 0 else N + 1, D, C) == 2 - route
    _case(L.BF16, "mfma" if route == 2 else "bf16_valu", route, "normal", N, D, C, B=1)


@pytest.mark.parametrize("gen", TWO)
@pytest.mark.parametrize("dtype,family,route,Hb,Wb,D,C", [
    pytest.param(L.BF16, "mfma", 2, 23, 25, 8, 64, id="mfma-8x64"),
    pytest.param(L.BF16, "mfma", 2, 17, 16, 16, 128, id="mfma-16x128"),
    pytest.param(L.F32, "f32", 0, 9, 15, 8, 32, id="valu-f32"),
    pytest.param(L.BF16, "bf16_valu", 0, 9, 15, 8, 16, id="valu-bf16"),
    pytest.param(L.F32, "f32", 1, 6, 5, 24, 40, id="any-f32"),
    pytest.param(L.BF16, "bf16_valu", 1, 6, 5, 24, 40, id="any-bf16"),
])
def test_extents(dtype, family, route, Hb, Wb, D, C, gen):
    sizes = [(Hb, Wb), (Hb - 2 | 1, Wb - 3 | 1), (1, 1)]
    B, N = len(sizes), Hb * Wb
    assert L.load().msau_selfattn_route(dtype, N, D, C) == route
    ext = torch.tensor(sizes, dtype=torch.int32)
    ins = AU.make_inputs(gen, B, N, D, C, extent=ext, W=Wb)
    got = run_core(dtype, ins, ext, Wb)
    AU.check(got, AU.attn_ref(*ins, extent=ext, W=Wb, device=DEV), family, f"{gen} extents {Hb}x{Wb} ({D},{C})", RATIOS)
    x = ins[3].to(DEV)
    for b in range(B):
        out = ~AU.extent_mask(ext[b], N, Wb, DEV)
        assert torch.equal(got["y"][b][out].float(), x[b][out]), "y = x outside the extent"
        for k in ("dh", "dg", "df"):
            assert float(got[k][b][out].float().abs().sum()) == 0.0, f"{k} = 0 outside the extent"
