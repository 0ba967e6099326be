"""CPU: the attention tests' float64 reference (tests/attention_util.py) is itself checked -- against float64 autograd through the
plain N x N formula, against the reference model's golden vectors, and its error bounds against an emulation of the kernels'
roundings: the bounds the GPU tests apply are satisfiable by correct arithmetic before any kernel is judged by them."""
import functools

import pytest
import torch

from oracle import msau_oracle as O
from tests import attention_util as AU
from tests.golden_util import load_ops


def _plain(f, g, h, x, dy):
    """one sample, float64 autograd through softmax / matmul -> y, df, dg, dh, m, Z, delta"""
    f, g, h = (t.clone().requires_grad_(True) for t in (f, g, h))
    s = g @ f.T
    P = torch.softmax(s, dim=-1)
    y = x + P.T @ h
    y.backward(dy)
    m = s.max(1).values
    dh = (P @ dy).detach()
    return dict(y=y.detach(), df=f.grad, dg=g.grad, dh=h.grad, m=m.detach(), Z=torch.exp(s - m[:, None]).sum(1).detach(),
                delta=(h.detach() * dh).sum(1))


def _close(a, b, what, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("N,D,C", [(37, 8, 16), (5, 16, 8), (130, 8, 32)])
def test_reference_equals_autograd(N, D, C):
    G = torch.Generator().manual_seed(N)
    B = 2
    f, g = (torch.randn(B, N, D, generator=G, dtype=torch.float64) for _ in range(2))
    h, x, dy = (torch.randn(B, N, C, generator=G, dtype=torch.float64) for _ in range(3))
    ref = AU.attn_ref(f, g, h, x, dy)
    for b in range(B):
        want = _plain(f[b], g[b], h[b], x[b], dy[b])
        for k, v in want.items():
            _close(ref[k][b], v, (k, b))
    # the sums of |terms| dominate what they bound
    S = ref["S"]
    assert bool((ref["dh"].abs() <= S["dh"] * (1 + 1e-12)).all()) and bool((ref["delta"].abs() <= S["delta"] * (1 + 1e-12)).all())
    assert bool(((ref["y"] - x).abs() <= S["y"] * (1 + 1e-12)).all())
    for k in ("dg", "df"):
        assert bool((ref[k].abs() <= S[k + "1"] * (1 + 1e-12)).all()) and bool((S[k + "1"] <= S[k + "2"] * (1 + 1e-12)).all())


def test_reference_with_extents_equals_each_sample_cropped_alone():
    Hb, Wb, D, C = 7, 9, 8, 16
    sizes = [(Hb, Wb), (Hb - 2 | 1, Wb - 3 | 1), (1, 1)]
    B, N = len(sizes), Hb * Wb
    ext = torch.tensor(sizes, dtype=torch.int32)
    f, g, h, x, dy = (t.double() for t in AU.make_inputs("normal", B, N, D, C, extent=ext, W=Wb))
    ref = AU.attn_ref(f, g, h, x, dy, extent=ext, W=Wb)
    for b in range(B):
        inn = AU.extent_mask(ext[b], N, Wb, "cpu")
        want = _plain(*(t[b][inn] for t in (f, g, h, x, dy)))
        for k, v in want.items():
            _close(ref[k][b][inn], v, (k, b))
        assert torch.equal(ref["y"][b][~inn], x[b][~inn])
        for k in ("dh", "dg", "df", "delta"):
            assert float(ref[k][b][~inn].abs().sum()) == 0.0, (k, b)


@pytest.mark.parametrize("tag", ["attn64", "attn32"])
def test_reference_reproduces_the_golden_attention_block(tag):
    """the projections from the golden weights (O.conv_same), attn_ref on them, and the 1x1 convs' backward by hand: y and the input
    gradient of the original model's block"""
    gd = load_ops()
    x = torch.tensor(gd[f"{tag}.x"]).double()
    gy = torch.tensor(gd[f"{tag}.gy"]).double()
    B, C, H, W = x.shape
    w = {m: torch.tensor(gd[f"{tag}.p.attention_block.{m}.conv.weight"]).double() for m in "fgh"}
    bias = {m: torch.tensor(gd[f"{tag}.p.attention_block.{m}.conv.bias"]).double() for m in "fgh"}
    flat = lambda t: t.reshape(B, t.shape[1], H * W).transpose(1, 2).contiguous()            # NCHW -> [B, N, c]
    f, g, h = (flat(O.conv_same(x, w[m], bias[m])) for m in "fgh")
    ref = AU.attn_ref(f, g, h, flat(x), flat(gy))
    unflat = lambda t: t.transpose(1, 2).reshape(B, -1, H, W)
    y = unflat(ref["y"])
    gx = gy + sum(unflat(ref["d" + m] @ w[m][:, :, 0, 0]) for m in "fgh")
    for got, key in ((y, "y"), (gx, "gx")):
        want = torch.tensor(gd[f"{tag}.{key}"]).double()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), key


RATIOS = {}
EMU_SHAPES = [(5, 8, 32), (31, 8, 32), (77, 8, 64), (257, 8, 8), (120, 16, 128), (30, 24, 40)]


@functools.lru_cache(maxsize=None)
def _case(gen, N, D, C):
    ins = AU.make_inputs(gen, 2, N, D, C)
    return ins, AU.attn_ref(*ins)


@pytest.mark.parametrize("family", ["mfma", "bf16_valu", "f32"])
@pytest.mark.parametrize("gen", AU.GENERATORS)
def test_emulated_roundings_stay_inside_the_bounds(gen, family):
    """float64 against fp32 sums with P and dS rounded to bf16 (mfma) / fp32 sums and bf16 stores (bf16_valu) / plain fp32: EVERY
    element inside the bounds of attention_util.check, for every generator of the GPU tests.  Run with -s for the worst ratios."""
    for N, D, C in EMU_SHAPES:
        ins, ref = _case(gen, N, D, C)
        AU.check(AU.emulate(*ins, family), ref, family, f"{gen} N={N} ({D},{C})", RATIOS)


def test_the_calibrated_mfma_constants_are_at_most_twice_what_the_emulation_needs():
    """K_DELTA_MFMA and K_CANCEL_MFMA replace the fp32 slack where delta is formed from bf16-rounded probabilities: the fp32 slack is
    NOT satisfiable there, and the raised constants are no more than 2x the worst ratio of float64 against the emulation"""
    wd = wc = 0.0
    for gen in AU.GENERATORS:
        for N, D, C in EMU_SHAPES:
            ins, ref = _case(gen, N, D, C)
            got, S = AU.emulate(*ins, "mfma"), ref["S"]
            wd = max(wd, float(((got["delta"].double() - ref["delta"]).abs() / S["delta"].clamp_min(1e-300)).max()))
            for k in ("dg", "df"):
                gk = got[k].double()
                e = (gk - ref[k]).abs() - 0.5 * AU.ulp_bf16(torch.maximum(gk.abs(), ref[k].abs())) * (1 + 1e-6) - AU.K_P_BF16 * S[k + "1"]
                wc = max(wc, float((e / S[k + "2"].clamp_min(1e-300)).max()))
    print(f"emulation needs: delta {wd:.3g} of S(delta); dg, df {wc:.3g} of S2")
    assert AU.ACC < wd <= AU.K_DELTA_MFMA <= 2 * wd, (wd, AU.K_DELTA_MFMA)
    assert AU.ACC < wc <= AU.K_CANCEL_MFMA <= 2 * wc, (wc, AU.K_CANCEL_MFMA)


@pytest.mark.parametrize("family", ["mfma", "bf16_valu", "f32"])
@pytest.mark.parametrize("gen", ["normal", "shift_neg"])
def test_emulated_roundings_with_extents(gen, family):
    Hb, Wb, D, C = 9, 15, 8, 32
    sizes = [(Hb, Wb), (Hb - 2 | 1, Wb - 3 | 1), (1, 1)]
    ext = torch.tensor(sizes, dtype=torch.int32)
    ins = AU.make_inputs(gen, 3, Hb * Wb, D, C, extent=ext, W=Wb)
    got = AU.emulate(*ins, family, extent=ext, W=Wb)
    AU.check(got, AU.attn_ref(*ins, extent=ext, W=Wb), family, f"{gen} extents", RATIOS)


def test_generators_are_what_they_claim():
    """shifted rows: every score near -+16 D; the last rows of the sample among them; peaked rows nearly one-hot"""
    N, D = 77, 8
    f, g, *_ = AU.make_inputs("shift_neg", 2, N, D, 32)
    s = g.double() @ f.double().transpose(1, 2)
    rows = (torch.arange(N) % 4 == 1) | (torch.arange(N) >= N - 3)
    assert float(s[:, rows].max()) < -100 and float(s[:, rows].min()) > -160 and bool(rows[-1])
    f, g, *_ = AU.make_inputs("shift_pos", 2, N, D, 32)
    assert float((g.double() @ f.double().transpose(1, 2))[:, rows].min()) > 100
    f, g, *_ = AU.make_inputs("peaked", 2, 257, D, 32)
    s = g.double() @ f.double().transpose(1, 2)
    assert 9 < float(s.std()) < 15 and float(torch.softmax(s, -1).max(-1).values.median()) > 0.5
    for t in AU.make_inputs("normal", 2, N, D, 32):
        assert torch.equal(t, t.bfloat16().float())
