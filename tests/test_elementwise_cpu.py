"""No GPU: the float64 references and the bounds of tests/elementwise_util.py, which tests/test_elementwise_gpu.py holds the
kernels of msau_amd/csrc/elementwise.hip to.

1. the references agree with torch (local_response_norm and its autograd, max_pool2d and its autograd) in float64;
2. a float32 restatement of each LRN kernel form stays inside the bound on every test input;
3. the bound catches a shifted window, swapped windows, n/2 taken as (n-1)/2, beta off by 1 % and alpha/n taken as alpha, by
   10 x at least, in bf16 storage as in fp32;
4. at the reference's alpha = 1e-4 a shifted window never fails the bf16 forward check by the 10 x of (3), and from 32 channels on
   moves no output by half a bf16 ulp: why settings (b) and (c) exist."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_util as U

FAST = [(8 * G, 8 * G, 8 * G) for G in U.FAST_G]
ALL_CCN = FAST + list(U.GENERIC)


def _is_fast(C, Cs, n):
    return (C, Cs, n) in FAST


def _cases():
    """every LRN test input of the GPU file: (id, fast, n, alpha, beta, k, x, dy)"""
    out = []
    for C, Cs, n in ALL_CCN:
        fast = _is_fast(C, Cs, n)
        for s in ("a", "b", "c") if fast else ("b", "c"):
            alpha, beta, k, scale = U.setting(s, n)
            x, dy = U.lrn_inputs(U.NPIX, C, scale, seed=100 * C + n)
            out.append((f"C{C}n{n}-{s}", fast, n, alpha, beta, k, x, dy))
        if fast:
            for s in ("b", "c"):
                alpha, beta, k, _ = U.setting(s, n)
                x, dy = U.energy_inputs(5, n, seed=n)
                out.append((f"C{C}n{n}-{s}-energy", fast, n, alpha, beta, k, x, dy))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("C,Cs,n", ALL_CCN)
def test_lrn_references_agree_with_torch(C, Cs, n):
    for s in ("a", "b", "c"):
        alpha, beta, k, scale = U.setting(s, n)
        x, dy = U.lrn_inputs(U.NPIX, C, scale, seed=C + n)
        xr = x.clone().requires_grad_(True)
        y = F.local_response_norm(xr.unsqueeze(-1), n, alpha, beta, k).squeeze(-1)
        y.backward(dy)
        for got, ref in ((U.lrn_fwd(x, n, alpha, beta, k), y.detach()), (U.lrn_bwd(x, dy, n, alpha, beta, k), xr.grad),
                         (U.lrn_bwd_ref(x, dy, n, alpha, beta, k, dim=1)[0], xr.grad)):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (s, C, n)


def test_lrn_bwd_ref_in_nchw_is_the_plan_level_statement():
    """test_launch_ulp_gpu.py calls lrn_bwd_ref(a, dy) on NCHW tensors with n == C and the reference's settings"""
    from oracle import msau_oracle as O
    torch.manual_seed(3)
    a, dy = 10 * torch.randn(2, 16, 3, 5, dtype=torch.float64), torch.randn(2, 16, 3, 5, dtype=torch.float64)
    ar = a.clone().requires_grad_(True)
    O.lrn(ar, 16).backward(dy)
    da, terms = U.lrn_bwd_ref(a, dy)
    assert float((da - ar.grad).abs().max()) <= 1e-12 * float(ar.grad.abs().max())
    d = (a / O.lrn(a, 16)) ** (1 / 0.75)
    want = dy.abs() * d ** -0.75 + a.abs() * (2 * 1e-4 * 0.75 / 16) * (dy.abs() * a.abs() * d ** -1.75).sum(1, keepdim=True)
    assert torch.allclose(terms, want, rtol=1e-10, atol=0)


@pytest.mark.parametrize("H,W", U.POOL_HW + ((3, 13),))
def test_pool_references_agree_with_torch(H, W):
    B, C = 3, 8
    for negative in (False, True):
        x = U.pool_input(B, H, W, C, seed=H * 10 + W, negative=negative).double()
        y, idx = U.pool_fwd(x)
        ref = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (0, W % 2, 0, H % 2)), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(y, ref)
        v = U.pool_windows(x)
        assert torch.equal(v.gather(0, idx.long().unsqueeze(0))[0], y)
        for pos in range(4):                       # the FIRST maximum: nothing before it is as large
            assert not bool(((v[pos] >= y) & (idx > pos)).any())
    # backward against autograd, tie-free (distinct non-zero values)
    g = torch.Generator().manual_seed(H + W)
    x = (torch.randperm(B * H * W * C, generator=g).double() - B * H * W * C / 2 + 0.5).reshape(B, H, W, C)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(F.pad(xr.permute(0, 3, 1, 2), (0, W % 2, 0, H % 2)), 2, 2).permute(0, 2, 3, 1)
    gy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    yr.backward(gy)
    y, idx = U.pool_fwd(x)
    assert torch.equal(y, yr.detach()) and torch.equal(U.pool_scatter(gy, idx, H, W), xr.grad)
    dx, _ = U.pool_bwd(gy, idx, None, None, False, None, H, W)
    assert torch.equal(dx, xr.grad)


def test_pool_backward_reference_order_and_extent():
    B, H, W, C = 3, 3, 5, 8
    g = torch.Generator().manual_seed(1)
    gy = torch.randn(B, 2, 3, C, generator=g)
    idx = torch.randint(0, 4, gy.shape, generator=g).to(torch.uint8)
    old = torch.randn(B, H, W, C, generator=g)
    mask = torch.tensor([1.0, 0.0, -0.0, -0.5])[torch.randint(0, 4, (B, H, W, C), generator=g)]
    ext = torch.tensor([[0, 0], [3, 5], [1, 3]], dtype=torch.int32)
    s = U.pool_scatter(gy, idx, H, W)
    assert float(s.abs().sum()) < float(gy.abs().sum())              # positions in the padding are dropped
    relu, _ = U.pool_bwd(gy, idx, old, mask, False, None, H, W)
    assert torch.equal(relu, torch.where(mask > 0, old + s, torch.zeros_like(s)))
    elu, slack = U.pool_bwd(gy, idx, old, mask, True, ext, H, W)
    want = torch.where(mask > 0, old + s, (old + s) * (mask + 1))
    assert float(elu[0].abs().max()) == 0 and torch.equal(elu[1], want[1]) and torch.equal(elu[2, :1, :3], want[2, :1, :3])
    assert float(elu[2, 1:].abs().max()) == 0 and float(elu[2, :, 3:].abs().max()) == 0 and float(slack[0].max()) == 0


def _restate(fast, n, alpha, beta, k, x, dy):
    xn, gn = x.numpy(), (None if dy is None else dy.numpy())
    out = U.lrn_fast32(xn, gn, alpha, beta, k) if fast else U.lrn_generic32(xn, gn, n, alpha, beta, k)
    return torch.from_numpy(out.astype(np.float64))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_restatement_stays_inside_the_bound(case):
    _, fast, n, alpha, beta, k, x, dy = case
    yf = U.worst_ratio(_restate(fast, n, alpha, beta, k, x, None), U.lrn_fwd(x, n, alpha, beta, k),
                       U.lrn_fwd_bound(x, n, alpha, beta, k, fast), False)
    yb = U.worst_ratio(_restate(fast, n, alpha, beta, k, x, dy), U.lrn_bwd(x, dy, n, alpha, beta, k),
                       U.lrn_bwd_bound(x, dy, n, alpha, beta, k, fast), False)
    print(f"restatement / bound: forward {yf:.3f} backward {yb:.3f}")
    assert yf <= 1 and yb <= 1, (yf, yb)


def test_restatement_is_not_the_reference_in_disguise():
    """the float32 restatement differs from float64 by fp32 rounding, and a float32 restatement with a shifted window fails"""
    x, dy = U.lrn_inputs(U.NPIX, 64, 1.0, seed=1)
    y32 = _restate(True, 64, 64.0, 0.75, 1.0, x, None)
    ref = U.lrn_fwd(x, 64, 64.0, 0.75, 1.0)
    assert 0 < float((y32 - ref).abs().max()) < 1e-6
    shifted = _restate(True, 64, 64.0, 0.75, 1.0, torch.roll(x, 1, 1), None).roll(-1, 1)
    assert U.worst_ratio(shifted, ref, U.lrn_fwd_bound(x, 64, 64.0, 0.75, 1.0, True), False) > 10


def _mutation_ratios(case, mut):
    """-> [(fp32 ratio, bf16 ratio)] for forward and backward, or None where the mutation changes nothing"""
    _, fast, n, alpha, beta, k, x, dy = case
    m = U.MUTATIONS[mut]
    refs = (U.lrn_fwd(x, n, alpha, beta, k), U.lrn_bwd(x, dy, n, alpha, beta, k))
    wrong = (U.lrn_fwd(x, n, alpha, beta, k, m), U.lrn_bwd(x, dy, n, alpha, beta, k, m))
    if U.mutation_is_identity(mut, n):
        assert all(torch.equal(a, b) for a, b in zip(refs, wrong))
        return None
    bounds = (U.lrn_fwd_bound(x, n, alpha, beta, k, fast), U.lrn_bwd_bound(x, dy, n, alpha, beta, k, fast))
    return [(U.worst_ratio(bad.float().double(), ref, bound, False), U.worst_ratio(U.bf16_round(bad), ref, bound, True))
            for ref, bad, bound in zip(refs, wrong, bounds)]


BC_CASES = [c for c in CASES if "-a" not in c[0]]


@pytest.mark.parametrize("mut", sorted(U.MUTATIONS))
@pytest.mark.parametrize("case", BC_CASES, ids=[c[0] for c in BC_CASES])
def test_bound_catches_the_mutation(case, mut):
    """Every input of settings (b), (c) and the single-channel-energy inputs, forward and backward: 10 x the bound in fp32 and in
    bf16 storage.  One exception, which is arithmetic and not a weakness of the bound: beta off by 1 % changes an output by
    0.01 beta ln d relative, half a bf16 ulp is up to 2^-8 relative, so 10 x needs beta ln d >= 3.9 (d >= 180 at beta = 0.75) --
    randn inputs reach that only in wide windows.  There the mutation must still FAIL the bf16 check on every input, and
    test_beta_mutation_fails_tenfold_on_every_instance shows the 10 x on some input of every kernel instance."""
    r = _mutation_ratios(case, mut)
    for f32, bf16 in r or ():
        assert f32 >= 10 and bf16 >= (2 if mut == "beta" else 10), (f32, bf16)


@pytest.mark.parametrize("s", ["b", "c"])
@pytest.mark.parametrize("inst", [f"G{G}" for G in U.FAST_G] + ["generic"])
def test_beta_mutation_fails_tenfold_on_every_instance(inst, s):
    """per kernel instance (G x F075, generic x F075): some input of the setting exceeds the bf16 bound 10 x, forward and backward"""
    mine = [c for c in BC_CASES if f"-{s}" in c[0] and (c[1] and f"C{8 * int(inst[1:])}n" in c[0] if inst != "generic" else not c[1])]
    assert mine
    rs = [_mutation_ratios(c, "beta") for c in mine]
    for direction in (0, 1):
        assert max(r[direction][1] for r in rs) >= 10, [r[direction][1] for r in rs]


@pytest.mark.parametrize("G", U.FAST_G)
def test_setting_a_barely_sees_a_shifted_window_in_bf16(G):
    """alpha = 1e-4, inputs 10 * randn, forward, bf16 storage: the shifted window never reaches the 10 x by which it fails in
    settings (b) and (c).  From 32 channels on it moves NO output by half a bf16 ulp: what is stored is then one rounding step
    from the correctly rounded value at most, and only where a rounding boundary happens to lie in between.  (At 8 and 16
    channels alpha / n is large enough for 3.5 and 1.5 half ulps.)  In fp32 storage the same window fails by orders of magnitude.
    The backward is not blind at this alpha: where dy_c is small the adjoint sum is all of da_c, and one term more or less in it
    is a change of order 1 -- printed, not asserted."""
    n = 8 * G
    alpha, beta, k, scale = U.setting("a", n)
    x, dy = U.lrn_inputs(U.NPIX, n, scale, seed=100 * n + n)
    m = U.MUTATIONS["shift"]
    ref, bad, bound = U.lrn_fwd(x, n, alpha, beta, k), U.lrn_fwd(x, n, alpha, beta, k, m), U.lrn_fwd_bound(x, n, alpha, beta, k, True)
    moved = float(((bad - ref).abs() / (0.5 * U.ulp_bf16(ref))).max())
    seen = U.worst_ratio(U.bf16_round(bad), ref, bound, True)
    rb, bb = U.lrn_bwd(x, dy, n, alpha, beta, k), U.lrn_bwd(x, dy, n, alpha, beta, k, m)
    print(f"G={G}: forward shift / half ulp {moved:.3f}, stored error / tolerance {seen:.3f}; backward stored error / tolerance "
          f"{U.worst_ratio(U.bf16_round(bb), rb, U.lrn_bwd_bound(x, dy, n, alpha, beta, k, True), True):.1f}")
    assert seen < 5
    if G >= 4:
        assert moved < 1 and seen < 2
    assert U.worst_ratio(bad, ref, bound, False) > 100


@pytest.mark.parametrize("G", U.FAST_G)
def test_setting_a_bound_is_no_looser_than_the_plan_level_one(G):
    """2e-6 |y| forward, ACC * 0.2 * terms backward (test_launch_ulp_gpu.py)"""
    n = 8 * G
    alpha, beta, k, scale = U.setting("a", n)
    x, dy = U.lrn_inputs(U.NPIX, n, scale, seed=100 * n + n)
    assert bool((U.lrn_fwd_bound(x, n, alpha, beta, k, True) <= 2e-6 * U.lrn_fwd(x, n, alpha, beta, k).abs() + 1e-300).all())
    _, terms = U.lrn_bwd_ref(x, dy, n, alpha, beta, k, dim=1)
    assert bool((U.lrn_bwd_bound(x, dy, n, alpha, beta, k, True) <= 3e-5 * 0.2 * terms + 1e-300).all())


def test_simple_references():
    src = torch.arange(2 * 3 * 8, dtype=torch.float64).reshape(2, 3, 8)
    assert torch.equal(U.nhwc_to_nchw(src, 5)[1, 4], src[1, :, 4])
    back = U.nchw_grad_to_nhwc(U.nhwc_to_nchw(src, 5), src, 8)
    assert torch.equal(back[..., :5], 2 * src[..., :5]) and float(back[..., 5:].abs().max()) == 0
    w = U.extent_words(2, 3, 4, 5, 2, seed=0)
    out = U.extent_copy(w, [(2, 3), (0, 0)])
    assert torch.equal(out[0, :, :2, :3], w[0, :, :2, :3]) and int(out[0, :, 2:].abs().max()) == 0 and int(out[1].abs().max()) == 0
    assert int(out[0, :, :, 3:].abs().max()) == 0
    assert any(int((w == (s - 2 ** 32 if s >= 2 ** 31 else s)).sum()) > 0 for s in U.SPECIAL_WORDS[:4])
    ids = U.onehot_ids(2, 4, 5, 5, 8, seed=0)
    oh = U.onehot(ids, 5, 8)
    assert torch.equal(oh.sum(-1), ((ids >= 0) & (ids < 5)).float()) and float(oh[..., 5:].abs().max()) == 0
    ok = (ids >= 0) & (ids < 5)
    assert torch.equal(oh.argmax(-1)[ok], ids[ok].long())
    assert float(U.onehot(ids, 5, 8, [(0, 0), (4, 5)])[0].abs().max()) == 0
