"""CPU: the float64 box-convolution reference of tests/box_util.py against oracle/box_oracle.py, autograd and finite differences;
the sharpness of its bounds (perturbations that must fail); fp32 prefix sums in the kernels' order and two others against the
integral-image bound.  tests/test_box_ops_gpu.py holds the HIP kernels to this reference."""
import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from oracle import box_oracle as BO
from tests import box_util as U

SMALL = [c for c in U.CASES if c.name in ("base", "H7", "C5of8", "F1", "C16F2")]


def _boxes(c, kind, seed=3):
    gen = torch.Generator().manual_seed(seed + c.H)
    return U.make_boxes(kind, c.C, c.F, c.H, c.W, gen, rot=seed)


def _rand64(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_definition_form_equals_the_oracle(c, kind):
    p = _boxes(c, kind)
    x = _rand64((c.B, c.C, c.H, c.W), 1)
    q = p.double().view(4, c.C, c.F)
    want = BO.box_conv(x, q[0], q[1], q[2], q[3])
    got = U.filter_def(x, p, U.fwd_planes(c.C, c.F))
    assert float((got - want).abs().max()) <= 1e-12 * float(x.abs().max())


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_own_ii_form_equals_the_definition_on_an_exact_integral_image(c):
    d = U.make_inputs(c, "int", L.F32)
    ii = U.integral(d["x"])
    v, m = U.filter_from_ii(ii, d["params"], c.H, c.W, U.fwd_planes(c.C, c.F))
    want = U.filter_def(d["x"], d["params"], U.fwd_planes(c.C, c.F))
    assert float((v - want).abs().max()) <= 1e-13 * float(m.max())
    assert bool((m + 1e-12 >= v.abs()).all())
    # the summed form on the reflected boxes
    iig = U.integral(d["g"])
    pr = U.reflected(d["params"])
    v = U.sum_filters(U.filter_from_ii(iig, pr, c.H, c.W, torch.arange(c.CF))[0], c.C, c.F)
    want = U.sum_filters(U.filter_def(d["g"], pr, torch.arange(c.CF)), c.C, c.F)
    assert float((v - want).abs().max()) <= 1e-12 * float(d["g"].abs().sum(1).max() + 1)


def _pair_losses(x, g, p, c):
    return (g * U.filter_def(x, p, U.fwd_planes(c.C, c.F))).sum((0, 2, 3))


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_parameter_gradient_equals_forward_differences(c):
    """Boxes on multiples of 1/8 (integer-positioned, border-touching, larger than the image and wholly outside ones among them,
    U.special_boxes) and a dyadic step h = 2^-10 towards +: the box integral G = sum g S is linear in the edge over [p, p + h] and so is
    A, hence L(h) - L(0) = h (dG - L(0) dA) / (A + h dA) EXACTLY: the difference quotient times (A + h dA) / A is the derivative
    towards + up to float64 rounding.  This pins the one-sided rule of U.edge_weights, p == 0 and p == H included."""
    p = _boxes(c, "int")
    assert {tuple(s) for s in U.special_boxes(c.H, c.W)} >= {tuple(p[:, k].tolist()) for k in range(min(c.CF, 8))}
    x, g = _rand64((c.B, c.C, c.H, c.W), 2), _rand64((c.B, c.CF, c.H, c.W), 3)
    mh, mw = 28.0, 7.0
    got = U.param_grad(U.integral(x), p, g, mh, mw)
    S = U.param_grad(U.integral(x.abs()), p, g.abs(), mh, mw, mag="terms")
    h = 2.0 ** -10
    L0 = _pair_losses(x, g, p, c)
    hh, ww, A = U.areas(p)
    for k in range(4):
        q = p.clone()
        q[k] += h
        dA = (ww if k < 2 else hh) * (-1 if k % 2 == 0 else 1)
        fd = (_pair_losses(x, g, q, c) - L0) / h * (A + h * dA) / A * (mh if k < 2 else mw)
        assert float(((fd - got[k]).abs() / (S[k] + 1e-9)).max()) < 1e-10, k
    # a box wholly outside the image: no output, no gradient; every pixel's edges of the all-covering box are clamped
    for k, b in enumerate(p.T.tolist()):
        if tuple(b) in [tuple(s) for s in U.special_boxes(c.H, c.W)[3:5]]:
            assert float(got[:, k].abs().max()) == 0.0 and float(L0[k]) == 0.0
    assert bool((S + 1e-9 >= got.abs()).all())


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_gradients_equal_autograd_away_from_ties(c):
    p = _boxes(c, "rand")
    pos = torch.cat([U.edges(c.H, p[0], p[1])[i].flatten() for i in (0, 1)] + [U.edges(c.W, p[2], p[3])[i].flatten() for i in (0, 1)]).double()
    assert float((pos - pos.round()).abs().min()) > 1e-6                      # no edge on a pixel boundary
    x, g = _rand64((c.B, c.C, c.H, c.W), 4), _rand64((c.B, c.CF, c.H, c.W), 5)
    q = p.double().view(4, c.C, c.F).clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    BO.box_conv(xr, q[0], q[1], q[2], q[3]).backward(g)
    mh, mw = 28.0, 7.0
    got = U.param_grad(U.integral(x), p, g, mh, mw)
    S = U.param_grad(U.integral(x.abs()), p, g.abs(), mh, mw, mag="terms")
    want = q.grad.view(4, c.CF) * torch.tensor([mh, mh, mw, mw], dtype=torch.float64)[:, None]
    # the reference forms the edge positions in fp32 as the kernels do: 2^-24 of a position of up to 2^7, relative to an extent >= 1
    assert float(((got - want).abs() / (S + 1e-9)).max()) < 1e-4
    taps = U.param_grad(U.integral(x.abs()), p, g.abs(), mh, mw, mag="taps")
    assert bool((taps >= S * (1 - 1e-9)).all())                               # on one II the tap magnitudes dominate the per-pixel terms
    # the input gradient: the reflected boxes over g, summed over the filters
    gin = U.sum_filters(U.filter_def(g, U.reflected(p), torch.arange(c.CF)), c.C, c.F)
    assert float((gin - xr.grad).abs().max()) <= 1e-12 * float(g.abs().sum(1).max())


# ---- sensitivity: what the bounds must see ------------------------------------------------------------------------------------
def test_one_ulp_in_one_entry_of_an_integer_integral_image_fails():
    c = U.LARGEST
    d = U.make_inputs(c, "int", L.F32)
    ii = U.integral(d["x"])
    P = U.integral(d["x"].abs())
    bound = U.ii_bound("int", P, c.H, c.W)
    assert U.check(ii.float(), ii, bound, "clean") == 0.0
    for sign in (1.0, -1.0):
        bad = ii.float().clone()
        v = bad[0, 2, c.H, c.W - 1]
        bad[0, 2, c.H, c.W - 1] = torch.nextafter(v, v + sign * 1e9)
        with pytest.raises(AssertionError):
            U.check(bad, ii, bound, "perturbed")


def test_one_dropped_pixel_at_the_far_corner_fails_the_random_bound():
    c = U.LARGEST
    d = U.make_inputs(c, "rand", L.F32)
    x = d["x"]
    P = U.integral(x.abs())
    bound = U.ii_bound("rand", P, c.H, c.W)
    ii = U.integral(x)
    U.check(torch.from_numpy(U.ii_fp32(x.reshape(-1, c.H, c.W).numpy(), "kernel")).view_as(ii), ii, bound, "clean")
    seen = 0
    for b in range(c.B):
        for ch in range(c.C):
            px = float(x[b, ch, -1, -1].abs())
            if px <= float(bound[b, ch, -1, -1]):
                continue                                                      # (a pixel below the rounding of its own sum)
            x2 = x.clone()
            x2[b, ch, -1, -1] = 0.0
            with pytest.raises(AssertionError):
                U.check(U.integral(x2).float(), ii, bound, "dropped")
            seen += 1
    assert seen >= 0.8 * c.B * c.C, seen


@pytest.mark.parametrize("kind", ["int", "rand"])
def test_two_bf16_ulps_in_one_output_element_fail(kind):
    c = U.LARGEST
    d = U.make_inputs(c, kind, L.BF16)
    ii = U.integral(torch.relu(d["x"])).float().double()
    v, m = U.filter_from_ii(ii, d["params"], c.H, c.W, U.fwd_planes(c.C, c.F))
    S = v.abs() if kind == "int" else m
    stored = v.bfloat16().double()
    U.check(stored, v, U.filter_bound(S, stored, v, L.BF16), "clean")
    i = tuple(int(k) for k in torch.unravel_index(v.abs().argmax(), v.shape))
    for sign in (1.0, -1.0):
        bad = stored.clone()
        bad[i] += sign * 2 * float(U.ulp_bf16(stored[i]))
        with pytest.raises(AssertionError):
            U.check(bad, v, U.filter_bound(S, bad, v, L.BF16), "perturbed")


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("c", U.CASES, ids=lambda c: c.name)
def test_one_dropped_edge_term_fails_the_gradient_bound(c, kind):
    """every shape the GPU test runs, every pair, every edge: a gradient that lost that edge term is beyond REL * S + ABS.  A bound
    relative to the magnitudes of the terms cannot see a term whose SIGNED sum over the pixels happens to cancel to below 2e-5 of
    them (random g: 2 of the ~1000 terms of the 'rand' cases); none may escape with integer inputs, at most one in fifty otherwise"""
    d = U.make_inputs(c, kind, L.F32)
    xt, g, p = torch.relu(d["x"]), d["g"], d["params"]
    ii = U.integral(xt) if kind == "int" else U.integral(xt).float().double()
    ref = U.param_grad(ii, p, g, c.max_size, c.max_size)
    S = U.param_grad(U.integral(xt), p, g.abs(), c.max_size, c.max_size, mag="terms")
    bound = U.REL * S + U.ABS
    U.check(ref.float(), ref, bound + 2.0 ** -24 * ref.abs(), "clean")
    loose = U.REL * U.param_grad(ii, p, g.abs(), c.max_size, c.max_size, mag="taps") + U.ABS
    seen = missed = missed_loose = 0
    for pair in range(c.CF):
        for k in range(4):
            bad = U.param_grad(ii, p, g, c.max_size, c.max_size, drop=(k, pair))
            if float((bad - ref).abs().max()) == 0.0:
                continue                                                      # (no such edge inside the image: nothing dropped)
            seen += 1
            missed += bool(((bad - ref).abs() <= bound).all())
            missed_loose += bool(((bad - ref).abs() <= loose).all())
    assert seen >= c.CF and missed <= (0 if kind == "int" else seen // 50), (seen, missed)
    # ... which is why S is NOT taken over the magnitudes of the integral-image taps, the worst-case bound of the kernel's arithmetic
    print(f"{c.name} {kind}: {seen} dropped terms, {missed} unseen, {missed_loose} unseen by a bound over the tap magnitudes")
    if c.H * c.W >= 9 * 63:
        assert missed_loose > missed, (missed_loose, missed)


# ---- fp32 prefix sums: the share of the bound that real orders use --------------------------------------------------------------
ORDERS = ("kernel", "cols-rows", "rows-cols")


def _shares(x):
    N, H, W = x.shape
    ref = U.integral(torch.from_numpy(x).double()[None])[0]
    bound = (H + W) * 2.0 ** -24 * U.integral(torch.from_numpy(x).double().abs()[None])[0]
    out = {}
    for o in ORDERS:
        err = (torch.from_numpy(U.ii_fp32(x, o)).double() - ref).abs()
        assert float(err[bound == 0].max()) == 0.0                             # (leading zeros of a relu'd plane: nothing to round)
        out[o] = float((err[bound > 0] / bound[bound > 0]).max())
    return out


@pytest.mark.parametrize("H,W", [(U.LARGEST.H, U.LARGEST.W), (512, 384)], ids=["largest-test-shape", "cfg5-513x385"])
def test_fp32_prefix_sums_stay_inside_the_bound(H, W):
    rng = np.random.default_rng(H)
    x = (0.5 * rng.standard_normal((4, H, W))).astype(np.float32)
    for name, v in (("signed", x), ("relu", np.maximum(x, 0))):
        shares = _shares(v)
        print(f"II {H + 1} x {W + 1} {name}: share of (H + W) 2^-24 P used -- " + ", ".join(f"{o} {s:.3f}" for o, s in shares.items()))
        assert max(shares.values()) < 0.5, shares
    if H == 512:
        # the known weakness of a fp32 integral image: a one-pixel box at the far corner is a difference of four sums of ~H * W terms
        xr = np.maximum(x, 0)
        for o in ORDERS:
            ii = torch.from_numpy(U.ii_fp32(xr, o)).double()
            one = ii[:, -1, -1] - ii[:, -2, -1] - ii[:, -1, -2] + ii[:, -2, -2]
            err = (one - torch.from_numpy(xr[:, -1, -1]).double()).abs()
            ulp = float(torch.from_numpy(np.spacing(U.ii_fp32(xr, o)[:, -1, -1])).max())
            print(f"one-pixel box at the far corner of 513 x 385, {o}: worst |error| {float(err.max()):.4g} "
                  f"(ulp of II there {ulp:.4g}, mean pixel {float(xr.mean()):.3f})")
            assert float(err.max()) <= 4 * (H + W) * 2.0 ** -24 * float(ii[:, -1, -1].max())
