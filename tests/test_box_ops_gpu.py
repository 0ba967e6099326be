"""GPU: every kernel of msau_amd/csrc/boxconv.hip through the C ABI, element by element against the float64 reference and the
derived bounds of tests/box_util.py (checked without a GPU in tests/test_box_cpu.py): f32 and bf16 storage, integer inputs (exact
arithmetic: equality for the integral image, 2^-21 for the filter) and random ones (the filter against the integral image the
launch itself read), NaN-filled outputs with guard bands behind them, padded channels, every epilogue operand, the launch records,
the refusals, and one bf16 training plan whose box launches are each checked on their own stored operands."""
import functools

import pytest
import torch

from msau_amd import _lib as L
from tests import box_util as U

pytestmark = pytest.mark.gpu

DTYPES = [L.F32, L.BF16]
KINDS = ["int", "rand"]
BY_NAME = {c.name: c for c in U.CASES + [U.LDS_CASE]}
MAX_H, MAX_W = 28.0, 7.0                     # two factors: a gradient scaled by the other axis' factor is off by 4x


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sweep(fn):
    fn = pytest.mark.parametrize("kind", KINDS)(fn)
    fn = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: U.TNAME[d])(fn)
    return pytest.mark.parametrize("name", [c.name for c in U.CASES])(fn)


def _report(group, ratio):
    print(f"[box] {group}: error / bound {U.record(group, ratio):.3f}")


def _integral(c, dtype, src, Cn, Cs, relu_in):
    """msau_box_integral on src (float64 NCHW, Cn planes stored in Cs channels, the padded ones NaN) -> the II on the CPU"""
    x = U.to_nhwc(src, Cs, dtype, pad=U.NAN).cuda()
    ii = U.Guarded(c.B * Cn * (c.H + 1) * (c.W + 1))
    ws = U.Guarded(int(L.load().msau_box_integral_ws_floats(c.B, c.H, c.W, Cn)))
    L.call("msau_box_integral", _stream(), dtype, x.data_ptr(), ii.ptr(), ws.ptr(), c.B, c.H, c.W, Cn, Cs, int(relu_in))
    torch.cuda.synchronize()
    ii.assert_guard("integral image")
    ws.assert_guard("segment sums")
    return ii


@functools.lru_cache(maxsize=None)
def _state(name, dtype, kind):
    """the inputs of a case and the two integral images the other launches read (device buffers, kept for the module)"""
    c = BY_NAME[name]
    d = U.make_inputs(c, kind, dtype)
    d["ii"] = _integral(c, dtype, d["x"], c.C, c.Cs, True)
    d["iig"] = _integral(c, dtype, d["g"], c.CF, c.Cs_out, False)
    return d


def _check_ii(c, kind, ii, xt, what):
    got = ii.data.cpu().view(c.B, xt.shape[1], c.H + 1, c.W + 1)
    assert not bool(torch.isnan(got).any()), f"{what}: entries left unwritten"
    assert float(got[:, :, 0].abs().max()) == 0.0 and float(got[:, :, :, 0].abs().max()) == 0.0, f"{what}: row 0 / column 0"
    return U.check(got, U.integral(xt), U.ii_bound(kind, U.integral(xt.abs()), c.H, c.W), what)


@_sweep
def test_integral_image(name, dtype, kind):
    c, d = BY_NAME[name], _state(name, dtype, kind)
    r1 = _check_ii(c, kind, d["ii"], torch.relu(d["x"]), "II of relu(x)")
    r2 = _check_ii(c, kind, d["iig"], d["g"], "II of g")
    if kind == "rand":
        _report(f"integral image, rand, {U.TNAME[dtype]}", max(r1, r2))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: U.TNAME[d])
@pytest.mark.parametrize("name", [c.name for c in U.CASES])
def test_integral_image_sums_in_the_documented_order(name, dtype):
    """boxconv.hip promises a fixed order (32-row segments started from the ordered sum of the earlier segments' totals, rows scanned
    in 64-lane chunks with a carry): U.ii_fp32 restates it in numpy fp32 and the device's integral image has its bits"""
    c, d = BY_NAME[name], _state(name, dtype, "rand")
    for ii, src in ((d["ii"], torch.relu(d["x"])), (d["iig"], d["g"])):
        want = torch.from_numpy(U.ii_fp32(src.reshape(-1, c.H, c.W).numpy(), "kernel")).reshape(-1)
        assert torch.equal(ii.data.cpu(), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: U.TNAME[d])
def test_integral_image_on_the_opt_in_lds_path(dtype, kind):
    c = U.LDS_CASE
    assert c.C * 129 * 4 > 60 * 1024
    x = U.make_inputs(c, kind, dtype)["x"]
    for relu_in in (False, True):
        ii = _integral(c, dtype, x, c.C, c.Cs, relu_in)
        r = _check_ii(c, kind, ii, torch.relu(x) if relu_in else x, f"II, 192 planes, relu_in {relu_in}")
        if kind == "rand":
            _report(f"integral image, rand, {U.TNAME[dtype]}", r)


def _filter(c, dtype, ii, params, sum_filters, Cs_out, ops=None):
    """msau_box_filter into a NaN buffer (known values under accumulate) -> (stored NHWC result on the CPU, its buffer)"""
    ops = ops or {}
    dev = {k: U.to_nhwc(v, Cs_out, dtype, pad=(U.NAN if k.startswith("mask") else 0.0)).cuda() for k, v in ops.items() if k != "old"}
    n = c.B * c.H * c.W * Cs_out
    out = U.Guarded(n, U.torch_dtype(dtype), fill=U.to_nhwc(ops["old"], Cs_out, dtype) if "old" in ops else None)
    pd = params.cuda()
    ptr = lambda k: dev[k].data_ptr() if k in dev else None
    L.call("msau_box_filter", _stream(), dtype, ii.ptr(), pd.data_ptr(), out.ptr(), c.B, c.H, c.W, c.C, c.F, Cs_out, int(sum_filters),
           int("old" in ops), ptr("mask_a"), ptr("add"), ptr("mask_b"))
    torch.cuda.synchronize()
    out.assert_guard("filter output")
    return out.data.cpu().view(c.B, c.H, c.W, Cs_out), out


def _check_filter(c, dtype, kind, stored, nout, refs, what):
    """refs: [(value, magnitude)]; the padded channels hold exactly 0"""
    assert not bool(torch.isnan(stored.float()).any()), f"{what}: elements left unwritten"
    assert float(stored[..., nout:].float().abs().sum()) == 0.0, f"{what}: padded channels"
    got = U.to_nchw(stored, nout)
    return max(U.check(got, v, U.filter_bound(S, got, v, dtype), what) for v, S in refs)


def _forward_refs(c, d, kind):
    planes = U.fwd_planes(c.C, c.F)
    ii = d["ii"].data.cpu().double().view(c.B, c.C, c.H + 1, c.W + 1)
    v, m = U.filter_from_ii(ii, d["params"], c.H, c.W, planes)
    if kind == "rand":
        return [(v, m)]
    U.assert_int_filter_exact(ii)
    vd = U.filter_def(torch.relu(d["x"]), d["params"], planes)
    return [(v, v.abs()), (vd, vd.abs())]


@_sweep
def test_filter_forward(name, dtype, kind):
    c, d = BY_NAME[name], _state(name, dtype, kind)
    stored, _ = _filter(c, dtype, d["ii"], d["params"], False, c.Cs_out)
    _report(f"filter forward, {kind}, {U.TNAME[dtype]}", _check_filter(c, dtype, kind, stored, c.CF, _forward_refs(c, d, kind), "forward filter"))


def _summed_refs(c, d, kind, ops):
    """the input gradient: reflected boxes over the II of g, summed over the filters, then the epilogue"""
    pr, planes = U.reflected(d["params"]), torch.arange(c.CF)
    iig = d["iig"].data.cpu().double().view(c.B, c.CF, c.H + 1, c.W + 1)
    v, m = U.filter_from_ii(iig, pr, c.H, c.W, planes)
    forms = [(v, m)] if kind == "rand" else [(v, v.abs()), (lambda t: (t, t.abs()))(U.filter_def(d["g"], pr, planes))]
    if kind == "int":
        U.assert_int_filter_exact(iig)
    return [U.epilogue(U.sum_filters(a, c.C, c.F), U.sum_filters(b, c.C, c.F), ops.get("mask_a"), ops.get("add"), ops.get("old"),
                       ops.get("mask_b")) for a, b in forms]


EPI_CASES = [(c.name, e) for c in U.CASES for e in (U.EPILOGUES if c.name in ("base", "mix-C5-33x65") else ("none", "all"))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: U.TNAME[d])
@pytest.mark.parametrize("name,epi", EPI_CASES)
def test_input_gradient_and_its_epilogue(name, epi, dtype, kind):
    c, d = BY_NAME[name], _state(name, dtype, kind)
    ops = {k: d[k] for k in U.EPILOGUES[epi]}
    stored, _ = _filter(c, dtype, d["iig"], U.reflected(d["params"]), True, c.Cs, ops)
    _report(f"input gradient, {kind}, {U.TNAME[dtype]}", _check_filter(c, dtype, kind, stored, c.C, _summed_refs(c, d, kind, ops), f"summed filter, {epi}"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: U.TNAME[d])
def test_forward_form_takes_the_epilogue_too(dtype, kind):
    c = BY_NAME["C5of8"]
    d = _state(c.name, dtype, kind)
    gen = torch.Generator().manual_seed(5)
    ops = {k: U.draw(kind, (c.B, c.CF, c.H, c.W), gen, dtype) for k in U.EPILOGUES["all"]}
    stored, _ = _filter(c, dtype, d["ii"], d["params"], False, c.Cs_out, ops)
    refs = [U.epilogue(v, S, ops["mask_a"], ops["add"], ops["old"], ops["mask_b"]) for v, S in _forward_refs(c, d, kind)]
    _report(f"filter forward, {kind}, {U.TNAME[dtype]}", _check_filter(c, dtype, kind, stored, c.CF, refs, "forward filter with the epilogue"))


def _offsets(CF):
    """four non-adjacent runs of a larger vector, not in ascending order"""
    return [3 * CF + 17, 5, 7 * CF + 40, 5 * CF + 23], 9 * CF + 64


def _param_grad(c, dtype, d):
    gd = U.to_nhwc(d["g"], c.Cs_out, dtype, pad=U.NAN).cuda()
    offs, n = _offsets(c.CF)
    ws = U.Guarded(int(L.load().msau_box_pgrad_ws_floats(c.B, c.H, c.W, c.C, c.F)))
    fg = U.Guarded(n)
    pd = d["params"].cuda()
    L.call("msau_box_param_grad", _stream(), dtype, d["ii"].ptr(), pd.data_ptr(), gd.data_ptr(), ws.ptr(), fg.ptr(), *offs,
           c.B, c.H, c.W, c.C, c.F, c.Cs_out, MAX_H, MAX_W)
    torch.cuda.synchronize()
    ws.assert_guard("partials")
    fg.assert_guard("gradient vector")
    return fg, offs


def _gather(fg, offs, CF):
    full = fg.data.cpu()
    addressed = torch.zeros(full.numel(), dtype=torch.bool)
    for o in offs:
        addressed[o:o + CF] = True
    assert bool(torch.isnan(full[~addressed]).all()), "gradient vector: floats outside the four addressed runs were written"
    return torch.stack([full[o:o + CF] for o in offs])


@_sweep
def test_parameter_gradient(name, dtype, kind):
    c, d = BY_NAME[name], _state(name, dtype, kind)
    fg, offs = _param_grad(c, dtype, d)
    got = _gather(fg, offs, c.CF)
    xt = torch.relu(d["x"])
    exact = U.integral(xt)
    ii = exact if kind == "int" else d["ii"].data.cpu().double().view_as(exact)
    ref = U.param_grad(ii, d["params"], d["g"], MAX_H, MAX_W)
    S = U.param_grad(exact, d["params"], d["g"].abs(), MAX_H, MAX_W, mag="terms")
    _report(f"parameter gradient, {kind}, {U.TNAME[dtype]}", U.check(got, ref, U.REL * S + U.ABS, "box-parameter gradient [hmin, hmax, wmin, wmax][pair]"))


@_sweep
def test_records_give_the_bits_of_the_separate_calls(name, dtype, kind):
    c, d = BY_NAME[name], _state(name, dtype, kind)
    s, td = _stream(), U.torch_dtype(dtype)
    ops = {k: d[k] for k in U.EPILOGUES["all"]}
    want_out, _ = _filter(c, dtype, d["ii"], d["params"], False, c.Cs_out)
    want_gin, _ = _filter(c, dtype, d["iig"], U.reflected(d["params"]), True, c.Cs, ops)
    want_fg, offs = _param_grad(c, dtype, d)
    npix, plane = c.B * c.H * c.W, (c.H + 1) * (c.W + 1)
    x = U.to_nhwc(d["x"], c.Cs, dtype, pad=U.NAN).cuda()
    g = U.to_nhwc(d["g"], c.Cs_out, dtype, pad=U.NAN).cuda()
    dev = {k: U.to_nhwc(v, c.Cs, dtype, pad=(U.NAN if k.startswith("mask") else 0.0)).cuda() for k, v in ops.items() if k != "old"}
    pf, pr = d["params"].cuda(), U.reflected(d["params"]).cuda()
    ii, ii_g = U.Guarded(c.B * c.C * plane), U.Guarded(c.B * c.CF * plane)
    out = U.Guarded(npix * c.Cs_out, td)
    ws_ii = U.Guarded(int(L.load().msau_box_integral_ws_floats(c.B, c.H, c.W, c.CF)))
    ws = U.Guarded(int(L.load().msau_box_pgrad_ws_floats(c.B, c.H, c.W, c.C, c.F)))
    a = U.box_args(in_=x.data_ptr(), ii=ii.ptr(), params_fwd=pf.data_ptr(), params_refl=pr.data_ptr(), out=out.ptr(), ws_ii=ws_ii.ptr(),
                   B=c.B, H=c.H, W=c.W, C=c.C, F=c.F, Cs_in=c.Cs, Cs_out=c.Cs_out, relu_in=1, max_h=MAX_H, max_w=MAX_W,
                   off_hmin=offs[0], off_hmax=offs[1], off_wmin=offs[2], off_wmax=offs[3])
    L.call("msau_box_fwd", s, dtype, U.byref(a))
    torch.cuda.synchronize()
    assert torch.equal(ii.data, d["ii"].data) and torch.equal(out.data.cpu().view_as(want_out), want_out)
    for with_gin in (True, False):
        fg, gin = U.Guarded(want_fg.n), U.Guarded(npix * c.Cs, td, fill=U.to_nhwc(ops["old"], c.Cs, dtype))
        ii_g.full.fill_(U.NAN)
        a.gout, a.ii_g, a.ws, a.flat_grads = g.data_ptr(), ii_g.ptr(), ws.ptr(), fg.ptr()
        a.gin, a.accumulate = (gin.ptr() if with_gin else None), 1
        a.mask_a, a.add, a.mask_b = dev["mask_a"].data_ptr(), dev["add"].data_ptr(), dev["mask_b"].data_ptr()
        L.call("msau_box_bwd", s, dtype, U.byref(a))
        torch.cuda.synchronize()
        assert torch.equal(_gather(fg, offs, c.CF), _gather(want_fg, offs, c.CF))
        if with_gin:
            assert torch.equal(ii_g.data, d["iig"].data) and torch.equal(gin.data.cpu().view_as(want_gin), want_gin)
        else:
            assert bool(torch.isnan(ii_g.full).all()), "gin = NULL: only the parameter gradient runs"
        for b, what in ((ii, "ii"), (ii_g, "ii_g"), (out, "out"), (gin, "gin"), (ws_ii, "ws_ii"), (ws, "ws"), (fg, "flat_grads")):
            b.assert_guard(what)


@pytest.mark.parametrize("Cn,F", [(8, 3), (5, 3), (3, 1), (24, 3)])
def test_box_params_clamp_order_and_reflect_exactly(Cn, F):
    CF = Cn * F
    offs, n = _offsets(CF)
    gen = torch.Generator().manual_seed(CF)
    flat = torch.randn(n, generator=gen) * 0.8                        # a fifth beyond the max size, half of the pairs with max < min
    flat[offs[0]], flat[offs[1]] = 1.0, -1.0                          # exactly on the clamp, and inverted
    flat[offs[2] + 1], flat[offs[3] + 1] = -3.0, -2.0                 # both beyond it on the same side
    fwd, refl = U.Guarded(4 * CF), U.Guarded(4 * CF)
    fd = flat.cuda()
    L.call("msau_box_params", _stream(), fd.data_ptr(), *offs, Cn, F, MAX_H, MAX_W, fwd.ptr(), refl.ptr())
    torch.cuda.synchronize()
    want_f, want_r = U.box_params_ref(flat, offs, CF, MAX_H, MAX_W)
    assert torch.equal(fwd.data.cpu().view(4, CF), want_f) and torch.equal(refl.data.cpu().view(4, CF), want_r)
    assert bool((want_f[1] >= want_f[0]).all() and (want_f.abs()[:2] <= MAX_H).all() and (want_f.abs()[2:] <= MAX_W).all())
    fwd.assert_guard("params")
    refl.assert_guard("reflected params")
    assert torch.equal(fd.cpu(), flat)


def test_refusals_return_an_error_and_launch_nothing():
    lib, s = L.load(), _stream()
    big = 1 << 20                                                      # every buffer is large enough for the call it refuses
    src = torch.zeros(big, device="cuda")
    outs = [U.Guarded(big) for _ in range(3)]
    p = torch.zeros(4 * 512, device="cuda")
    a, b, w = (o.ptr() for o in outs)
    B, H, W = 1, 3, 5
    refused = [
        ("C > Cs", lib.msau_box_integral(s, L.F32, src.data_ptr(), a, w, B, H, W, 9, 8, 0)),
        ("Cs % 8", lib.msau_box_integral(s, L.F32, src.data_ptr(), a, w, B, H, W, 4, 4, 0)),
        ("integral LDS", lib.msau_box_integral(s, L.F32, src.data_ptr(), a, w, B, H, W, 304, 304, 0)),
        ("integral dtype", lib.msau_box_integral(s, 7, src.data_ptr(), a, w, B, H, W, 8, 8, 0)),
        ("Cs_out % 8", lib.msau_box_filter(s, L.F32, src.data_ptr(), p.data_ptr(), a, B, H, W, 4, 3, 12, 0, 0, None, None, None)),
        ("nout > Cs_out", lib.msau_box_filter(s, L.F32, src.data_ptr(), p.data_ptr(), a, B, H, W, 8, 3, 16, 0, 0, None, None, None)),
        ("nout > Cs_out, summed", lib.msau_box_filter(s, L.F32, src.data_ptr(), p.data_ptr(), a, B, H, W, 9, 3, 8, 1, 0, None, None, None)),
        ("filter LDS", lib.msau_box_filter(s, L.BF16, src.data_ptr(), p.data_ptr(), a, B, H, W, 80, 3, 240, 0, 0, None, None, None)),
        ("filter dtype", lib.msau_box_filter(s, 7, src.data_ptr(), p.data_ptr(), a, B, H, W, 8, 3, 24, 0, 0, None, None, None)),
        ("pgrad C * F > Cs_out", lib.msau_box_param_grad(s, L.F32, src.data_ptr(), p.data_ptr(), src.data_ptr(), w, b, 0, 24, 48, 72,
                                                         B, H, W, 8, 3, 16, 1.0, 1.0)),
        ("pgrad LDS", lib.msau_box_param_grad(s, L.F32, src.data_ptr(), p.data_ptr(), src.data_ptr(), w, b, 0, 232, 464, 696,
                                              B, H, W, 232, 1, 232, 1.0, 1.0)),
        ("pgrad dtype", lib.msau_box_param_grad(s, 7, src.data_ptr(), p.data_ptr(), src.data_ptr(), w, b, 0, 24, 48, 72,
                                                B, H, W, 8, 3, 24, 1.0, 1.0)),
        ("fwd null", lib.msau_box_fwd(s, L.F32, U.byref(U.box_args(B=B, H=H, W=W, C=8, F=3, Cs_in=8, Cs_out=24)))),
        ("bwd null", lib.msau_box_bwd(s, L.F32, U.byref(U.box_args(B=B, H=H, W=W, C=8, F=3, Cs_in=8, Cs_out=24)))),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for _, rc in refused), [(k, rc) for k, rc in refused if rc == 0]
    assert lib.msau_last_error()
    for o in outs:
        assert bool(torch.isnan(o.full).all()), "a refused call wrote to its outputs"


# ---- one training plan: every box launch on its own stored operands ---------------------------------------------------------------
def test_every_box_launch_of_a_bf16_training_step():
    """2 x 13 x 40 x 56, 3 stages (the configuration of test_box_gpu.py's restatement test), bf16 storage, one TrainEngine step.  A
    training plan gives every activation, every gradient and every forward integral image a buffer of its own (only the integral image
    of the output gradient is shared scratch), so after the step each BoxOp still holds what its launches read and wrote:
    op.ii against the stored x, y against op.ii and op.params[0], the four parameter gradients in eng.flat_grad against op.ii and
    y.grad.  Stored input gradients accumulate several contributions and are left to test_input_gradient_and_its_epilogue."""
    from msau_amd import BMSAUWrapper, TrainEngine
    from oracle import box_oracle as BO
    from oracle import msau_oracle as O
    cfg = dict(BO.DEFAULT_BOX_CFG, channels=13, n_class=5, featRoot=8, scale_space_num=3, num_box_convs=2, num_box_per_channels=3,
               max_box_sizes=7, num_blocks=3)
    sd = BO.init_params(cfg, seed=21)
    x, label = O.synthetic_batch(2, 13, 40, 56, 5, seed=22)
    m = BMSAUWrapper(13, 5, dict(scale_space_num=3, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3,
                                 num_box_convs=2, num_box_per_channels=3, max_box_sizes=7, dtype="bf16"))
    m.load_state_dict(sd)
    m = m.cuda()
    eng = TrainEngine(m)
    eng.step(x.cuda(), label.cuda())
    torch.cuda.synchronize()
    plan = m._plan_for_shape(2, 40, 56, torch.device("cuda", 0), True)
    mb, nchecked, worst = float(cfg["max_box_sizes"]), 0, {"ii": 0.0, "y": 0.0, "grad": 0.0}
    for op in plan.box_ops:
        xa, ya, B, F = op.x, op.y, plan.B, op.F
        xt = U.to_nchw(xa.data, xa.C)
        xt = torch.relu(xt) if op.relu_in else xt
        ii = op.ii.cpu().double().view(B, xa.C, xa.H + 1, xa.W + 1)
        P = U.integral(xt.abs())
        worst["ii"] = max(worst["ii"], U.check(ii, U.integral(xt), U.ii_bound("rand", P, xa.H, xa.W), f"{op.name}: ii"))
        params = op.params[0].cpu()
        v, mag = U.filter_from_ii(ii, params, xa.H, xa.W, U.fwd_planes(xa.C, F))
        got = U.to_nchw(ya.data, ya.C)
        assert float(ya.data[..., ya.C:].float().abs().sum()) == 0.0
        worst["y"] = max(worst["y"], U.check(got, v, U.filter_bound(mag, got, v, L.BF16), f"{op.name}: y"))
        if ya.grad is None or op.ws is None:
            continue
        g = U.to_nchw(ya.grad, ya.C)
        ref = U.param_grad(ii, params, g, mb, mb)
        S = U.param_grad(P, params, g.abs(), mb, mb, mag="terms")
        offs = [m._poff[f"{op.pname}.{nm}"] for nm in ("x_min", "x_max", "y_min", "y_max")]
        gotg = torch.stack([eng.flat_grad[o:o + xa.C * F].cpu() for o in offs])
        worst["grad"] = max(worst["grad"], U.check(gotg, ref, U.REL * S + U.ABS, f"{op.name}: parameter gradient"))
        nchecked += 1
    for k, v in worst.items():
        _report(f"plan, {k}", v)
    # 3 stages x (3 levels down + 2 levels up) blocks x 2 box convs, every one with a parameter gradient
    assert nchecked == len(plan.box_ops) == 3 * 5 * 2, (nchecked, len(plan.box_ops))
