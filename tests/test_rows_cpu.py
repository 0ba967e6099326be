"""No GPU: what tests/rows_util.py states, proved.  (1) every float64 reference against torch.nn.functional / autograd; (2) the
claims behind the bit-exact `int` and `sparse` kinds; (3) the headroom of the `rand` bound: float32 evaluations in other summation
orders stay inside it; (4) the comparisons the GPU tests call reject eight defects a row kernel could really have; (5) every case
of the two instance tables is routed to the row family on every one of its shapes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from tests import elementwise_util as E
from tests import rows_util as U
from tests import wgrad_util as WU

f64 = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=f64)


def close(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max())), (what, float((a - b).abs().max()))


# ---- (1) the references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pad,cin,cout", [(1, 0, 16, 8), (3, 1, 8, 8), (3, 1, 16, 8), (3, 1, 16, 16), (4, 1, 8, 8), (4, 2, 8, 8)])
@pytest.mark.parametrize("hw", [(1, 1), (2, 5), (7, 9)])
def test_conv_reference_is_the_same_conv_as_torch(k, pad, cin, cout, hw):
    """SAME padding: `pad` before, k - 1 - pad after (the 4x4 conv: 1 / 2 forward, 2 / 1 for the flipped data-gradient image)"""
    x, w, b = rnd(2, *hw, cin, seed=1), rnd(cout, cin, k, k, seed=2), rnd(cout, seed=3)
    want = F.conv2d(F.pad(nchw(x), (pad, k - 1 - pad, pad, k - 1 - pad)), w, b)
    close(U.conv(x, w, b, (pad, pad)), nhwc(want), "conv")
    close(U.conv_mag(x, w, b, (pad, pad)), nhwc(F.conv2d(F.pad(nchw(x.abs()), (pad, k - 1 - pad, pad, k - 1 - pad)), w.abs(), b.abs())), "S")
    for order in U.orders(cin, k * k, 5):
        assert sorted(t for blk in order for t in blk) == [(t, c) for t in range(k * k) for c in range(cin)]
        got = U.conv(x, w, b, (pad, pad), order=order)
        assert float((got - nhwc(want)).abs().max()) < 1e-4


@pytest.mark.parametrize("cin", [16, 32])
@pytest.mark.parametrize("hw,odd", [((1, 1), (0, 0)), ((1, 3), (1, 1)), ((4, 5), (1, 0)), ((5, 4), (0, 1)), ((3, 3), (1, 1))])
def test_transposed_conv_reference_is_conv_transpose2d(cin, hw, odd):
    """ConvTranspose2d(k 3, stride 2, padding 1, output_padding = 1 - odd): the launch's weight is the flipped, transposed one"""
    x, wt, b = rnd(2, *hw, cin, seed=4), rnd(cin, cin // 2, 3, 3, seed=5), rnd(cin // 2, seed=6)
    Ho, Wo = 2 * hw[0] - odd[0], 2 * hw[1] - odd[1]
    want = F.conv_transpose2d(nchw(x), wt, b, stride=2, padding=1, output_padding=(1 - odd[0], 1 - odd[1]))
    assert tuple(want.shape[2:]) == (Ho, Wo)
    close(U.deconv(x, U.dgrad_weight(wt), b, Ho, Wo), nhwc(want), "deconv")


@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1), (4, 1)])
def test_two_output_data_gradient_is_autograd_of_the_conv_over_the_concat(k, pad):
    """g -> (dx1, dx2): the rows of the launch's weight are the channels of x1 (first half) and x2; the 4x4 conv's gradient is the
    flipped image with pad 2"""
    x = rnd(2, 16, 6, 7, seed=7).requires_grad_(True)
    w, g = rnd(8, 16, k, k, seed=8), rnd(2, 8, 6, 7, seed=9)
    F.conv2d(F.pad(x, (pad, k - 1 - pad, pad, k - 1 - pad)), w).backward(g)
    got = U.conv(nhwc(g), U.dgrad_weight(w), None, (k - 1 - pad, k - 1 - pad))
    close(got, nhwc(x.grad), "dgrad")


def _block(x, p):
    pre1 = F.conv2d(torch.relu(x), p["w1"], p["b1"], padding=1)
    mid = torch.relu(pre1)
    y = torch.relu(F.conv2d(mid, p["w2"], p["b2"], padding=1) + x)
    return pre1, mid, y


@pytest.mark.parametrize("Cc", [8, 16])
def test_pair_references_are_the_residual_block_and_its_chain_rule(Cc):
    """forward: mid, y, the coupling conv, the zero-padded pool.  Backward: through both ReLUs and the residual add -- the launch reads
    g = dL/dy already masked by (y > 0), as the plan hands it over"""
    B, H, W = 2, 5, 7
    p = {"w1": rnd(Cc, Cc, 3, 3, seed=1), "b1": rnd(Cc, seed=2), "w2": rnd(Cc, Cc, 3, 3, seed=3), "b2": rnd(Cc, seed=4),
         "wc": rnd(Cc, 2 * Cc, 1, 1, seed=5), "bc": rnd(Cc, seed=6)}
    x = rnd(B, Cc, H, W, seed=7).requires_grad_(True)
    prev, gy = rnd(B, Cc, H, W, seed=8), rnd(B, Cc, H, W, seed=9)
    pre1, mid, y = _block(x, p)
    pre1.retain_grad()
    (y * gy).sum().backward()
    xh = nhwc(x.detach())
    mid_r = U.relu(U.conv(U.relu(xh), p["w1"], p["b1"]))
    y_r = U.relu(U.conv(mid_r, p["w2"], p["b2"]) + xh)
    close(mid_r, nhwc(mid.detach()), "mid")
    close(y_r, nhwc(y.detach()), "y")
    z = torch.relu(F.conv2d(torch.cat([prev, y.detach()], 1), p["wc"], p["bc"]))
    z_r = U.relu(U.conv(torch.cat([nhwc(prev), y_r], -1), p["wc"], p["bc"], (0, 0)))
    close(z_r, nhwc(z), "z")
    py, pi = U.pool(z_r)
    close(py, nhwc(F.max_pool2d(F.pad(z, (0, W % 2, 0, H % 2)), 2, 2)), "pool")
    win = E.pool_windows(z_r)
    assert torch.equal(torch.gather(win, 0, pi.long()[None])[0], py)
    # backward
    g = nhwc(gy) * U.mask(y_r)
    gmid = U.conv(g, U.dgrad_weight(p["w2"])) * U.mask(mid_r)
    gx = U.conv(gmid, U.dgrad_weight(p["w1"])) * U.mask(xh) + g
    close(gmid, nhwc(pre1.grad), "gradient of mid")
    close(gx, nhwc(x.grad), "gradient of x")
    # the model of a launch, stage by stage, is the same chain with a bf16 store after each stage
    case = next(c for c in U.PAIR_CASES if c.C == Cc and c.cpl == 2 and c.bits)
    inp = dict(p, x=E.bf16_round(xh), prev=E.bf16_round(nhwc(prev)), g=E.bf16_round(g), lrn_a=E.bf16_round(xh))
    fwd = U.model_pair_fwd(case, inp)
    assert U.verify_pair_fwd(case, inp, fwd, "rand").max() <= 1.0


def test_slab_references_are_autograd_of_the_weights():
    B, H, W = 2, 6, 9
    x0, gmid = rnd(B, H, W, 8, seed=1), rnd(B, H, W, 8, seed=2)
    w = rnd(8, 8, 3, 3, seed=3).requires_grad_(True)
    b = torch.zeros(8, dtype=f64, requires_grad=True)
    F.conv2d(torch.relu(nchw(x0)), w, b, padding=1).backward(nchw(gmid))
    ref, S, m = U.wg1_reference(x0, gmid)
    assert ref.shape == (1, 8, 80) and int(m.sum()) == 73
    close(ref[0, :, :72].reshape(8, 9, 8), w.grad.permute(0, 2, 3, 1).reshape(8, 9, 8), "wg1 weight")
    close(ref[0, :, 72], b.grad, "wg1 bias")
    assert bool((S >= ref.abs() - 1e-12).all())
    prev, cur, g = rnd(B, H, W, 8, seed=4), rnd(B, H, W, 8, seed=5), rnd(B, H, W, 8, seed=6)
    wc = rnd(8, 16, 1, 1, seed=7).requires_grad_(True)
    bc = torch.zeros(8, dtype=f64, requires_grad=True)
    F.conv2d(torch.cat([nchw(prev), nchw(cur)], 1), wc, bc).backward(nchw(g))
    ref, S = U.rider_reference(prev, cur, g)
    assert ref.shape == (2, 8, 16)
    close(ref[0, :, :8], wc.grad[:, :8, 0, 0], "coupling weight, first source")
    close(ref[1, :, :8], wc.grad[:, 8:, 0, 0], "coupling weight, second source")
    close(ref[0, :, 8], bc.grad, "coupling bias")
    assert float(ref[1, :, 8].abs().max()) == 0 and float(ref[:, :, 9:].abs().max()) == 0


# ---- the geometry of a case on a shape (what the defects are modelled on) ---------------------------------------------------------------
def geometry(case, shp):
    """(strip width in output columns, segment height) as conv_rows.hip splits the launch"""
    env = dict(shp.env)
    if isinstance(case, U.PairCase):
        strip = 14 if case.c16 else 30
        sh = env.get(U.SH) or (env.get("MSAU_ROWS_SH16", 16) if case.c16 else 10)
        sh = min(sh, shp.H)
        if case.pooled and sh % 2 and sh < shp.H:
            sh += 1
        return strip, sh
    if case.kind != "conv8":
        return 32, 8
    trip = 8 if case.k == 4 else case.k + 3
    return 32, min(shp.H, -(-max(env.get(U.SH, 1), 8) // trip) * trip)


def run_model(case, shp, kind, mut=U.EXACT, order=None):
    """the device model of a case on a shape and the verification the GPU test applies to a launch -> the Report"""
    if isinstance(case, U.PairCase):
        inp = U.pair_inputs(case.C, shp.B, shp.H, shp.W, kind)
        fcase = case if not case.bwd else next(c for c in U.PAIR_CASES if c.C == case.C and not c.bwd and c.bits and not c.cpl and not c.pool)
        fwd = U.model_pair_fwd(fcase, inp, mut, order)
        if not case.bwd:
            rep = U.verify_pair_fwd(case, inp, fwd, kind)
            if case.bits:                  # the planes, as the GPU test checks them: the plain backward on this instance's planes
                U.verify_planes(rep, case, inp, fwd["mid"], U.model_pair_bwd(U.plain_bwd(case.C), inp, fwd, mut, order), kind)
            return rep, fwd
        plain = U.model_pair_bwd(dataclasses.replace(case, lrnb=False, wg1=False), inp, fwd, mut, order)
        got = U.model_pair_bwd(case, inp, fwd, mut, order)
        return U.verify_pair_bwd(case, inp, got, fwd["mid"], kind, dy=plain["y"], mid=plain["mid"]), got
    inp = U.conv_inputs(case, shp.B, shp.H, shp.W, kind)
    got = U.model_conv(case, shp, inp, mut, order)
    return U.verify_conv(case, shp, inp, got, kind), got


ALL = [(c, s) for c in U.PAIR_CASES + U.CONV_CASES for s in c.shapes]
ALL_IDS = [f"{c.name}-{s.id}" for c, s in ALL]


# ---- (2) the claims of the int and sparse kinds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,shp", ALL, ids=ALL_IDS)
def test_int_and_sparse_inputs_are_exact_in_every_order(case, shp):
    """every partial sum below 2^24 (`hold` asserts it from S, the sum of the magnitudes), every intermediate that passes through
    LDS in bf16 at most 256, and the exact model passes the GPU test's own verification"""
    for kind in ("int", "sparse"):
        rep, got = run_model(case, shp, kind)
        assert all(r == 0.0 for g, r in rep.worst.items() if not g.startswith("lrn")) and rep.max() <= 1.0      # (LRN outputs: a bound in every kind)
        if isinstance(case, U.PairCase) and "mid" in got:
            m = float(got["mid"].abs().max())
            assert m <= 256, m
            assert bool((got["mid"] == got["mid"].round()).all())


@pytest.mark.parametrize("Cc", [8, 16])
def test_sparse_inputs_pin_the_mask_convention_and_the_pool_order(Cc):
    """pre-activations of exactly 0 before each ReLU, and pool windows whose maximum is tied, on every shape with 8 pixels or more"""
    cases = [c for c in U.PAIR_CASES if c.C == Cc and not c.bwd and c.bits]
    seen = 0
    for shp in sorted({s for c in cases for s in c.shapes}, key=lambda s: s.id):
        if shp.B * shp.H * shp.W < 8:
            continue
        inp = U.pair_inputs(Cc, shp.B, shp.H, shp.W, "sparse")
        pre1 = U.conv(U.relu(inp["x"]), inp["w1"], inp["b1"])
        mid = U.store(U.relu(pre1))
        pre2 = U.conv(mid, inp["w2"], inp["b2"]) + inp["x"]
        y = U.store(U.relu(pre2))
        prez = U.conv(torch.cat([inp["prev"], y], -1), inp["wc"], inp["bc"], (0, 0))
        z = U.store(U.relu(prez))
        zeros = [int((t == 0).sum()) for t in (pre1, pre2, prez, inp["x"])]
        assert min(zeros) > 0, (shp.id, zeros)
        assert U.pool_ties(z) > 0 and U.pool_ties(y) > 0, shp.id
        seen += 1
    assert seen == {8: 13, 16: 9}[Cc], seen             # (all but 1x1x1, 2x1x2, 2x2x1: the list cannot shrink unnoticed)


# ---- (3) the headroom of the rand bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,shp", ALL, ids=ALL_IDS)
def test_float32_sums_in_other_orders_stay_inside_the_rand_bound(case, shp):
    """the condition that the reference ALONE passes: the launch's stages evaluated in float32, one product at a time, in three shuffled
    orders and in k-steps of 32, each stage rounded to bf16 -- inside half a bf16 ulp + ACC * S.  (An output element belongs to one
    strip and one segment: the task split does not divide its sum; the slab sums it does divide have their own test below.)"""
    worst = 0.0
    Ci = case.C if isinstance(case, U.PairCase) else case.cin * case.ns
    taps = 9 if isinstance(case, U.PairCase) else case.k * case.k
    for o1, oc in zip(U.orders(Ci, taps, 1), U.orders(2 * Ci, 1, 2)):
        rep, _ = run_model(case, shp, "rand", order=(o1, oc) if isinstance(case, U.PairCase) else o1)
        worst = max(worst, max((r for g, r in rep.worst.items() if not g.startswith("lrn")), default=0.0))
    print(f"HEADROOM {case.name} {shp.id} {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("which,B,H,W", [("wg1", 3, 10, 61), ("wg1", 2, 13, 61), ("rider", 2, 13, 33), ("rider", 2, 25, 65)])
def test_float32_slab_sums_split_by_task_stay_inside_the_slab_bound(which, B, H, W):
    """the riders' sums are split over workgroups by (sample, segment, strip): float32 partial sums per slab, added slab by slab, and
    three shuffled orders, against REL * S + ABS of wgrad_util"""
    inp = U.pair_inputs(8, B, H, W, "rand")
    if which == "wg1":
        c = WU.Case("wg1", L.BF16, WU.ROWS, 8, 8, 3, B=B, hw=(H, W), flags=L.CONV_RELU_IN)
        xt, g, elems, cch, strip, sh = U.relu(inp["x"]), inp["g"], [(0, 0, 0), (0, 3, 37), (0, 7, 71), (0, 5, 72)], 8, 30, 10
        ref, S, _ = U.wg1_reference(inp["x"], g)
    else:
        c = WU.Case("cplwg", L.BF16, WU.ROWS, 8, 8, 1, C2=8, B=B, hw=(H, W))
        xt, g, elems, cch, strip, sh = torch.cat([inp["prev"], inp["x"]], -1), inp["g"], [(0, 0, 0), (1, 3, 5), (0, 7, 8), (1, 7, 7)], 8, 32, 8
        ref, S = U.rider_reference(inp["prev"], inp["x"], g)
    t = WU.terms(c, xt, g, elems, cch)
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    nstrips, nseg = -(-W // strip), -(-H // sh)
    task = ((b * nseg + y // sh) * nstrips + x // strip).reshape(-1)
    ntasks = B * nseg * nstrips
    per_xcd = -(-(-(-ntasks // 8)) // 4) * 4
    slab = (task // per_xcd) + 8 * ((task % per_xcd) // 4)              # workgroup of a task: XCD + 8 * (its four-task group)
    sums = WU.fp32_orders(t.numpy(), slab, 8 * (per_xcd // 4))
    worst = 0.0
    for i, (ch, co, col) in enumerate(elems):
        bound = WU.REL * float(S[ch, co, col]) + WU.ABS
        worst = max(worst, float(np.abs(sums[:, i] - float(ref[ch, co, col])).max()) / bound)
    print(f"HEADROOM slabs-{which} {B}x{H}x{W} {worst:.4f}")
    assert worst <= 1.0


# ---- (4) the checker has teeth --------------------------------------------------------------------------------------------------------------
TEETH = [c for c in U.PAIR_CASES if c.name in ("c8-fwd-cplpool-bits", "c8-bwd-plain", "c16-fwd-pool-bits", "c16-bwd-plain")] + \
        [c for c in U.CONV_CASES if c.name in ("k3-plain", "k4-accum-maskb", "k1-dout-maskb2", "deconv8", "deconv16")]


def rejected(case, shp, kind, mut):
    try:
        run_model(case, shp, kind, mut)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", U.MUTATIONS)
def test_every_defect_is_rejected(name):
    """each defect, built into the device model, must fail the verification the GPU tests apply: on some shape of the list in the
    int or sparse kind, and -- unless it is a pure rounding defect -- in the rand kind too"""
    caught = {k: [] for k in U.KINDS}
    for case in TEETH:
        for shp in case.shapes:
            strip, sh = geometry(case, shp)
            mut = dataclasses.replace(U.EXACT, strip=strip, sh=sh, **{name: True})
            for kind in U.KINDS:
                if rejected(case, shp, kind, mut):
                    caught[kind].append(f"{case.name}-{shp.id}")
    for kind in U.KINDS:
        print(f"MUTATION {name} {kind}: {len(caught[kind])} (case, shape) pairs reject it, e.g. {caught[kind][:3]}")
    assert caught["int"] or caught["sparse"], name
    assert caught["rand"] or name in U.ROUNDING_ONLY, name
    if name in ("mask_ge", "pool_last"):
        assert caught["sparse"], name                       # what the sparse kind is there for
    if name == "mask_ge":                                   # a wrong ballot plane of a coupled / pooled forward instance: through verify_planes
        assert all(any(c.startswith(f) for k in U.KINDS for c in caught[k]) for f in ("c8-fwd-cplpool-bits", "c16-fwd-pool-bits")), caught


def test_the_exact_model_is_rejected_nowhere():
    for case in TEETH:
        for shp in case.shapes:
            for kind in U.KINDS:
                assert not rejected(case, shp, kind, U.EXACT), (case.name, shp.id, kind)


# ---- (5) routing ----------------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_are_the_instance_tables():
    assert len(U.PAIR_CASES) == 20 and len({c.flag_set for c in U.PAIR_CASES}) == 20 and len({c.name for c in U.PAIR_CASES}) == 20
    assert len(U.CONV_CASES) == 14 and len({c.flag_set for c in U.CONV_CASES}) == 14 and len({c.name for c in U.CONV_CASES}) == 14
    assert sum(c.c16 for c in U.PAIR_CASES) == 10 and sum(c.bwd for c in U.PAIR_CASES) == 6
    for shapes in (U.PAIR8_SHAPES, U.POOL8_SHAPES, U.PAIR16_SHAPES, U.POOL16_SHAPES, U.CONV8_SHAPES, U.DECONV_SHAPES):
        assert all(s.B <= 3 and s.H <= 25 and s.W <= 65 and s.why for s in shapes)


@pytest.mark.parametrize("case,shp", ALL, ids=ALL_IDS)
def test_every_case_is_taken_by_the_row_family_on_every_shape(case, shp):
    lib = L.load()
    pair = isinstance(case, U.PairCase)
    d = U.fake_pointers(case, U.pair_desc(case, shp) if pair else U.conv_desc(case, shp))
    with U.rows_env(**shp.switches):
        if pair:
            assert U.pair_route(d) == 2 and lib.msau_conv_pair_applicable(L.BF16, C.byref(d)) == 1
            assert int(lib.msau_conv_pair_bits_bytes(L.BF16, C.byref(d))) == shp.B * shp.H * -(-shp.W // (14 if case.c16 else 30)) * 32
            assert (lib.msau_conv_pair_wgrad_slabs(L.BF16, C.byref(d)) > 0) == case.wg1
        else:
            rc, info = U.conv_route(d)
            assert rc == 0 and info[6] == 3, info
            assert (lib.msau_conv2d_rider_slabs(L.BF16, C.byref(d)) > 0) == case.wg
            g = U.conv_geometry(case)
            assert (g.kchunk, g.rows) == {"conv8": (-(-case.k * case.k * 8 // 32) * 32, 16), "deconv8": (160, 16), "deconv16": (288, 16)}[case.kind]
    with U.rows_env(**dict(shp.switches, MSAU_PAIR_ROWS=0)):
        if pair:
            assert U.pair_route(d) != 2
        else:
            assert U.conv_route(d)[1][6] != 3


def test_rows_env_restores_the_environment():
    import os
    os.environ["MSAU_ROWS_SH"] = "7"
    try:
        with U.rows_env(MSAU_ROWS_MIN_TASKS=1):
            assert "MSAU_ROWS_SH" not in os.environ and os.environ["MSAU_ROWS_MIN_TASKS"] == "1"
        assert os.environ["MSAU_ROWS_SH"] == "7" and "MSAU_ROWS_MIN_TASKS" not in os.environ
    finally:
        del os.environ["MSAU_ROWS_SH"]
        L.load().msau_reload_env()
