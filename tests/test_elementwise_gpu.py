"""GPU: every kernel of msau_amd/csrc/elementwise.hip that touches a tensor, called through the C ABI on tensors the test lays
out itself (NHWC with Cs stored channels), element by element against the float64 references of tests/elementwise_util.py:
layout conversion, the LRN (every fast instance G x forward / backward x F075, the generic kernel with padded channels and
n != C), the 2x2 max pool forward and backward (every accumulate / mask / ELU / extent combination, positions supplied by the
test), extent copy, one-hot ids, and the second trip of every grid-stride loop.  tests/test_elementwise_cpu.py proves the
references and the bounds.  Each check prints `RATIO <group> <storage> <worst error / bound>` (profiles/elementwise_tests.md).

msau_channel_sum and msau_clip_adam_step: test_wgrad_gpu.py and test_optim_gpu.py."""
import pytest
import torch

from msau_amd import _lib as L
from tests import elementwise_util as U
from tests.test_launch_ulp_gpu import assert_rounded

pytestmark = pytest.mark.gpu

DT = [pytest.param(L.F32, id="f32"), pytest.param(L.BF16, id="bf16")]
TD = {L.F32: torch.float32, L.BF16: torch.bfloat16}
BITS = {L.F32: torch.int32, L.BF16: torch.int16}
TRIP = 4096 * 256                              # work items of one trip of a grid-stride loop (grid_for's cap x the workgroup)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(t, dtype):
    return t.to(TD[dtype]).cuda().contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.double().cpu()


def bits(t, dtype):
    return t.to(TD[dtype]).contiguous().view(BITS[dtype]).cpu()


def same_bits(got, ref, dtype, what):
    """`got`: device tensor in storage type; `ref`: CPU tensor whose values are exact in it"""
    torch.cuda.synchronize()
    g, r = bits(got, dtype), bits(ref, dtype)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = g != r
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def hold(group, dtype, got, ref, slack, what, mag=None):
    """fp32 storage: |got - ref| <= slack.  bf16 storage: assert_rounded, half a bf16 ulp on top of it."""
    bf = dtype == L.BF16
    print(f"RATIO {group} {'bf16' if bf else 'f32'} {U.worst_ratio(got, ref, slack, bf, mag):.4f}")
    if bf:
        assert_rounded(got, ref, slack, what, mag=mag)
        return
    d = (got - ref).abs()
    bad = d > slack + 1e-30
    if bad.any():
        i = int(torch.argmax((d / (slack + 1e-30)).flatten()))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the fp32 bound; worst: got "
                             f"{float(got.flatten()[i])!r} exact {float(ref.flatten()[i])!r} bound {float(slack.flatten()[i])!r}")


def padded(t, Cs, fill=0.0):
    out = torch.full(t.shape[:-1] + (Cs,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


# ---- LRN -------------------------------------------------------------------------------------------------------------------------
def run_lrn(dtype, x, dy, C, n, alpha, beta, k, fill=0.0):
    """x, dy: [npix, Cs] CPU (storage-exact values) -> (y, da) [npix, Cs] float64; the outputs start as garbage"""
    npix, Cs = x.shape
    xd, gd = dev(x, dtype), dev(dy, dtype)
    y, da = torch.full_like(xd, fill), torch.full_like(xd, fill)
    L.call("msau_lrn_fwd", stream(), dtype, xd.data_ptr(), y.data_ptr(), npix, C, Cs, n, alpha, beta, k)
    L.call("msau_lrn_bwd", stream(), dtype, xd.data_ptr(), gd.data_ptr(), da.data_ptr(), npix, C, Cs, n, alpha, beta, k)
    return host(y), host(da)


def check_lrn(group, dtype, x, dy, n, alpha, beta, k, fast, y, da, what):
    hold(group + "-fwd", dtype, y, U.lrn_fwd(x, n, alpha, beta, k), U.lrn_fwd_bound(x, n, alpha, beta, k, fast), what + " forward")
    hold(group + "-bwd", dtype, da, U.lrn_bwd(x, dy, n, alpha, beta, k), U.lrn_bwd_bound(x, dy, n, alpha, beta, k, fast), what + " backward")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("G", U.FAST_G)
def test_lrn_fast_every_instance(G, dtype):
    """C == Cs == n == 8 G.  (a) the reference's alpha = 1e-4; (b) alpha / n = 1, the F075 instances with a window error of order
    1; (c) beta = 0.5, k = 2: the exp / log instances.  Then all of a pixel's energy in channel 0, n/2 - 1, n/2, n - 1."""
    n = 8 * G
    for s in ("a", "b", "c"):
        alpha, beta, k, scale = U.setting(s, n)
        x, dy = U.lrn_inputs(U.NPIX, n, scale, seed=100 * n + n)
        y, da = run_lrn(dtype, x, dy, n, n, alpha, beta, k, fill=5.0)
        check_lrn(f"lrn-fast-{s}", dtype, x, dy, n, alpha, beta, k, True, y, da, f"G={G} setting {s}")
    for s in ("b", "c"):
        alpha, beta, k, _ = U.setting(s, n)
        x, dy = U.energy_inputs(5, n, seed=n)
        y, da = run_lrn(dtype, x, dy, n, n, alpha, beta, k, fill=5.0)
        check_lrn(f"lrn-fast-{s}-energy", dtype, x, dy, n, alpha, beta, k, True, y, da, f"G={G} setting {s}, energy in one channel")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,Cs,n", U.GENERIC)
def test_lrn_generic_padded_channels_and_any_n(C, Cs, n, dtype):
    """the padded channels of a and dy hold poison: the outputs' padded channels are exactly 0, the real ones do not depend on it"""
    for s in ("b", "c"):
        alpha, beta, k, scale = U.setting(s, n)
        x, dy = U.lrn_inputs(U.NPIX, C, scale, seed=100 * C + n)
        outs = []
        for poison in (7.0, -1024.0):
            y, da = run_lrn(dtype, padded(x, Cs, poison), padded(dy, Cs, -poison), C, n, alpha, beta, k, fill=5.0)
            assert float(y[:, C:].abs().sum()) == 0 and float(da[:, C:].abs().sum()) == 0, "padded output channels"
            outs.append((y[:, :C], da[:, :C]))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the poison reached a real channel"
        check_lrn(f"lrn-generic-{s}", dtype, x, dy, n, alpha, beta, k, False, outs[0][0], outs[0][1], f"C={C} Cs={Cs} n={n} setting {s}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,Cs,n", [(200, 256, 200), (256, 256, 7)])
def test_lrn_generic_refuses_more_than_128_stored_channels(C, Cs, n, dtype):
    x = dev(torch.ones(U.NPIX, Cs), dtype)
    out = torch.full_like(x, 5.0)
    with pytest.raises(L.MsauHipError, match="generic path"):
        L.call("msau_lrn_fwd", stream(), dtype, x.data_ptr(), out.data_ptr(), U.NPIX, C, Cs, n, 1.0, 0.75, 1.0)
    with pytest.raises(L.MsauHipError, match="generic path"):
        L.call("msau_lrn_bwd", stream(), dtype, x.data_ptr(), x.data_ptr(), out.data_ptr(), U.NPIX, C, Cs, n, 1.0, 0.75, 1.0)
    assert float((host(out) - 5.0).abs().max()) == 0, "a refused call launched"


@pytest.mark.parametrize("G", [1, 32])
def test_lrn_fast_second_trip(G):
    """npix * G = 2^20 + 37 G lanes: the second trip of the loop is a partial workgroup whose G-groups shuffle while the other
    lanes of their waves have left (bf16, setting (b), about 8 M elements)"""
    n = 8 * G
    npix = (TRIP + 37 * G) // G
    alpha, beta, k, scale = U.setting("b", n)
    x, dy = U.lrn_inputs(npix, n, scale, seed=G)
    y, da = run_lrn(L.BF16, x, dy, n, n, alpha, beta, k, fill=5.0)
    check_lrn("lrn-fast-second-trip", L.BF16, x, dy, n, alpha, beta, k, True, y, da, f"G={G} npix={npix}")


def test_lrn_generic_second_trip():
    C, Cs, n = 5, 8, 5
    npix = TRIP + 101
    alpha, beta, k, scale = U.setting("b", n)
    x, dy = U.lrn_inputs(npix, C, scale, seed=9)
    y, da = run_lrn(L.BF16, padded(x, Cs, 7.0), padded(dy, Cs, 7.0), C, n, alpha, beta, k, fill=5.0)
    assert float(y[:, C:].abs().sum()) == 0 and float(da[:, C:].abs().sum()) == 0
    check_lrn("lrn-generic-second-trip", L.BF16, x, dy, n, alpha, beta, k, False, y[:, :C], da[:, :C], f"npix={npix}")


# ---- max pool --------------------------------------------------------------------------------------------------------------------
def run_pool_fwd(dtype, x, with_idx=True):
    B, H, W, Cs = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xd = dev(x, dtype)
    y = torch.full((B, Ho, Wo, Cs), 5.0, dtype=TD[dtype], device="cuda")
    idx = torch.full((B, Ho, Wo, Cs), 77, dtype=torch.uint8, device="cuda")
    L.call("msau_maxpool2x2_fwd", stream(), dtype, xd.data_ptr(), y.data_ptr(), idx.data_ptr() if with_idx else None, B, H, W, Cs)
    torch.cuda.synchronize()
    return y, idx.cpu()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Cs", U.POOL_CS)
@pytest.mark.parametrize("H,W", U.POOL_HW)
def test_pool_forward_is_exact(H, W, Cs, dtype):
    """ties, +0 / -0 and negatives; y: the bits of the first maximum in row-major order of the zero-padded window, idx: its position"""
    B = 3
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for negative in (False, True):
        x = U.pool_input(B, H, W, Cs, seed=100 * H + 10 * W + Cs, negative=negative)
        ry, ridx = U.pool_fwd(x)
        y, idx = run_pool_fwd(dtype, x)
        same_bits(y, ry, dtype, "y")
        assert torch.equal(idx, ridx), "idx"
        y2, idx2 = run_pool_fwd(dtype, x, with_idx=False)
        same_bits(y2, ry, dtype, "y without idx")
        assert bool((idx2 == 77).all()), "idx == NULL wrote positions"
        if negative:                                     # the zero padding wins at the odd edges
            yb = bits(y, dtype)
            if W % 2:
                assert bool((yb[:, :, -1] == 0).all()) and bool((idx[:, :Ho - H % 2, -1] == 1).all())
            if H % 2:
                assert bool((yb[:, -1] == 0).all()) and bool((idx[:, -1, :Wo - W % 2] == 2).all())
            if H % 2 and W % 2:
                assert bool((idx[:, -1, -1] == 1).all())
            assert bool((yb[:, :H // 2, :W // 2] != 0).all())
    print("RATIO pool-fwd", "bf16" if dtype == L.BF16 else "f32", "equal")


def test_pool_forward_second_trip():
    B, H, W, Cs = 1, 2, 2 * (TRIP + 101) - 1, 8
    x = U.pool_input(B, H, W, Cs, seed=3)
    ry, ridx = U.pool_fwd(x)
    y, idx = run_pool_fwd(L.BF16, x)
    same_bits(y, ry, L.BF16, "y")
    assert torch.equal(idx, ridx)


MASK_RELU = (1.5, 0.25, 0.0, -0.0)
MASK_ELU = (1.5, 0.25, 0.0, -0.0, -0.5, -0.75, -0.99609375)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("H,W,Cs", [(h, w, c) for h, w in U.POOL_HW for c in U.POOL_CS] + [(4, 5, 8), (3, 513, 8), (5, 514, 8)])
def test_pool_backward_every_combination(H, W, Cs, dtype):
    """positions supplied by the test (every value 0..3 in every window, those in the padding included) x accumulate x mask NULL /
    ReLU output / ELU output x extent NULL / per sample.  (4, 5, 8): Wo * Cs / 8 = 3; (., 513 / 514, 8): 257, pooled rows straddle
    workgroups.  fp32 storage: the bits of the float32 evaluation in the kernel's order; bf16: correctly rounded."""
    B = 3
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Cs)
    gy = U.bf16_round(torch.randn(B, Ho, Wo, Cs, generator=g))
    idx = ((torch.arange(Cs).view(1, 1, 1, Cs) + torch.randint(0, 4, (B, Ho, Wo, 1), generator=g)) % 4).to(torch.uint8)
    old = U.bf16_round(torch.randn(B, H, W, Cs, generator=g))
    masks = {"none": None,
             "relu": torch.tensor(MASK_RELU, dtype=torch.float64)[torch.randint(0, len(MASK_RELU), (B, H, W, Cs), generator=g)],
             "elu": torch.tensor(MASK_ELU, dtype=torch.float64)[torch.randint(0, len(MASK_ELU), (B, H, W, Cs), generator=g)]}
    extent = U.pool_extents(B, H, W)
    gd, idxd, extd = dev(gy, dtype), idx.cuda(), extent.cuda()
    worst = 0.0
    for acc in (0, 1):
        for mname, mask in masks.items():
            for ext in (None, extent):
                dx = dev(old if acc else torch.full_like(old, 99.0), dtype)
                md = None if mask is None else dev(mask, dtype)
                flags = acc | (2 if mname == "elu" else 0)
                args = (stream(), dtype, gd.data_ptr(), idxd.data_ptr(), dx.data_ptr(), None if md is None else md.data_ptr(),
                        B, H, W, Cs, flags)
                if ext is None:
                    L.call("msau_maxpool2x2_bwd", *args)
                else:
                    L.call("msau_maxpool2x2_bwd_ext", *args, extd.data_ptr())
                what = f"accumulate={acc} mask={mname} extent={'yes' if ext is not None else 'no'}"
                if dtype == L.F32:
                    ref, _ = U.pool_bwd(gy.float(), idx, old.float() if acc else None, None if mask is None else mask.float(),
                                        mname == "elu", ext, H, W)
                    same_bits(dx, ref, dtype, what)
                else:
                    ref, slack = U.pool_bwd(gy, idx, old if acc else None, mask, mname == "elu", ext, H, W)
                    got = host(dx)
                    worst = max(worst, U.worst_ratio(got, ref, slack, True))
                    assert_rounded(got, ref, slack, what)
    print("RATIO pool-bwd", "bf16" if dtype == L.BF16 else "f32", f"{worst:.4f}" if dtype == L.BF16 else "equal")


# ---- layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("H,W", U.LAYOUT_HW)
@pytest.mark.parametrize("C,Cs", U.LAYOUT_CCS)
def test_layout_conversions(C, Cs, H, W, dtype):
    B, HW = 2, H * W
    g = torch.Generator().manual_seed(100 * C + HW)
    # NHWC -> NCHW fp32: exact; the padded channels of the source hold poison
    src = padded(U.bf16_round(torch.randn(B, HW, C, generator=g)), Cs, 7.0)
    srcd = dev(src, dtype)
    out = torch.full((B, C, HW), 5.0, device="cuda")
    L.call("msau_nhwc_to_nchw", stream(), dtype, srcd.data_ptr(), out.data_ptr(), B, C, Cs, H, W)
    same_bits(out, U.nhwc_to_nchw(src, C), L.F32, "nhwc_to_nchw")
    # NCHW fp32 gradient -> NHWC, written or accumulated; dst holds garbage in its padded channels
    gsrc = torch.randn(B, C, HW, generator=g).double()                      # full fp32 mantissas
    old = padded(U.bf16_round(torch.randn(B, HW, C, generator=g)), Cs, 7.0)
    gsd = gsrc.float().cuda()
    for acc in (0, 1):
        dst = dev(old, dtype)
        L.call("msau_nchw_grad_to_nhwc", stream(), dtype, gsd.data_ptr(), dst.data_ptr(), B, C, Cs, H, W, acc)
        got = host(dst)
        assert float(got[..., C:].abs().sum()) == 0, "padded channels"
        if dtype == L.F32:
            same_bits(dst, U.nchw_grad_to_nhwc(gsrc.float(), old.float() if acc else None, Cs), dtype, f"accumulate={acc}")
        else:
            ref = U.nchw_grad_to_nhwc(gsrc, old if acc else None, Cs)
            hold(f"nchw-grad-to-nhwc-acc{acc}", dtype, got, ref, 2.0 ** -24 * ref.abs(), f"accumulate={acc}")
    print("RATIO nhwc-to-nchw", "bf16" if dtype == L.BF16 else "f32", "equal")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel", ["plain", "register"])
def test_nchw_to_nhwc_second_trip(kernel, dtype):
    """plain kernel (Cs = 8): 2^20 + 101 work items; register kernel (Cs = 16, HW % 4 == 0): 2^20 + 100 threads, more than 4096
    workgroups and a partial last one"""
    B, C, Cs, H, W = (1, 5, 8, 1, TRIP + 101) if kernel == "plain" else (1, 9, 16, 4, TRIP // 2 + 50)
    HW = H * W
    src = torch.randn(B, C, HW, generator=torch.Generator().manual_seed(4))
    srcd = src.cuda()
    dst = torch.full((B, HW, Cs), 5.0, dtype=TD[dtype], device="cuda")
    L.call("msau_nchw_to_nhwc", stream(), dtype, srcd.data_ptr(), dst.data_ptr(), B, C, Cs, H, W)
    ref = torch.zeros(B, HW, Cs)
    ref[..., :C] = src.transpose(1, 2)
    same_bits(dst, ref.to(TD[dtype]), dtype, kernel)


@pytest.mark.parametrize("dtype", DT)
def test_nhwc_nchw_second_trip(dtype):
    B, C, Cs, H, W = 1, 5, 8, 1, TRIP + 101
    g = torch.Generator().manual_seed(5)
    src = padded(U.bf16_round(torch.randn(B, W, C, generator=g)), Cs, 7.0)
    srcd = dev(src, dtype)
    out = torch.full((B, C, W), 5.0, device="cuda")
    L.call("msau_nhwc_to_nchw", stream(), dtype, srcd.data_ptr(), out.data_ptr(), B, C, Cs, H, W)
    same_bits(out, U.nhwc_to_nchw(src, C), L.F32, "nhwc_to_nchw")
    gsrc = out                                                              # (bf16-exact values: the accumulated sum is exact in fp32)
    dst = dev(src, dtype)
    L.call("msau_nchw_grad_to_nhwc", stream(), dtype, gsrc.data_ptr(), dst.data_ptr(), B, C, Cs, H, W, 1)
    ref = U.nchw_grad_to_nhwc(U.nhwc_to_nchw(src, C), src, Cs)              # = 2 x: exact in both storage types
    same_bits(dst, ref, dtype, "nchw_grad_to_nhwc")


# ---- extent copy, one-hot ids ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in-place"])
@pytest.mark.parametrize("planes,pixel_bytes", [(1, 48), (1, 96), (1, 8), (5, 4)],
                         ids=["nhwc-bf16-Cs24", "nhwc-f32-Cs24", "int64-labels", "nchw-f32-C5"])
def test_extent_copy_bit_patterns(planes, pixel_bytes, in_place):
    """(0, 0), the full image, (h, W), (H, w) and an interior extent, one per sample; NaN, infinity and -0.0 patterns inside
    and outside: inside unchanged, outside all-zero words"""
    H, W = 7, 5
    ext = torch.tensor(U.extent_cases(H, W), dtype=torch.int32)
    B = ext.shape[0]
    words = U.extent_words(B, planes, H, W, pixel_bytes // 4, seed=planes + pixel_bytes)
    src = words.cuda()
    dst = src if in_place else torch.full_like(src, 0x55555555)
    L.call("msau_extent_copy", stream(), src.data_ptr(), dst.data_ptr(), B, planes, H, W, pixel_bytes, ext.cuda().data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), U.extent_copy(words, ext))
    if not in_place:
        assert torch.equal(src.cpu(), words)


def test_extent_copy_second_trip():
    B, planes, H, W = 3, 1, 1, (TRIP + 101) // 3                            # 2^20 + 101 = 3 x 349559 words
    assert B * W == TRIP + 101
    ext = torch.tensor([(0, 0), (1, W), (1, W // 2)], dtype=torch.int32)
    words = U.extent_words(B, planes, H, W, 1, seed=6)
    src = words.cuda()
    dst = torch.full_like(src, 0x55555555)
    L.call("msau_extent_copy", stream(), src.data_ptr(), dst.data_ptr(), B, planes, H, W, 4, ext.cuda().data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), U.extent_copy(words, ext))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,Cs", [(5, 8), (13, 16), (20, 32)])
def test_onehot_ids(C, Cs, dtype):
    """ids with -1, C - 1, C, Cs - 1 and large values among them, C < Cs; with and without extents"""
    B, H, W = 5, 7, 5
    ids = U.onehot_ids(B, H, W, C, Cs, seed=C)
    idd = ids.cuda()
    grid = torch.full((B, H, W, Cs), 5.0, dtype=TD[dtype], device="cuda")
    L.call("msau_onehot_ids", stream(), dtype, idd.data_ptr(), grid.data_ptr(), B * H * W, C, Cs)
    same_bits(grid, U.onehot(ids, C, Cs), dtype, "onehot_ids")
    ext = torch.tensor(U.extent_cases(H, W), dtype=torch.int32)
    grid.fill_(5.0)
    L.call("msau_onehot_ids_ext", stream(), dtype, idd.data_ptr(), grid.data_ptr(), B, H, W, C, Cs, ext.cuda().data_ptr())
    same_bits(grid, U.onehot(ids, C, Cs, ext), dtype, "onehot_ids_ext")


@pytest.mark.parametrize("dtype", DT)
def test_onehot_ids_second_trip(dtype):
    B, H, W, C, Cs = 3, 1, (TRIP + 101) // 3, 5, 8
    ids = U.onehot_ids(B, H, W, C, Cs, seed=7)
    idd = ids.cuda()
    grid = torch.full((B, H, W, Cs), 5.0, dtype=TD[dtype], device="cuda")
    L.call("msau_onehot_ids", stream(), dtype, idd.data_ptr(), grid.data_ptr(), B * H * W, C, Cs)
    same_bits(grid, U.onehot(ids, C, Cs), dtype, "onehot_ids")
    ext = torch.tensor([(0, 0), (1, W), (1, W // 2)], dtype=torch.int32)
    grid.fill_(5.0)
    L.call("msau_onehot_ids_ext", stream(), dtype, idd.data_ptr(), grid.data_ptr(), B, H, W, C, Cs, ext.cuda().data_ptr())
    same_bits(grid, U.onehot(ids, C, Cs, ext), dtype, "onehot_ids_ext")
