"""GPU: every instance of the row-streaming family (ROWPAIR_TABLE, ROWCONV_TABLE of msau_amd/csrc/conv_rows.hip) called through the C
ABI (msau_conv_pair, msau_conv2d) on tensors this file lays out itself, every output element against the float64 references of
tests/rows_util.py: bit for bit on the `int` and `sparse` inputs, within half a bf16 ulp + ACC * S on the `rand` ones.  Inputs sit
between NaN images, outputs start as poison between guard images, the planes and slabs between guard bands; what an instance must
leave alone is asserted untouched.  A case whose route leaves the row family FAILS.  tests/test_rows_cpu.py proves the references,
the bounds and that these comparisons reject the defects a row kernel could have."""
import ctypes as C
import dataclasses

import pytest
import torch

from msau_amd import _lib as L
from tests import rows_util as U
from tests import wgrad_util as WU

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_bias(b):
    """fp32 [16], zero beyond the real channels (as msau_pack_params writes it)"""
    out = torch.zeros(16, dtype=torch.float32)
    out[:b.numel()] = b.float()
    return out.cuda()


def dev_w(w, C1, C2, ups=1):
    return U.pack_image(w, C1, C2, ups)[0].cuda()


FWD_PLAIN_BITS = {Cc: next(c for c in U.PAIR_CASES if c.C == Cc and not c.bwd and c.bits and not c.cpl and not c.pool) for Cc in (8, 16)}


def run_pair_fwd(case, shp, inp, plane_fill=0x00, null_idx=False):
    """one forward launch -> (outputs on the host, the two planes or None)"""
    lib, (B, H, W, Cc) = L.load(), (shp.B, shp.H, shp.W, case.C)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = U.dev_in(inp["x"])
    keep = [x, dev_w(inp["w1"], Cc, 0), dev_bias(inp["b1"]), dev_w(inp["w2"], Cc, 0), dev_bias(inp["b2"])]
    out = {"mid": U.dev_out(B, (H, W, Cc)), "y": U.dev_out(B, (H, W, Cc))}
    d = U.pair_desc(case, shp, x=U.ptr(x), add=U.ptr(x), w1=keep[1].data_ptr(), b1=keep[2].data_ptr(), mid=U.ptr(out["mid"]),
                    w2=keep[3].data_ptr(), b2=keep[4].data_ptr(), y=U.ptr(out["y"]))
    idx = None
    if case.cpl:
        keep += [U.dev_in(inp["prev"]), dev_w(inp["wc"], Cc, Cc), dev_bias(inp["bc"])]
        out["z"] = U.dev_out(B, (H, W, Cc))
        d.cpl_prev, d.cpl_w, d.cpl_b, d.cpl_y = U.ptr(keep[-3]), keep[-2].data_ptr(), keep[-1].data_ptr(), U.ptr(out["z"])
    if case.pooled:
        out["pool"], idx = U.dev_out(B, (Ho, Wo, Cc)), U.dev_out(B, (Ho, Wo, Cc), torch.uint8)
        py, pi = U.ptr(out["pool"]), (None if null_idx else U.ptr(idx))
        if case.cpl == 2:
            d.cpl_pool_y, d.cpl_pool_idx = py, pi
        else:
            d.pool_y, d.pool_idx = py, pi
    planes = None
    if case.bits:
        nbytes = int(lib.msau_conv_pair_bits_bytes(L.BF16, C.byref(d)))
        assert nbytes == B * H * -(-W // (14 if case.c16 else 30)) * 32
        planes = (U.plane_buffer(nbytes, plane_fill), U.plane_buffer(nbytes, plane_fill))
        d.bits_mid, d.bits_a = U.plane_ptr(planes[0]), U.plane_ptr(planes[1])
    assert U.pair_route(d) == 2, "the case left the row family"
    L.check(lib.msau_conv_pair(stream(), L.BF16, C.byref(d)), case.name)
    torch.cuda.synchronize()
    got = {k: U.take(v, f"{case.name} {k}") for k, v in out.items()}
    if idx is not None:
        if null_idx:
            U.untouched(idx, "pool positions (NULL was passed)")
        else:
            got["pool_idx"] = U.take(idx, "pool positions")
    if planes is not None:
        planes = tuple(U.plane_take(p, plane_fill, f"{case.name} plane {i}").clone() for i, p in enumerate(planes))
    return got, planes


def run_pair_bwd(case, shp, inp, planes):
    """one data-gradient launch on the planes a forward launch wrote -> (outputs on the host, (slab buffer, slab count) or None)"""
    lib, (B, H, W, Cc) = L.load(), (shp.B, shp.H, shp.W, case.C)
    g = U.dev_in(inp["g"])
    keep = [g, dev_w(U.dgrad_weight(inp["w2"]), Cc, 0), dev_w(U.dgrad_weight(inp["w1"]), Cc, 0)]
    pl = [torch.cat([torch.zeros(U.PLANE_GUARD, dtype=torch.uint8, device="cuda"), p, torch.zeros(U.PLANE_GUARD, dtype=torch.uint8, device="cuda")]) for p in planes]
    out = {"mid": U.dev_out(B, (H, W, Cc)), "y": U.dev_out(B, (H, W, Cc))}
    d = U.pair_desc(case, shp, x=U.ptr(g), add=U.ptr(g), w1=keep[1].data_ptr(), mid=U.ptr(out["mid"]), w2=keep[2].data_ptr(), y=U.ptr(out["y"]),
                    bits_mid=U.plane_ptr(pl[0]), bits_a=U.plane_ptr(pl[1]))
    if case.lrnb:
        keep.append(U.dev_in(inp["lrn_a"]))
        out["lrn_da"] = U.dev_out(B, (H, W, Cc))
        d.lrn_a, d.lrn_da = U.ptr(keep[-1]), U.ptr(out["lrn_da"])
    slabs = None
    if case.wg1:
        keep.append(U.dev_in(inp["x"]))
        d.wg1_x = d.wg1_slabs = U.ptr(keep[-1])                        # (the slab count is asked of a descriptor that has its operands)
        n = int(lib.msau_conv_pair_wgrad_slabs(L.BF16, C.byref(d)))
        assert n > 0
        full, part = U.slab_buffer(n, 8 * 80)
        d.wg1_slabs, d.wg1_nslabs = part.data_ptr(), n
        slabs = (full, part, n)
    assert U.pair_route(d) == 2, "the case left the row family"
    L.check(lib.msau_conv_pair(stream(), L.BF16, C.byref(d)), case.name)
    torch.cuda.synchronize()
    for p, q in zip(pl, planes):
        assert torch.equal(p[U.PLANE_GUARD:-U.PLANE_GUARD], q) and not bool(p[:U.PLANE_GUARD].any()) and not bool(p[-U.PLANE_GUARD:].any()), "the backward wrote a plane"
    if case.lrnb:
        U.untouched(out.pop("y"), "y under MSAU_PAIR_LRN_BWD")
    if case.wg1:
        U.untouched(out.pop("mid"), "mid under MSAU_PAIR_WGRAD1")
        assert bool(torch.isnan(slabs[0][:WU.GUARD]).all()), "the guard band before the slabs was written"
    return {k: U.take(v, f"{case.name} {k}") for k, v in out.items()}, slabs


def run_conv(case, shp, inp):
    """one msau_conv2d launch -> (outputs on the host, (slab buffer, slab count) or None)"""
    lib, B = L.load(), shp.B
    Ho, Wo = shp.out_hw if case.kind != "conv8" else (shp.H, shp.W)
    keep = [U.dev_in(inp["x1"]), dev_w(inp["w"], case.cin, 8 if case.ns == 2 else 0, 1 if case.kind == "conv8" else 2)]
    cy = 8 if case.kind == "conv8" else case.cout
    out = {"y": U.dev_out(B, (Ho, Wo, cy), init=inp["y_old"] if case.epi & L.CONV_ACCUM else None)}
    d = U.conv_desc(case, shp, x1=U.ptr(keep[0]), wpack=keep[1].data_ptr(), y=U.ptr(out["y"]))
    if inp["b"] is not None:
        keep.append(dev_bias(inp["b"]))
        d.bias = keep[-1].data_ptr()
    if case.ns == 2:
        keep.append(U.dev_in(inp["x2"]))
        d.x2 = U.ptr(keep[-1])
    if case.dout or case.epi & L.CONV_LRN:
        out["y2"] = U.dev_out(B, (Ho, Wo, 8))
        d.y2 = U.ptr(out["y2"])
    if case.epi & L.CONV_MASK_B:
        keep.append(U.dev_in(inp["mask_b"]))
        d.mask_b = U.ptr(keep[-1])
    if case.epi2 & L.CONV_MASK_B:
        keep.append(U.dev_in(inp["mask_b2"]))
        d.mask_b2 = U.ptr(keep[-1])
    slabs = None
    if case.wg:
        keep.append(U.dev_in(inp["wg_x1"]))
        d.wg_x1 = d.wg_slabs = U.ptr(keep[-1])
        n = int(lib.msau_conv2d_rider_slabs(L.BF16, C.byref(d)))
        assert n > 0
        full, part = U.slab_buffer(n, 2 * 8 * 16)
        d.wg_slabs, d.wg_nslabs = part.data_ptr(), n
        slabs = (full, part, n)
    rc, info = U.conv_route(d)
    assert rc == 0 and info[6] == 3, f"the case left the row family: {info}"
    L.check(lib.msau_conv2d(stream(), L.BF16, C.byref(d)), case.name)
    torch.cuda.synchronize()
    if slabs is not None:
        assert bool(torch.isnan(slabs[0][:WU.GUARD]).all()), "the guard band before the slabs was written"
    return {k: U.take(v, f"{case.name} {k}") for k, v in out.items()}, slabs


COUPLING_ALONE = next(c for c in U.CONV_CASES if c.name == "k1-dual-relu")


def _pair(case, shp, kind):
    inp = U.pair_inputs(case.C, shp.B, shp.H, shp.W, kind)
    with U.rows_env(**shp.switches):
        if not case.bwd:
            got, planes = run_pair_fwd(case, shp, inp)
            rep = U.verify_pair_fwd(case, inp, got, kind)
            if case.bits:
                # the same launch over planes that start as 0xFF: equal planes <=> every byte of them is written
                got2, planes2 = run_pair_fwd(case, shp, inp, plane_fill=0xFF)
                assert all(torch.equal(a, b) for a, b in zip(planes, planes2)), "a plane byte is not written"
                assert all(torch.equal(got[k], got2[k]) for k in got), "the launch is not deterministic"
                # ... and their values: the plain data-gradient launch on THIS instance's planes gives the gradients masked by
                # (stored mid > 0) and (x > 0), element by element
                bgot, _ = run_pair_bwd(U.plain_bwd(case.C), shp, inp, planes)
                U.verify_planes(rep, case, inp, got["mid"], bgot, kind)
            if case.pooled:
                got3, _ = run_pair_fwd(case, shp, inp, null_idx=True)
                assert all(torch.equal(got[k], got3[k]) for k in got3), "outputs change when the positions are not asked for"
            if case.cpl and not case.c16:
                # the kernel's promise: z is the stand-alone rowconv8<2, 1, 1, RELU_OUT> launch on the stored y, bit for bit
                alone, _ = run_conv(COUPLING_ALONE, shp, {"x1": inp["prev"], "x2": got["y"], "w": inp["wc"], "b": inp["bc"]})
                assert torch.equal(alone["y"], got["z"]), "z differs from the stand-alone coupling launch"
        else:
            fgot, planes = run_pair_fwd(FWD_PLAIN_BITS[case.C], shp, inp)
            pgot = None
            if case.lrnb or case.wg1:
                pgot, _ = run_pair_bwd(dataclasses.replace(case, lrnb=False, wg1=False), shp, inp, planes)
            got, slabs = run_pair_bwd(case, shp, inp, planes)
            rep = U.verify_pair_bwd(case, inp, got, fgot["mid"], kind, dy=pgot and pgot["y"], mid=pgot and pgot["mid"])
            if case.wg1:
                # the rider changes no data gradient: bit-identical to the same launch without it
                twin, _ = run_pair_bwd(dataclasses.replace(case, wg1=False), shp, inp, planes)
                key = "lrn_da" if case.lrnb else "y"
                assert torch.equal(got[key], twin[key]), f"{key} changes with the weight-gradient rider"
                ref, S, m = U.wg1_reference(inp["x"], pgot["mid"])
                _, part, n = slabs
                rep.add("slabs", WU.check_slabs(part, n, ref.cuda(), S.cuda(), m.cuda(), U.slab_kind(kind), f"{case.name} slabs"))
    rep.show(case.name)


@pytest.mark.parametrize("case,shp,kind", U.params(U.PAIR_CASES, lambda c: not c.c16))
def test_rowpair_c8(case, shp, kind):
    """rowpair_c8_kernel<BWD, BITS, LRNB, WG1, CPL>: the ten 8-channel rows of ROWPAIR_TABLE"""
    _pair(case, shp, kind)


@pytest.mark.parametrize("case,shp,kind", U.params(U.PAIR_CASES, lambda c: c.c16))
def test_rowpair_c16(case, shp, kind):
    """rowpair_c16_kernel<BWD, BITS, POOL, CPL, LRNB>: the ten 16-channel rows of ROWPAIR_TABLE"""
    _pair(case, shp, kind)


def _conv(case, shp, kind):
    inp = U.conv_inputs(case, shp.B, shp.H, shp.W, kind)
    with U.rows_env(**shp.switches):
        got, slabs = run_conv(case, shp, inp)
        rep = U.verify_conv(case, shp, inp, got, kind)
        if case.wg:
            twin, _ = run_conv(dataclasses.replace(case, wg=False), shp, inp)
            assert torch.equal(got["y"], twin["y"]) and torch.equal(got["y2"], twin["y2"]), "a data gradient changes with the weight-gradient rider"
            ref, S = U.rider_reference(inp["wg_x1"], inp["mask_b2"], inp["x1"])
            _, part, n = slabs
            rep.add("slabs", U.check_rider_slabs(part, n, ref, S, U.slab_kind(kind), f"{case.name} slabs"))
    rep.show(case.name)


@pytest.mark.parametrize("case,shp,kind", U.params(U.CONV_CASES, lambda c: c.kind == "conv8"))
def test_rowconv8(case, shp, kind):
    """rowconv8_kernel<NS, KH, KW, EPI, EPI2, WG>: the twelve rows of ROWCONV_TABLE it has (the 4x4 ones with pad 1 and pad 2)"""
    _conv(case, shp, kind)


@pytest.mark.parametrize("case,shp,kind", U.params(U.CONV_CASES, lambda c: c.kind == "deconv8"))
def test_rowdeconv8(case, shp, kind):
    """rowdeconv8_kernel: 16 -> 8 channels, all four parities of the output size"""
    _conv(case, shp, kind)


@pytest.mark.parametrize("case,shp,kind", U.params(U.CONV_CASES, lambda c: c.kind == "deconv16"))
def test_rowdeconv16(case, shp, kind):
    """rowdeconv16_kernel: 32 -> 16 channels"""
    _conv(case, shp, kind)
