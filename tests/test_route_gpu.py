"""conv2d routing on the device: for every instance family the smallest descriptor the router sends there and its neighbour just
across the threshold, launched through msau_conv2d -- the family msau_conv2d_launch_info names, and the output against a float64
reference.  Every <family>_launch switch runs with a case number handed over by the router, where the two could disagree."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from tests.test_launch_ulp_gpu import ACC, assert_rounded

pytestmark = pytest.mark.gpu
TILE, LEAN, CHUNKED, ROWS = 0, 1, 2, 3

#        what                    B  Hin Win  C1  Cout k ups head  family
CASES = [("rows 3x3",            2, 64, 32,   8,  8, 3, 1, False, ROWS),        # 16 tasks = MSAU_ROWS_MIN_TASKS
         ("rows 3x3, below",     2, 56, 32,   8,  8, 3, 1, False, TILE),
         ("lean 3x3",            1, 128, 128, 16, 16, 3, 1, False, LEAN),       # 64 tiles
         ("lean 3x3, below",     1, 128, 112, 16, 16, 3, 1, False, TILE),       # 56 tiles
         ("chunked",             1, 128, 128, 768, 8, 3, 1, False, CHUNKED),
         ("chunked, below",      1, 64, 64,  768,  8, 3, 1, False, TILE),       # 16 tiles
         ("4x4",                 1, 128, 128,  8,  8, 4, 1, False, ROWS),
         ("4x4 with the head",   1, 128, 128,  8,  8, 4, 1, True, LEAN),
         ("deconv, rows",        2, 32, 32,   16,  8, 3, 2, False, ROWS),
         ("deconv, below",       1, 16, 16,   16,  8, 3, 2, False, TILE)]


@pytest.mark.parametrize("what,B,Hin,Win,C1,Cout,k,ups,head,family", CASES, ids=[c[0] for c in CASES])
def test_routed_launch(what, B, Hin, Win, C1, Cout, k, ups, head, family):
    dev = torch.device("cuda")
    lib = L.load()
    lib.msau_reload_env()
    g = torch.Generator(device="cpu").manual_seed(Hin * 1000 + Win + C1)
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(B, Hin, Win, C1, generator=g))
    w = bf(torch.randn(Cout, C1, k, k, generator=g) * (k * k * C1) ** -0.5)
    bias = torch.randn(16, generator=g)
    Hout, Wout = Hin * ups, Win * ups
    pad = (k - 1) // 2 if ups == 1 else 1
    # the packed image: [chunk][16 rows][tap][channel of the chunk], k padded to a multiple of 32; rows = output channels (one 16-row tile)
    geom = L.ConvPackGeom()
    L.call("msau_conv_pack_geometry", L.BF16, C1, 0, Cout, k, k, 1, 1, ups, C.byref(geom))
    assert geom.rows == 16 and geom.cch * geom.nchunks == C1
    wp = torch.zeros(geom.nchunks, 16, geom.kchunk, dtype=torch.bfloat16)
    for c in range(geom.nchunks):
        wp[c, :Cout, :k * k * geom.cch] = w[:, c * geom.cch:(c + 1) * geom.cch].permute(0, 2, 3, 1).reshape(Cout, -1)
    xd, wpd, bd = x.to(dev), wp.to(dev), bias.to(dev)
    y = torch.full((B, Hout, Wout, Cout), 7.0, device=dev, dtype=torch.bfloat16)
    d = L.ConvDesc()
    d.B, d.Hin, d.Win, d.Hout, d.Wout = B, Hin, Win, Hout, Wout
    d.C1, d.C2, d.Cout, d.KH, d.KW = C1, 0, Cout, k, k
    d.dil, d.pad_t, d.pad_l, d.stride, d.ups = 1, pad, pad, 1, ups
    d.x1, d.wpack, d.bias, d.y = xd.data_ptr(), wpd.data_ptr(), bd.data_ptr(), y.data_ptr()
    if head:
        probs = torch.full((B, Hout, Wout, 5), 7.0, device=dev)
        amax = torch.full((B, Hout, Wout), 77, device=dev, dtype=torch.uint8)
        d.flags, d.head_probs, d.head_argmax, d.head_classes = L.CONV_HEAD, probs.data_ptr(), amax.data_ptr(), 5
    info = (L.i32 * 8)()
    L.call("msau_conv2d_launch_info", L.BF16, C.byref(d), info)
    assert info[6] == family, list(info)
    L.call("msau_conv2d", torch.cuda.current_stream().cuda_stream, L.BF16, C.byref(d))
    torch.cuda.synchronize()
    # float64: v = sum in(oy + ky - pad, ox + kx - pad, c) W[co][tap][c] + bias; ups = 2: `in` is the zero-stuffed image
    xi = x.double().permute(0, 3, 1, 2)
    if ups == 2:
        st = torch.zeros(B, C1, 2 * Hin, 2 * Win, dtype=torch.float64)
        st[:, :, ::2, ::2] = xi
        xi = st
    xi = F.pad(xi, (pad, k - 1 - pad, pad, k - 1 - pad))
    ref = F.conv2d(xi, w.double(), bias[:Cout].double())
    mag = F.conv2d(xi.abs(), w.double().abs(), bias[:Cout].double().abs())
    got = y.double().cpu().permute(0, 3, 1, 2)
    assert_rounded(got, ref, ACC * mag, what)
    if head:
        pref = torch.softmax(got[:, :5], dim=1)                          # of the storage-rounded result
        pgot = probs.double().cpu().permute(0, 3, 1, 2)
        assert_rounded(pgot, pref, 0.0, what + ": head_probs")
        assert torch.equal(amax.cpu().long(), pgot.argmax(dim=1))
