"""Ragged batches on the CPU: the exactness argument of DESIGN.md "Ragged batches" in float64 with the reference's op definitions,
the per-level extents, the pack / unpack / batches helpers, host-side validation of `sizes` and the ABI of the extent flag."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from msau_amd.data.ragged import batches, pack, padded_fraction, unpack
from msau_amd.plan import Plan, same_pads

DOCS = [(7, 5), (8, 8), (9, 6), (6, 11), (1, 1), (13, 13)]        # odd and even h and w
CANVAS = (16, 16)


def _place(doc: torch.Tensor, H: int, W: int) -> torch.Tensor:
    out = torch.zeros(doc.shape[:-2] + (H, W), dtype=doc.dtype)
    out[..., :doc.shape[-2], :doc.shape[-1]] = doc
    return out


def _same_conv(x, w, b, dil):
    """SAME conv as the reference writes it: utils.pad_2d (TF padding, model/layers/utils.py) + Conv2d"""
    k = w.shape[-1]
    pt, pb = same_pads(x.shape[-2], k, 1, dil)
    pl, pr = same_pads(x.shape[-1], k, 1, dil)
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b, dilation=dil)


def _pool(x):
    """2x2 max pool after zero SAME padding (bottom / right only: model/model.py:158-160)"""
    H, W = x.shape[-2:]
    return F.max_pool2d(F.pad(x, (0, W % 2, 0, H % 2)), 2, 2)


def _deconv(x, w, b, out_hw):
    """ConvTranspose2d(k3, s2, p1)(x, output_size=out_hw) (model/layers/layers.py:249-250)"""
    op = [o - ((i - 1) * 2 - 2 + 3) for o, i in zip(out_hw, x.shape[-2:])]
    return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=tuple(op))


@pytest.mark.parametrize("h,w", DOCS)
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 8), (1, 1), (4, 1)])
def test_same_conv_on_a_zero_extended_canvas_is_the_document_conv(h, w, k, dil):
    g = torch.Generator().manual_seed(h * 100 + w + k * 7 + dil)
    x = torch.randn((1, 3, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((4, 3, k, k), generator=g, dtype=torch.float64)
    b = torch.randn((4,), generator=g, dtype=torch.float64)
    alone = _same_conv(x, wt, b, dil)
    canvas = _same_conv(_place(x, *CANVAS), wt, b, dil)
    assert tuple(alone.shape[-2:]) == (h, w)
    torch.testing.assert_close(canvas[..., :h, :w], alone, rtol=1e-12, atol=1e-12)
    # (the bias makes the canvas non-zero beyond the document: what the extent mask removes)
    if (h, w) != CANVAS:
        assert float(canvas.abs().sum()) > float(canvas[..., :h, :w].abs().sum())


@pytest.mark.parametrize("h,w", DOCS)
def test_zero_padded_pool_on_a_zero_extended_canvas_is_the_document_pool(h, w):
    g = torch.Generator().manual_seed(h * 31 + w)
    for x in (torch.relu(torch.randn((1, 2, h, w), generator=g, dtype=torch.float64)),       # ReLU net: values >= 0
              torch.nn.functional.elu(torch.randn((1, 2, h, w), generator=g, dtype=torch.float64))):   # ELU net: negative values
        alone = _pool(x)
        canvas = _pool(_place(x, *CANVAS))
        eh, ew = -(-h // 2), -(-w // 2)
        assert tuple(alone.shape[-2:]) == (eh, ew)
        torch.testing.assert_close(canvas[..., :eh, :ew], alone, rtol=0, atol=0)
        # the argmax positions agree too (the padded position comes last in scan order)
        _, ia = F.max_pool2d(F.pad(x, (0, w % 2, 0, h % 2)), 2, 2, return_indices=True)
        _, ic = F.max_pool2d(_place(x, *CANVAS), 2, 2, return_indices=True)
        ra, ca = ia // (w + w % 2), ia % (w + w % 2)
        rc, cc = ic[..., :eh, :ew] // CANVAS[1], ic[..., :eh, :ew] % CANVAS[1]
        assert torch.equal(ra, rc) and torch.equal(ca, cc)


@pytest.mark.parametrize("h,w", DOCS)
def test_transposed_conv_on_a_zero_extended_canvas_is_the_document_deconv(h, w):
    """output_size odd and even: output_padding only extends the end; the one input row / column an output pixel inside the
    document can read beyond ceil(h/2) is outside the document, hence zero on the canvas as well"""
    g = torch.Generator().manual_seed(h * 17 + w)
    lo = (-(-h // 2), -(-w // 2))
    x = torch.randn((1, 3, *lo), generator=g, dtype=torch.float64)
    wt = torch.randn((3, 2, 3, 3), generator=g, dtype=torch.float64)                 # IOHW
    b = torch.randn((2,), generator=g, dtype=torch.float64)
    alone = _deconv(x, wt, b, (h, w))
    canvas_lo = (CANVAS[0] // 2, CANVAS[1] // 2)
    canvas = _deconv(_place(x, *canvas_lo), wt, b, CANVAS)
    torch.testing.assert_close(canvas[..., :h, :w], alone, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("h,w", [(7, 5), (9, 6)])
def test_a_conv_chain_with_the_extent_mask_is_the_document_chain(h, w):
    """conv -> ReLU -> pool -> dilated conv -> deconv -> 4x4 end conv, masking after every op: the crop equals the document's
    own chain, the forward AND the gradient of the input (backward = the same 0/1 masks)"""
    g = torch.Generator().manual_seed(5)
    W1, b1 = torch.randn((4, 3, 3, 3), generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    W2, b2 = torch.randn((4, 4, 3, 3), generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    W3, b3 = torch.randn((4, 4, 3, 3), generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    W4, b4 = torch.randn((2, 4, 4, 4), generator=g, dtype=torch.float64), torch.randn(2, generator=g, dtype=torch.float64)

    def chain(x, ext):
        def m(t, lv):
            if ext is None:
                return t
            eh, ew = -(-ext[0] // 2 ** lv), -(-ext[1] // 2 ** lv)
            mask = torch.zeros_like(t)
            mask[..., :eh, :ew] = 1
            return t * mask
        a = m(torch.relu(_same_conv(x, W1, b1, 1)), 0)
        p = _pool(a)
        c = m(torch.relu(_same_conv(p, W2, b2, 2)), 1)
        d = m(_deconv(c, W3, b3, a.shape[-2:]), 0)
        return m(_same_conv(d + a, W4, b4, 1), 0)

    x = torch.randn((1, 3, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    xc = _place(x.detach(), *CANVAS).requires_grad_(True)
    alone, canvas = chain(x, None), chain(xc, (h, w))
    torch.testing.assert_close(canvas[..., :h, :w], alone, rtol=1e-12, atol=1e-12)
    assert float(canvas.detach()[..., h:, :].abs().sum() + canvas.detach()[..., :, w:].abs().sum()) == 0.0
    gy = torch.randn(alone.shape, generator=g, dtype=torch.float64)
    alone.backward(gy)
    canvas.backward(_place(gy, *CANVAS))
    torch.testing.assert_close(xc.grad[..., :h, :w], x.grad, rtol=1e-12, atol=1e-12)


def test_level_extents_are_the_sizes_the_document_alone_produces():
    sizes = torch.tensor([[37, 29], [40, 40], [21, 33], [1, 1], [8, 6]])
    ext = Plan.level_extents(sizes, 4)
    assert ext.dtype == torch.int32 and tuple(ext.shape) == (4, 5, 2)
    for b, (h, w) in enumerate(sizes.tolist()):
        x = torch.zeros((1, 1, h, w))
        for lv in range(4):
            assert tuple(ext[lv, b].tolist()) == tuple(x.shape[-2:]), (b, lv)
            x = _pool(x)                                        # what the net's PoolOp produces: (H + 1) // 2
    assert tuple(ext[3, 4].tolist()) == (1, 1)                  # an 8 x 6 document is one pixel at the bottleneck


def _docs(shapes, C=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"mask": torch.rand((1, C, h, w), generator=g), "label": torch.randint(0, 4, (1, h, w), generator=g).float()}
            for h, w in shapes]


def test_pack_unpack_round_trip_and_canvas_rounding():
    docs = _docs([(37, 29), (40, 40), (21, 33)])
    x, labels, sizes = pack(docs, round_to=16)
    assert tuple(x.shape) == (3, 5, 48, 48) and tuple(labels.shape) == (3, 48, 48)
    assert x.dtype == torch.float32 and labels.dtype == torch.int64 and sizes.device.type == "cpu"
    assert sizes.tolist() == [[37, 29], [40, 40], [21, 33]]
    for d, xm, lm in zip(docs, unpack(x, sizes), unpack(labels, sizes)):
        assert torch.equal(xm, d["mask"][0]) and torch.equal(lm, d["label"][0].long())
    for b, (h, w) in enumerate(sizes.tolist()):
        assert float(x[b, :, h:].abs().sum() + x[b, :, :, w:].abs().sum()) == 0.0
        assert int(labels[b, h:].abs().sum() + labels[b, :, w:].abs().sum()) == 0
    x1, _, _ = pack(docs, round_to=1)
    assert tuple(x1.shape[-2:]) == (40, 40)
    x8, _, _ = pack(docs[:1], round_to=8)
    assert tuple(x8.shape[-2:]) == (40, 32)
    assert abs(padded_fraction(sizes, 48, 48) - (1 - (37 * 29 + 40 * 40 + 21 * 33) / (3 * 48 * 48))) < 1e-12


def test_batches_group_similar_sizes_and_cover_every_document_once():
    shapes = [(60 + (i * 37) % 110, 40 + (i * 53) % 90) for i in range(37)]
    docs = _docs(shapes, C=2)
    groups = list(batches(docs, 8))
    assert sorted(i for gr in groups for i in gr) == list(range(37))
    assert all(1 <= len(gr) <= 8 for gr in groups) and len(groups) == 5
    areas = [[shapes[i][0] * shapes[i][1] for i in gr] for gr in groups]
    assert all(max(a) <= min(b) for a, b in zip(areas, areas[1:]))          # sorted by area: groups do not interleave
    with pytest.raises(ValueError):
        next(batches(docs, 0))


def test_bad_sizes_are_refused_on_the_host():
    from msau_amd import MSAUWrapper
    m = MSAUWrapper(5, 3, dict(scale_space_num=2, res_depth=1, featRoot=8, num_blocks=1, seed=0))
    x = torch.zeros((2, 5, 16, 16))
    ok = m._check_sizes(x, torch.tensor([[16, 16], [1, 3]]))
    assert ok.tolist() == [[16, 16], [1, 3]]
    for bad in (torch.tensor([[0, 4], [3, 3]]), torch.tensor([[4, 0], [3, 3]]), torch.tensor([[17, 4], [3, 3]]),
                torch.tensor([[4, 4], [3, 17]]), torch.tensor([[4, 4]]), torch.tensor([[4, 4], [3, 3], [2, 2]]),
                torch.tensor([[4.0, 4.0], [3.0, 3.0]])):
        with pytest.raises(ValueError):
            m._check_sizes(x, bad)
    with pytest.raises(ValueError):
        unpack(torch.zeros((2, 3, 8, 8)), torch.tensor([[9, 1], [1, 1]]))


def test_box_variant_refuses_sizes():
    from msau_amd.model_box import BMSAUWrapper
    m = BMSAUWrapper(5, 3, dict(scale_space_num=2, res_depth=1, featRoot=8, num_blocks=1, seed=0))
    with pytest.raises(NotImplementedError, match="ragged"):
        m._check_sizes(torch.zeros((1, 5, 8, 8)), torch.tensor([[4, 4]]))


def _desc(B=2, H=20, W=18, C1=16, C2=0, Cout=16, k=3, dil=1, flags=0):
    d = L.ConvDesc()
    d.B, d.Hin, d.Win, d.Hout, d.Wout = B, H, W, H, W
    d.C1, d.C2, d.Cout, d.KH, d.KW, d.dil = C1, C2, Cout, k, k, dil
    d.pad_t = d.pad_l = same_pads(H, k, 1, dil)[0]
    d.stride = d.ups = 1
    d.flags = flags
    return d


def test_extent_flag_abi():
    lib = L.load()
    assert lib.msau_version() == 11
    assert L.CONV_EXTENT == 65536
    assert L.ConvDesc.extent.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(L.ConvDesc) == lib.msau_sizeof(0)
    info = (L.i32 * 8)()
    for dtype in (L.F32, L.BF16):
        for d in (_desc(), _desc(k=1, C1=8, C2=8, Cout=8), _desc(dil=8), _desc(k=4, C1=8, Cout=8)):
            L.call("msau_conv2d_launch_info", dtype, ctypes.byref(d), info)
            assert info[7] & 128, (dtype, d.KH)                  # the generic tile kernel takes the launch with the flag
            d.flags |= L.CONV_EXTENT
            L.call("msau_conv2d_launch_info", dtype, ctypes.byref(d), info)
            assert info[6] == 0 and info[7] & 128                # ... and it is the instance chosen
        # flags that only the specialised instances implement: no extent
        dout = _desc(k=1, C1=8, Cout=16, flags=L.CONV_DOUT)
        L.call("msau_conv2d_launch_info", dtype, ctypes.byref(dout), info)
        assert not info[7] & 128
    # msau_conv2d refuses such a descriptor before any launch
    dummy = torch.zeros(16)
    dout = _desc(k=1, C1=8, Cout=16, flags=L.CONV_DOUT | L.CONV_EXTENT)
    dout.x1 = dout.wpack = dout.y = dout.y2 = dout.extent = dummy.data_ptr()
    with pytest.raises(L.MsauHipError, match="EXTENT"):
        L.call("msau_conv2d", None, L.BF16, ctypes.byref(dout))
    noext = _desc(flags=L.CONV_EXTENT)
    noext.x1 = noext.wpack = noext.y = dummy.data_ptr()
    with pytest.raises(L.MsauHipError, match="extent pointer"):
        L.call("msau_conv2d", None, L.F32, ctypes.byref(noext))
