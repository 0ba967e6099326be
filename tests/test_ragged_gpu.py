"""GPU: ragged batches -- documents of their own (h, w) on one canvas.  The extent flag of the generic conv kernel, the masked
attention and pool backward, and the whole net: every document of a ragged batch computes what it computes alone."""
import ctypes as C

import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.data.ragged import pack, unpack
from msau_amd.plan import Act, ConvOp, Plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _ext(sizes):
    return torch.tensor(sizes, dtype=torch.int32, device=DEV).contiguous()


def _outside(t, sizes):
    """t [B, H, W, C]: the elements outside each sample's (h, w)"""
    parts = []
    for b, (h, w) in enumerate(sizes):
        parts += [t[b, h:].reshape(-1), t[b, :h, w:].reshape(-1)]
    return torch.cat(parts)


# ---- 1. msau_conv2d + MSAU_CONV_EXTENT ----------------------------------------------------------------------------------
def _conv_plan(dtype, B, H, W, cin, cout, k, dil=1, kind="conv", cin2=0):
    out_hw = (2 * H - 1, 2 * W) if kind == "deconv" else (H, W)
    wshape = (cin, cout, k, k) if kind == "deconv" else (cout, cin + cin2, k, k)
    g = torch.Generator().manual_seed(k * 100 + cin + cout + dil + cin2)
    params = {"w": torch.randn(wshape, generator=g) * 0.2, "b": torch.randn((cout,), generator=g) * 0.2}
    poff, pshape, off = {}, {}, 0
    for n, v in params.items():
        poff[n], pshape[n] = off, tuple(v.shape)
        off += -(-v.numel() // 4) * 4
    flat = torch.zeros(off)
    for n, v in params.items():
        flat[poff[n]:poff[n] + v.numel()] = v.reshape(-1)

    def build(plan):
        x2 = Act(plan, "x2", H, W, cin2) if cin2 else None
        y = Act(plan, "y", *out_hw, cout)
        ConvOp(plan, "c", plan.x_in, x2, "w", "b", y, k, dil=dil, kind=kind)
        plan.logits = y
    plan = Plan(dict(channels=cin, input_grad=True), B, H, W, dtype, DEV, poff, pshape, training=True, builder=build)
    plan.pack(flat.to(DEV))
    for a in plan.acts:
        a.data.copy_(torch.randn(a.data.shape, generator=g).to(a.data.dtype))
        if a.grad is not None:
            a.grad.copy_(torch.randn(a.grad.shape, generator=g).to(a.grad.dtype))
    return plan, next(op for op in plan.ops if isinstance(op, ConvOp))


def _launch(dtype, desc, out, flags_add=0, extent=None):
    d = L.ConvDesc.from_buffer_copy(desc)
    d.flags |= flags_add
    d.extent = extent.data_ptr() if extent is not None else None
    out.fill_(7.0)                                   # (stale values must not survive outside the extent)
    L.call("msau_conv2d", _stream(), dtype, C.byref(d))
    torch.cuda.synchronize()
    info = (L.i32 * 8)()
    L.call("msau_conv2d_launch_info", dtype, C.byref(d), info)
    return out.float().clone(), list(info)


CONV_CASES = [  # (cin, cout, k, dil, kind, cin2)
    pytest.param(8, 8, 3, 1, "conv", 0, id="3x3"),
    pytest.param(16, 32, 3, 8, "conv", 0, id="3x3dil8"),
    pytest.param(16, 16, 1, 1, "conv", 16, id="1x1concat"),
    pytest.param(8, 8, 4, 1, "conv", 0, id="4x4"),
    pytest.param(16, 8, 3, 1, "deconv", 0, id="deconv"),
]


@pytest.mark.parametrize("dtype", [pytest.param(L.F32, id="f32"), pytest.param(L.BF16, id="bf16")])
@pytest.mark.parametrize("cin,cout,k,dil,kind,cin2", CONV_CASES)
def test_conv_extent_zeroes_outside_and_keeps_inside(dtype, cin, cout, k, dil, kind, cin2):
    B, H, W = 3, 19, 21
    plan, op = _conv_plan(dtype, B, H, W, cin, cout, k, dil, kind, cin2)
    launches = [(op.fdesc, op.out.data)] + [(dd, x.grad) for dd, x in zip(op.ddesc, (op.x1, op.x2)) if dd is not None]
    assert len(launches) >= 2                                   # forward + data gradient(s) (stride 2 for the deconv)
    for desc, out in launches:
        Ho, Wo = desc.Hout, desc.Wout
        sizes = [(Ho, Wo), (max(1, Ho - 6) | 1, max(1, Wo - 8) | 1), (1, 1)]       # the full canvas, odd sizes, one pixel
        ref, info0 = _launch(dtype, desc, out)
        got, info1 = _launch(dtype, desc, out, L.CONV_EXTENT, _ext(sizes))
        assert info1[7] & 128 and info1[6] == 0, info1
        assert float(_outside(got, sizes).abs().max()) == 0.0
        for b, (h, w) in enumerate(sizes):
            r, q = ref[b, :h, :w], got[b, :h, :w]
            if info0[:2] == info1[:2] and info0[6] == info1[6]:
                assert torch.equal(r, q), "same instance: bit-identical"
            else:
                tol = 1e-6 if dtype == L.F32 else 2.0 ** -7
                assert float((r - q).abs().max()) <= tol * max(float(r.abs().max()), 1e-30), (b, float((r - q).abs().max()))


def test_conv_extent_is_refused_with_dout():
    plan, op = _conv_plan(L.BF16, 2, 16, 16, 8, 8, 1, cin2=8)
    d = L.ConvDesc.from_buffer_copy(op.ddesc[0])
    d.Cout, d.flags, d.y2 = 16, L.CONV_DOUT | L.CONV_EXTENT, op.x2.grad.data_ptr()
    ext = _ext([(16, 16), (3, 5)])
    d.extent = ext.data_ptr()
    info = (L.i32 * 8)()
    L.call("msau_conv2d_launch_info", L.BF16, C.byref(d), info)
    assert not info[7] & 128
    with pytest.raises(L.MsauHipError, match="EXTENT"):
        L.call("msau_conv2d", _stream(), L.BF16, C.byref(d))


# ---- 2. attention with extents ----------------------------------------------------------------------------------------
def _attn_case(dtype, Hb, Wb, Ds, Cs, sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, N = len(sizes), Hb * Wb
    td = torch.float32 if dtype == L.F32 else torch.bfloat16

    def t(c):
        v = torch.randn((B, Hb, Wb, c), generator=g)
        for b, (h, w) in enumerate(sizes):
            v[b, h:] = 0
            v[b, :, w:] = 0
        return v.to(td).to(DEV).contiguous()
    return [t(Ds), t(Ds), t(Cs), t(Cs), t(Cs)]         # f, g, h, x, dy


def _attn_run(dtype, f, g, h, x, dy, ext, W):
    B, Hb, Wb, Ds = f.shape
    Cs = h.shape[-1]
    N = Hb * Wb
    y, df, dg, dh = torch.empty_like(x), torch.empty_like(f), torch.empty_like(g), torch.empty_like(h)
    for t in (y, df, dg, dh):
        t.fill_(5.0)
    stats = torch.zeros((B, N, 2), dtype=torch.float32, device=DEV)
    ws = torch.zeros((B * N * (Cs + 4),), dtype=torch.float32, device=DEV)
    ep = ext.data_ptr() if ext is not None else None
    L.call("msau_selfattn_fwd_ext", _stream(), dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), x.data_ptr(), y.data_ptr(),
           stats.data_ptr(), B, N, Ds, Cs, ep, W)
    L.call("msau_selfattn_bwd_ext", _stream(), dtype, f.data_ptr(), g.data_ptr(), h.data_ptr(), dy.data_ptr(), stats.data_ptr(),
           df.data_ptr(), dg.data_ptr(), dh.data_ptr(), ws.data_ptr(), B, N, Ds, Cs, ep, W)
    torch.cuda.synchronize()
    return y, df, dg, dh


@pytest.mark.parametrize("dtype,Hb,Wb,Ds,Cs", [
    pytest.param(L.F32, 7, 9, 8, 64, id="f32-valu"),
    pytest.param(L.F32, 6, 5, 32, 256, id="f32-anywidth"),
    pytest.param(L.BF16, 7, 9, 8, 64, id="bf16-mfma"),
    pytest.param(L.BF16, 6, 6, 8, 32, id="bf16-mfma-c32"),
    pytest.param(L.BF16, 100, 100, 8, 64, id="bf16-valu-large"),
])
def test_attention_extent_equals_each_sample_alone(dtype, Hb, Wb, Ds, Cs):
    if Hb == 100:                                       # N = 10000: beyond the MFMA statistics kernel's LDS, the VALU kernels
        sizes = [(100, 100), (97, 61), (1, 1)]
    else:
        sizes = [(Hb, Wb), (Hb - 2 | 1, Wb - 3 | 1), (1, 1)]
    f, g, h, x, dy = _attn_case(dtype, Hb, Wb, Ds, Cs, sizes)
    outs = _attn_run(dtype, f, g, h, x, dy, _ext(sizes), Wb)
    tol = 1e-5 if dtype == L.F32 else 2e-2
    for b, (hh, ww) in enumerate(sizes):
        crop = [t[b:b + 1, :hh, :ww].contiguous() for t in (f, g, h, x, dy)]
        alone = _attn_run(dtype, *crop, None, ww)       # (a small crop may run on the other kernel family)
        for nm, full, a in zip(("y", "df", "dg", "dh"), outs, alone):
            mine = full[b:b + 1, :hh, :ww].double().cpu()
            a = a.double().cpu()
            # relative to the output's scale (inputs ~N(0, 1)): a 1 x 1 document has df = dg = 0 in exact arithmetic, and the two
            # evaluations leave different rounding residue there
            err = float((mine - a).norm()) / max(float(a.norm()), 1.0)
            assert err <= tol, (nm, b, err)
    dh = outs[3]
    assert float(_outside(dh.float(), sizes).abs().max()) == 0.0
    for t in outs[:3]:
        assert float(_outside(t.float(), sizes).abs().max()) == 0.0


# ---- 3. pool backward with extents --------------------------------------------------------------------------------------
@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_pool_backward_extent(elu, dtype):
    B, H, W, Cs = 3, 17, 15, 16
    sizes = [(17, 15), (9, 7), (1, 1)]
    g = torch.Generator().manual_seed(3)
    td = torch.float32 if dtype == L.F32 else torch.bfloat16
    x = torch.randn((B, H, W, Cs), generator=g)
    x = torch.nn.functional.elu(x) if elu else torch.relu(x)
    for b, (h, w) in enumerate(sizes):
        x[b, h:] = 0
        x[b, :, w:] = 0
    x = x.to(td).to(DEV)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y = torch.zeros((B, Ho, Wo, Cs), dtype=td, device=DEV)
    idx = torch.zeros((B, Ho, Wo, Cs), dtype=torch.uint8, device=DEV)
    L.call("msau_maxpool2x2_fwd", _stream(), dtype, x.data_ptr(), y.data_ptr(), idx.data_ptr(), B, H, W, Cs)
    dy = torch.randn((B, Ho, Wo, Cs), generator=g)
    for b, (h, w) in enumerate(sizes):
        dy[b, -(-h // 2):] = 0
        dy[b, :, -(-w // 2):] = 0
    dy = dy.to(td).to(DEV)
    acc = 2 if elu else 0
    ref, got = torch.empty_like(x), torch.empty_like(x)
    L.call("msau_maxpool2x2_bwd", _stream(), dtype, dy.data_ptr(), idx.data_ptr(), ref.data_ptr(), x.data_ptr(), B, H, W, Cs, acc)
    ext = _ext(sizes)
    L.call("msau_maxpool2x2_bwd_ext", _stream(), dtype, dy.data_ptr(), idx.data_ptr(), got.data_ptr(), x.data_ptr(), B, H, W, Cs,
           acc, ext.data_ptr())
    torch.cuda.synchronize()
    assert float(_outside(got.float(), sizes).abs().max()) == 0.0
    if elu:                                            # the ELU mask keeps what a window sends to its zero padding: the extent does not
        assert float(_outside(ref.float(), sizes).abs().max()) > 0.0
    for b, (h, w) in enumerate(sizes):
        assert torch.equal(got[b, :h, :w], ref[b, :h, :w])


# ---- 4.-9. the network --------------------------------------------------------------------------------------------------
CH, NCLS = 13, 5
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
DOCS = [(37, 29), (40, 40), (21, 33)]


def _model(dtype="fp32", **extra):
    return MSAUWrapper(CH, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


def _docs(shapes, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        occ = torch.rand((1, h, w), generator=g) < 0.3
        ids = torch.randint(0, CH, (1, h, w), generator=g)
        x = torch.zeros((1, CH, h, w))
        x.scatter_(1, ids.unsqueeze(1), occ.unsqueeze(1).float())
        lab = (occ * torch.randint(1, NCLS, (1, h, w), generator=g)).float()
        out.append({"mask": x, "label": lab})
    return out


def _forward(m, x, sizes=None):
    with torch.no_grad():
        _, logits, aux = m(x.to(DEV), sizes)
    torch.cuda.synchronize()
    return logits.cpu(), aux.cpu()


def _forward_case(activation="relu"):
    extra = {} if activation == "relu" else dict(activation_name="elu")
    m = _model(**extra)
    docs = _docs(DOCS)
    x, labels, sizes = pack(docs, round_to=16)
    assert tuple(x.shape[-2:]) == (48, 48)
    lg, ax = _forward(m, x, sizes)
    for b, d in enumerate(docs):
        l1, a1 = _forward(m, d["mask"])
        for nm, crop, alone in (("logits", unpack(lg, sizes)[b], l1[0]), ("aux", unpack(ax, sizes)[b], a1[0])):
            assert _rel(crop, alone) <= 1e-5, (nm, b, _rel(crop, alone))
    assert float(lg[0, :, 37:].abs().max()) == 0.0 and float(lg[2, :, :, 33:].abs().max()) == 0.0
    # the same canvas without sizes: the zero padding is not the documents' padding
    ld, _ = _forward(m, x)
    far = max(_rel(unpack(ld, sizes)[b], _forward(m, d["mask"])[0][0]) for b, d in enumerate(docs))
    assert far > 1e-2, far


def test_fp32_network_forward_ragged_equals_each_document_alone():
    _forward_case()


def test_elu_network_forward_ragged_equals_each_document_alone():
    _forward_case("elu")


def test_bf16_forward_costs_no_more_than_bf16_itself():
    m32, m16 = _model(), _model("bf16")
    docs = _docs(DOCS)
    x, _, sizes = pack(docs, round_to=16)
    lg, ax = _forward(m16, x, sizes)
    num_r = num_1 = 0.0
    for b, d in enumerate(docs):
        r32 = _forward(m32, d["mask"])
        r16 = _forward(m16, d["mask"])
        for crop, one, ref in ((unpack(lg, sizes)[b], r16[0][0], r32[0][0]), (unpack(ax, sizes)[b], r16[1][0], r32[1][0])):
            num_r += float((crop.double() - ref.double()).norm()) ** 2
            num_1 += float((one.double() - ref.double()).norm()) ** 2
    assert num_1 > 0 and num_r ** 0.5 <= 1.5 * num_1 ** 0.5, (num_r ** 0.5, num_1 ** 0.5)


def _engine_step(m, x, lab, sizes=None, use_graph=False, eng=None):
    eng = eng or TrainEngine(m, lr=0.0, use_graph=use_graph)          # lr 0: the parameters stay put between steps
    loss = eng.step(x.to(DEV), lab.to(DEV), sizes)
    torch.cuda.synchronize()
    return float(loss), eng.flat_grad.clone().cpu(), eng


def test_fp32_train_step_is_the_mean_of_the_documents():
    shapes = DOCS + [(8, 6)]                                           # 8 x 6: one pixel at the bottleneck
    docs = _docs(shapes, seed=2)
    x, labels, sizes = pack(docs, round_to=16)
    m = _model()
    loss, grad, _ = _engine_step(m, x, labels, sizes)
    losses, grads = [], []
    for d in docs:
        l1, g1, _ = _engine_step(m, d["mask"], d["label"])
        losses.append(l1)
        grads.append(g1)
    ref_loss = sum(losses) / len(losses)
    ref_grad = sum(grads) / len(grads)
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert _rel(grad, ref_grad) <= 1e-4, _rel(grad, ref_grad)
    # the reference-style autograd loop on the same ragged batch
    m.zero_grad(set_to_none=True)
    _, logits, aux = m(x.to(DEV), sizes)
    l_ag = m.loss(logits, aux, labels.to(DEV))
    l_ag.backward()
    torch.cuda.synchronize()
    assert abs(float(l_ag.detach()) - ref_loss) <= 1e-5 * abs(ref_loss)
    ag = torch.zeros_like(ref_grad)
    for key, p in m._named:
        if p.grad is not None:
            ag[m._poff[key]:m._poff[key] + p.numel()] = p.grad.reshape(-1).cpu()
    assert _rel(ag, ref_grad) <= 1e-4, _rel(ag, ref_grad)


def test_garbage_outside_the_extents_is_ignored():
    docs = _docs(DOCS, seed=3)
    x, labels, sizes = pack(docs, round_to=16)
    g = torch.Generator().manual_seed(9)
    xg, lg = x.clone(), labels.clone()
    for b, (h, w) in enumerate(sizes.tolist()):
        for t, v in ((xg, torch.rand(x.shape[1:], generator=g) * 5), (lg, torch.randint(1, NCLS, labels.shape[1:], generator=g))):
            keep = t[b].clone()
            t[b] = v.to(t.dtype)
            t[b][..., :h, :w] = keep[..., :h, :w]
    m = _model(deterministic=True)
    l0, g0, _ = _engine_step(m, x, labels, sizes)
    l1, g1, _ = _engine_step(m, xg, lg, sizes)
    assert l0 == l1 and torch.equal(g0, g1)
    f0, f1 = _forward(m, x, sizes), _forward(m, xg, sizes)
    assert torch.equal(f0[0], f1[0]) and torch.equal(f0[1], f1[1])
    # external logit gradients of the autograd path
    G = torch.randn(f0[0].shape, generator=g)
    Gz = G.clone()
    for b, (h, w) in enumerate(sizes.tolist()):
        Gz[b, :, h:] = 0
        Gz[b, :, :, w:] = 0
    res = []
    for GG in (G, Gz):
        m.zero_grad(set_to_none=True)
        _, logits, aux = m(xg.to(DEV), sizes)
        (logits * GG.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        res.append([p.grad.clone().cpu() for _, p in m._named if p.grad is not None])
    assert len(res[0]) > 0 and all(torch.equal(a, b) for a, b in zip(*res))


def test_graph_replay_with_different_size_sets():
    m = _model(deterministic=True)
    sets = [DOCS, [(48, 48), (9, 7), (8, 6)]]
    eager, graph = [], []
    eng_e = eng_g = None
    for shapes in sets:
        docs = _docs(shapes, seed=4)
        x, labels, sizes = pack(docs, round_to=16)
        assert tuple(x.shape[-2:]) == (48, 48)
        l, gr, eng_e = _engine_step(m, x, labels, sizes, eng=eng_e)
        eager.append((l, gr))
        l, gr, eng_g = _engine_step(m, x, labels, sizes, use_graph=True, eng=eng_g)
        graph.append((l, gr))
    assert len(m._plan_for(torch.zeros((3, CH, 48, 48), device=DEV), True, ragged=True).__dict__.get("_tgraphs", {})) == 1
    for (le, ge), (lgr, gg) in zip(eager, graph):
        assert le == lgr and torch.equal(ge, gg)
    assert not torch.equal(eager[0][1], eager[1][1])
