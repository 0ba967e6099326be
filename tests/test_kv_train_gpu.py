"""GPU: key-value training on the device -- the training painter (msau_kv_paint_train) against `paint_train_host`, the class
histogram and the UNetLoss kernel (msau_label_hist, msau_unet_ce) against torch in float64, and `TrainEngine.step_unet` /
`step_kv`: the ragged rule, the reference's form of the loss, tables against canvases, garbage outside the documents, bf16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import UNetLoss
from msau_amd.training import kv_data as D
from tests import kv_train_util as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = 60, T.N_CLASS
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
EXTENTS = [(37, 29), (8, 6), (1, 1)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---- 6: the painter ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return [T.gold_tables(si) for si in range(len(T.SETTINGS))]


def _assert_painted(tables, round_to=16):
    got = D.paint_train_device(tables, round_to=round_to, device=DEV)
    torch.cuda.synchronize()
    want = T.canvases_want(tables, round_to=round_to)
    assert [g_.dtype for g_ in got[:3]] == [torch.int32, torch.int64, torch.int64]
    for plane, g_, w in zip(("ids", "labels", "aux"), got[:3], want[:3]):
        assert tuple(g_.shape) == w.shape and np.array_equal(g_.cpu().numpy(), w), (plane, int((g_.cpu().numpy() != w).sum()))
    assert np.array_equal(got[3].numpy(), want[3])
    return got


def test_painter_equals_host_on_goldens_dense_and_ragged(gold):
    for tables in gold:
        for t in tables:
            _assert_painted([t], round_to=1)                               # dense: a document on its own shape
    for tables in gold:
        _assert_painted(tables)                                            # ragged: three documents on one canvas
    ids, lab, aux, sizes = _assert_painted([t for tables in gold for t in tables])
    for b, (h, w) in enumerate(sizes.tolist()):
        for g_ in (ids, lab, aux):
            assert bool((g_[b, h:] == -1).all()) and bool((g_[b, :, w:] == -1).all()) and bool((g_[b, :h, :w] >= 0).all())


def test_painter_big_layout_and_fallback():
    from tests import glyphs_util as U
    named = dict(T.all_tables())
    big, jit = named["big"], named["big_jitter"]
    assert len(big.line_rec) <= 256 < len(named["lines_600"].line_rec)
    _assert_painted([big], round_to=1)
    _assert_painted([named["lines_600"], jit, named["narrow_box"]])         # more than one staging pass, beside smaller documents
    before = dict(D.STATS)
    bad = T.table_of(T.with_labels(U.unrepresentable_layouts()[0][1], 2))
    _assert_painted([named["types"], bad, named["zero_height"]])            # the document without a table: painted on the host
    assert D.STATS["host_painted"] == before["host_painted"] + 1 and D.STATS["documents"] == before["documents"] + 3


def test_second_launch_leaves_no_trace_of_the_first(gold):
    """two groups painted into the SAME canvases, one after the other: nothing is cleared in between"""
    first, second = gold[2], gold[4]
    r1, o1, s1, c1 = D.pack_train_tables(first)
    r2, o2, s2, c2 = D.pack_train_tables(second)
    H, W = max(c1[0], c2[0]), max(c1[1], c2[1])
    ids = torch.empty((3, H, W), dtype=torch.int32, device=DEV)
    lab, aux = (torch.empty((3, H, W), dtype=torch.int64, device=DEV) for _ in range(2))
    for rec, off, tables in ((r1, o1, first), (r2, o2, second)):
        d = torch.from_numpy(rec).to(DEV)
        at = lambda name: d.data_ptr() + 4 * off[name]
        L.call("msau_kv_paint_train", _stream(), at("lines"), at("glyphs"), at("labels"), at("line_off"), at("glyph_off"), at("sizes"),
               3, H, W, ids.data_ptr(), lab.data_ptr(), aux.data_ptr())
        torch.cuda.synchronize()
    want = np.full((3, H, W), -1, dtype=np.int64), np.full((3, H, W), -1, dtype=np.int64), np.full((3, H, W), -1, dtype=np.int64)
    for b, t in enumerate(second):
        h, w = t.shape
        for dst, src in zip(want, D.paint_train_host(t)):
            dst[b, :h, :w] = src
    for g_, w in zip((ids, lab, aux), want):
        assert np.array_equal(g_.cpu().numpy().astype(np.int64), w)


# ---- 7: the histogram ---------------------------------------------------------------------------------------------------------------
def _labels(B, H, W, C, seed, ragged):
    """labels in [0, C) inside the extents; -1 and C sprinkled inside (when asked) and outside"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    if ragged:
        for b, (h, w) in enumerate(EXTENTS):
            junk = torch.randint(-1, C + 1, (H, W), generator=g)
            keep = lab[b, :h, :w].clone()
            lab[b] = junk
            lab[b, :h, :w] = keep
    return lab


@pytest.mark.parametrize("K", [1, 4])
def test_label_hist_equals_bincount(K):
    B, H, W, C = 3, 37, 29, 17
    for ragged in (True, False):
        lab = _labels(B, H, W, C, 3, ragged)
        lab[0, 5, 7], lab[0, 36, 28], lab[1, 2, 3], lab[1, 0, 0] = -1, C, C, -1        # outside [0, C) INSIDE the extents
        ext = torch.tensor(EXTENTS, dtype=torch.int32, device=DEV) if ragged else None
        part = torch.full((B, K, C), 77, dtype=torch.int32, device=DEV)
        d = lab.to(DEV)
        L.call("msau_label_hist", _stream(), d.data_ptr(), ext.data_ptr() if ragged else None, part.data_ptr(), B, H, W, C, K)
        torch.cuda.synchronize()
        got = part.sum(dim=1).cpu()
        for b in range(B):
            h, w = EXTENTS[b] if ragged else (H, W)
            v = lab[b, :h, :w].reshape(-1)
            v = v[(v >= 0) & (v < C)]
            assert torch.equal(got[b].long(), torch.bincount(v, minlength=C)), (ragged, b)


# ---- 8: the loss kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 12, 17])
def test_unet_ce_equals_float64_torch(C, dtype):
    B, H, W = 3, 37, 29
    Cs = -(-C // 8) * 8
    td, dt = (torch.float32, L.F32) if dtype == "fp32" else (torch.bfloat16, L.BF16)
    tol = 1e-5 if dtype == "fp32" else 1e-2
    g = torch.Generator().manual_seed(C)
    K = 4
    ws = torch.zeros(int(L.load().msau_unet_ce_ws_floats(B * H * W)), device=DEV)
    for ragged in (False, True):
        ext_l = EXTENTS if ragged else [(H, W)] * B
        logits = [(torch.randn(B, H, W, Cs, generator=g) * 2).to(td) for _ in range(2)]
        labs = [_labels(B, H, W, C, 20 + t, False) for t in range(2)]
        cw_h = torch.rand(C, generator=g) + 0.5
        cw_h[2] = 0.0                                                       # one weight is 0 ...
        if ragged:
            labs[0][2, 0, 0], labs[1][2, 0, 0] = 2, 3                       # ... and the 1 x 1 document's final head has only that class
            for b, (h, w) in enumerate(ext_l):                              # label -1 and garbage logits outside the extents
                for t in range(2):
                    keep_l, keep_x = labs[t][b, :h, :w].clone(), logits[t][b, :h, :w].clone()
                    labs[t][b] = -1
                    logits[t][b] = (torch.randn(H, W, Cs, generator=g) * 1e4).to(td)
                    if h < H:
                        logits[t][b, h, 0] = float("inf")
                    labs[t][b, :h, :w], logits[t][b, :h, :w] = keep_l, keep_x
        ext = torch.tensor(ext_l, dtype=torch.int32, device=DEV) if ragged else None
        lg_d, lab_d = [x.to(DEV) for x in logits], [x.to(DEV) for x in labs]
        for with_aux in (True, False):
            for weighted in (False, True):
                cw = cw_h.to(DEV) if weighted else None
                hist = None
                if weighted:
                    hist = torch.zeros((2, B, K, C), dtype=torch.int32, device=DEV)
                    for t in range(2 if with_aux else 1):
                        L.call("msau_label_hist", _stream(), lab_d[t].data_ptr(), ext.data_ptr() if ragged else None,
                               hist[t].data_ptr(), B, H, W, C, K)
                # float64 torch: every document's crop alone, the mean of the documents
                xs = [x[..., :C].double().clone().requires_grad_(True) for x in logits[:2 if with_aux else 1]]
                per_head = []
                for t, x in enumerate(xs):
                    tot = 0.0
                    for b, (h, w) in enumerate(ext_l):
                        tg = labs[t][b, :h, :w].reshape(-1)
                        wv = cw_h.double() if weighted else torch.ones(C, dtype=torch.float64)
                        Db = float(wv[tg].sum())
                        if Db > 0:
                            tot = tot + F.cross_entropy(x[b, :h, :w].reshape(-1, C), tg, weight=wv, reduction="sum") / Db / B
                    per_head.append(tot)
                ref_total = 0.5 * per_head[0] + 0.5 * per_head[1] if with_aux else per_head[0]
                ref_total.backward()
                ref3 = [float(ref_total.detach()), float(per_head[0].detach()), float(per_head[1].detach()) if with_aux else 0.0]
                outs = []
                for _rep in range(2):
                    loss3 = torch.full((3,), 123.0, device=DEV)
                    d = [torch.full_like(x, 9.0) for x in lg_d]
                    L.call("msau_unet_ce", _stream(), dt, lg_d[0].data_ptr(), lg_d[1].data_ptr() if with_aux else None, lab_d[0].data_ptr(),
                           lab_d[1].data_ptr() if with_aux else None, ext.data_ptr() if ragged else None,
                           cw.data_ptr() if weighted else None, hist.data_ptr() if weighted else None, K, d[0].data_ptr(),
                           d[1].data_ptr() if with_aux else None, loss3.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
                    torch.cuda.synchronize()
                    outs.append((loss3.cpu(), [x.cpu() for x in d]))
                what = (C, dtype, ragged, with_aux, weighted)
                loss3, d = outs[0]
                print(what, "loss", loss3.tolist(), "ref", ref3)
                assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b_) for a, b_ in zip(outs[0][1], outs[1][1])), what
                for got, ref in zip(loss3.tolist(), ref3):
                    assert abs(got - ref) <= tol * abs(ref), (what, got, ref)
                if ragged and weighted:
                    assert ref3[1] > 0 and float(xs[0].grad[2].abs().max()) == 0.0       # the D_b = 0 document
                for t, x in enumerate(xs):
                    got = d[t].float()
                    err = float((got[..., :C].double() - x.grad).abs().max())
                    print(what, "head", t, "grad err", err, "max", float(x.grad.abs().max()))
                    assert err <= tol * float(x.grad.abs().max()) + 1e-7, (what, t, err)
                    assert Cs == C or float(got[..., C:].abs().max()) == 0.0, what           # padded channels: exactly 0
                    for b, (h, w) in enumerate(ext_l):                                      # outside the extents: exactly 0
                        assert float(got[b, h:].abs().sum()) == 0.0 and float(got[b, :, w:].abs().sum()) == 0.0, (what, b)
                if not with_aux:
                    assert bool((d[1] == 9.0).all())                                         # the absent head is not written


def test_unet_ce_wide_form_matches_register_form():
    """Cs > 32 takes the cache-read kernel: 40 classes, against float64 torch"""
    B, H, W, C, Cs = 2, 19, 23, 40, 40
    g = torch.Generator().manual_seed(1)
    lg = [(torch.randn(B, H, W, Cs, generator=g) * 2).to(DEV) for _ in range(2)]
    lab = [torch.randint(0, C, (B, H, W), generator=g).to(DEV) for _ in range(2)]
    d = [torch.empty_like(x) for x in lg]
    loss3 = torch.full((3,), 123.0, device=DEV)
    ws = torch.zeros(int(L.load().msau_unet_ce_ws_floats(B * H * W)), device=DEV)
    L.call("msau_unet_ce", _stream(), L.F32, lg[0].data_ptr(), lg[1].data_ptr(), lab[0].data_ptr(), lab[1].data_ptr(), None, None, None, 1,
           d[0].data_ptr(), d[1].data_ptr(), loss3.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
    torch.cuda.synchronize()
    for t in range(2):
        x = lg[t].double().cpu().requires_grad_(True)
        ref = F.cross_entropy(x.reshape(-1, C), lab[t].cpu().reshape(-1))
        (0.5 * ref).backward()
        assert abs(float(loss3[1 + t]) - float(ref)) <= 1e-5 * float(ref)
        assert float((d[t].cpu().double() - x.grad).abs().max()) <= 1e-5 * float(x.grad.abs().max()) + 1e-7
    assert abs(float(loss3[0]) - 0.5 * (float(loss3[1]) + float(loss3[2]))) <= 1e-6 * float(loss3[0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_unet_ce_register_form_equals_cache_form(dtype):
    """the same 17 real logits stored at Cs = 24 (a pixel in registers) and zero-padded to Cs = 40 (a pixel read from the cache): the
    two forms share one statement of the log-sum-exp and of the gradient (loss.hip) -- the same three loss bits, the same gradient
    bits in the real channels, zeros in the padded ones; ragged and dense, with and without class weights and the second head"""
    B, H, W, C, K = 3, 37, 29, 17, 4
    td, dt = (torch.float32, L.F32) if dtype == "fp32" else (torch.bfloat16, L.BF16)
    g = torch.Generator().manual_seed(17)
    real = [(torch.randn(B, H, W, C, generator=g) * 2).to(td) for _ in range(2)]
    lab_d = [_labels(B, H, W, C, 40 + t, True).to(DEV) for t in range(2)]
    cw = torch.rand(C, generator=g) + 0.5
    cw[2] = 0.0
    cw = cw.to(DEV)
    ws = torch.zeros(int(L.load().msau_unet_ce_ws_floats(B * H * W)), device=DEV)
    got = {}
    for Cs in (24, 40):
        lg_d = []
        for x in real:
            p = torch.zeros(B, H, W, Cs, dtype=td)
            p[..., :C] = x
            lg_d.append(p.to(DEV))
        for ragged in (False, True):
            ext = torch.tensor(EXTENTS, dtype=torch.int32, device=DEV) if ragged else None
            hist = torch.zeros((2, B, K, C), dtype=torch.int32, device=DEV)
            for t in range(2):
                L.call("msau_label_hist", _stream(), lab_d[t].data_ptr(), ext.data_ptr() if ragged else None, hist[t].data_ptr(), B, H, W, C, K)
            for with_aux in (True, False):
                for weighted in (False, True):
                    loss3 = torch.full((3,), 123.0, device=DEV)
                    d = [torch.full_like(x, 9.0) for x in lg_d]
                    L.call("msau_unet_ce", _stream(), dt, lg_d[0].data_ptr(), lg_d[1].data_ptr() if with_aux else None, lab_d[0].data_ptr(),
                           lab_d[1].data_ptr() if with_aux else None, ext.data_ptr() if ragged else None,
                           cw.data_ptr() if weighted else None, hist.data_ptr() if weighted else None, K, d[0].data_ptr(),
                           d[1].data_ptr() if with_aux else None, loss3.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
                    torch.cuda.synchronize()
                    got[(Cs, ragged, with_aux, weighted)] = (loss3.cpu(), [x.cpu() for x in d[:2 if with_aux else 1]])
    for (Cs, *what), (loss3, d) in got.items():
        if Cs != 24:
            continue
        wide_loss3, wide_d = got[(40, *what)]
        assert torch.equal(loss3, wide_loss3) and bool(torch.isfinite(loss3).all()) and float(loss3[0]) > 0, (what, loss3, wide_loss3)
        for a, b in zip(d, wide_d):
            assert torch.equal(a[..., :C], b[..., :C]) and float(a[..., :C].float().abs().max()) > 0, what
            assert float(a[..., C:].float().abs().max()) == 0.0 and float(b[..., C:].float().abs().max()) == 0.0, what


# ---- 9 - 15: the step -----------------------------------------------------------------------------------------------------------------
def _model(dtype="fp32", **extra):
    return MSAUWrapper(CH, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


@pytest.fixture(scope="module")
def canvases(gold):
    """the three golden documents (deterministic tables) on one canvas, as CPU tensors; shared and left unchanged"""
    ids, lab, aux, sizes = T.canvases_want(gold[0])
    return torch.from_numpy(ids), torch.from_numpy(lab), torch.from_numpy(aux), torch.from_numpy(sizes)


CW = [0.0, 2.0] + [0.5 + 0.1 * c for c in range(NCLS - 2)]


def _step(eng, ids, lab, aux, sizes=None, cw=None):
    loss = eng.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw)
    torch.cuda.synchronize()
    return loss.cpu().clone(), eng.flat_grad.clone().cpu()


@pytest.mark.parametrize("weighted", [False, True])
def test_fp32_step_is_the_mean_of_the_documents(canvases, weighted):
    ids, lab, aux, sizes = canvases
    cw = CW if weighted else None
    eng = TrainEngine(_model(), lr=0.0)
    loss, grad = _step(eng, ids, lab, aux, sizes, cw)
    losses, grads = [], []
    for b, (h, w) in enumerate(sizes.tolist()):
        l1, g1 = _step(eng, ids[b:b + 1, :h, :w], lab[b:b + 1, :h, :w], aux[b:b + 1, :h, :w], None, cw)
        losses.append(l1.double())
        grads.append(g1.double())
    ref_loss, ref_grad = sum(losses) / 3, sum(grads) / 3
    print("loss", loss.tolist(), "ref", ref_loss.tolist(), "grad rel", _rel(grad, ref_grad))
    for got, ref in zip(loss.tolist(), ref_loss.tolist()):
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    assert _rel(grad, ref_grad) <= 1e-4
    assert float(ref_grad.norm()) > 0


def test_fp32_step_against_the_reference_form(canvases):
    ids, lab, aux, sizes = canvases
    h, w = sizes[0].tolist()
    ids1, lab1, aux1 = ids[:1, :h, :w], lab[:1, :h, :w], aux[:1, :h, :w]
    m = _model()
    eng = TrainEngine(m, lr=0.0)
    loss, grad = _step(eng, ids1, lab1, aux1)
    one_hot = lambda t, n: F.one_hot(t.long(), n).permute(0, 3, 1, 2).float().to(DEV)
    m.zero_grad(set_to_none=True)
    _, logits, aux_logits = m(one_hot(ids1, CH))
    _acc, total, final = UNetLoss({})(logits, one_hot(lab1, NCLS), {"aux_logits": aux_logits, "aux_tgt": one_hot(aux1, NCLS)})
    with torch.no_grad():
        _acc, aux_alone, _none = UNetLoss({})(aux_logits.detach(), one_hot(aux1, NCLS), {})
    total.backward()
    torch.cuda.synchronize()
    ag = torch.zeros_like(grad)
    for key, p in m._named:
        if p.grad is not None:
            ag[m._poff[key]:m._poff[key] + p.numel()] = p.grad.reshape(-1).cpu()
    print("loss", loss.tolist(), "ref", float(total), float(final), "grad rel", _rel(grad, ag))
    assert abs(float(loss[0]) - float(total)) <= 1e-5 * abs(float(total))
    assert abs(float(loss[1]) - float(final)) <= 1e-5 * abs(float(final))
    assert abs(float(loss[2]) - float(aux_alone)) <= 1e-5 * abs(float(aux_alone))
    assert _rel(grad, ag) <= 1e-4


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tables_and_canvases_give_the_same_bits(gold, canvases, dtype):
    ids, lab, aux, sizes = canvases
    a, b = TrainEngine(_model(dtype, deterministic=True)), TrainEngine(_model(dtype, deterministic=True))
    assert torch.equal(a.model._flat, b.model._flat)
    for _step_no in range(2):
        la = a.step_kv(gold[0])
        lb = b.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.flat_grad, b.flat_grad) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and bool(torch.isfinite(a.model._flat).all())


def test_garbage_outside_the_documents_is_ignored(canvases):
    ids, lab, aux, sizes = canvases
    g = torch.Generator().manual_seed(9)
    junk = []
    for t, hi in ((ids, CH), (lab, NCLS), (aux, NCLS)):
        j = torch.randint(-2, hi + 2, t.shape, generator=g).to(t.dtype)    # valid classes included
        for b_, (h, w) in enumerate(sizes.tolist()):
            j[b_, :h, :w] = t[b_, :h, :w]
        junk.append(j)
    assert not torch.equal(junk[1], lab)
    for cw in (None, CW):
        a, b = TrainEngine(_model(deterministic=True)), TrainEngine(_model(deterministic=True))
        la, ga = _step(a, ids, lab, aux, sizes, cw)
        lb, gb = _step(b, *junk, sizes, cw)
        assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(a.model._flat, b.model._flat)


def test_bf16_step_is_close_to_fp32(canvases):
    ids, lab, aux, sizes = canvases
    out = {}
    for dtype in ("fp32", "bf16"):
        eng = TrainEngine(_model(dtype), lr=0.0)
        loss, _ = _step(eng, ids, lab, aux, sizes)
        out[dtype] = (loss.tolist(), float(eng.grad_norm))
    print(out)
    for got, ref in zip(out["bf16"][0], out["fp32"][0]):
        assert abs(got - ref) <= 3e-2 * abs(ref), (got, ref)
    assert abs(out["bf16"][1] - out["fp32"][1]) <= 3e-2 * out["fp32"][1], out


def test_guards(canvases):
    ids, lab, aux, sizes = canvases
    m = _model()
    with pytest.raises(RuntimeError, match="eager"):
        TrainEngine(m, use_graph=True).step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
    with pytest.raises(RuntimeError, match="eager"):
        TrainEngine(m, use_graph=True).step_kv(T.gold_tables())
    with pytest.raises(ValueError, match="n_class"):
        TrainEngine(m).step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=[1.0] * (NCLS - 1))


def test_it_trains(gold):
    eng = TrainEngine(_model())
    losses = []
    for _ in range(20):
        losses.append(eng.step_kv(gold[0]).clone())
    torch.cuda.synchronize()
    losses = torch.stack(losses).cpu().double()
    print(losses[:, 0].tolist())
    assert bool(torch.isfinite(losses).all())
    for l3 in losses.tolist():
        assert abs(l3[0] - (0.5 * l3[1] + 0.5 * l3[2])) <= 1e-6 * abs(l3[0]), l3
    assert float(losses[-1, 0]) < float(losses[0, 0])
