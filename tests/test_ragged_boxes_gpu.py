"""GPU: ragged batches from BOX LISTS -- the painters with `sizes` (msau_raster_owner_ext), the box-list instance of the first conv
under MSAU_CONV_EXTENT, `TrainEngine.step_boxes(..., sizes=)`, `step_ids(..., sizes=)` and `MSAUWrapper.confusion_matrix_boxes`.
Configuration, documents and the error measure are those of tests/test_ragged_gpu.py; "ragged equals alone" keeps its tolerances
(1e-5 on the fp32 loss, 1e-4 on the fp32 gradient), box-fed against painted keeps those of
tests/test_train_gpu.py::test_first_conv_fed_with_box_lists_matches_the_painted_grid (1e-3 fp32, 2e-2 bf16 on gradients)."""
import numpy as np
import pytest
import torch

from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.data import raster
from msau_amd.data.ragged import pack, pack_boxes, pack_ids

from . import ragged_boxes_util as U
from .test_ragged_gpu import CH, DOCS, KW, NCLS, _docs, _rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _box_doc(rng, h, w, n, C, cross=True):
    """one document as box lists in its own coordinates: text-line-like boxes, overlapping, with `cross` some over its edges; the
    first box lies inside, so every document has labelled pixels"""
    fb, lb = [], []
    for i in range(n):
        if i == 0:
            y0, x0 = int(rng.integers(0, max(h - 2, 1))), int(rng.integers(0, max(w - 3, 1)))
        else:
            y0, x0 = int(rng.integers(-2 if cross else 0, h)), int(rng.integers(-3 if cross else 0, w))
        y1, x1 = y0 + int(rng.integers(1, 6)), x0 + int(rng.integers(2, 14))
        fb.append((0, y0, y1, x0, x1, i))
        lb.append((0, y0, y1, x0, x1, int(rng.integers(1, NCLS))))
    return (np.asarray(fb, np.int32).reshape(-1, 6), np.asarray(lb, np.int32).reshape(-1, 6), h, w,
            rng.standard_normal((max(n, 1), C)).astype(np.float32))


def _model(C, dtype="fp32", **extra):
    return MSAUWrapper(C, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


def _host_docs(docs):
    """every document painted alone on the host (numpy slicing on its own array) as the FUNSD loader's items"""
    out = []
    for fb, lb, h, w, feats in docs:
        sizes = [(h, w)]
        x = U.dense_ragged(fb, feats, sizes, h, w)[0].transpose(2, 0, 1)
        out.append({"mask": torch.from_numpy(np.ascontiguousarray(x))[None], "label": torch.from_numpy(U.labels_ragged(lb, sizes, h, w)).float()})
    return out


# ---- 1. the painters with sizes -------------------------------------------------------------------------------------------------
def test_painters_with_sizes_equal_the_cpu_restatement_and_leave_nothing_outside():
    rng = np.random.default_rng(3)
    C = 13
    docs = [_box_doc(rng, 37, 29, 16, C), _box_doc(rng, 40, 40, 0, C), _box_doc(rng, 21, 33, 16, C), _box_doc(rng, 8, 6, 4, C)]
    between = np.asarray([(0, 5, 9, 31, 44, 0), (0, 39, 47, 2, 9, 1), (0, 30, 45, 20, 45, 2)], np.int32)   # beside / below / straddling document 0
    docs[0] = (np.concatenate([docs[0][0], between]), np.concatenate([docs[0][1], between]), 37, 29, docs[0][4])
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    B, sz = len(docs), sizes.tolist()
    assert (H, W) == (48, 48)
    want_owner, want_lab = U.owner_ragged(gb, sz, H, W), U.labels_ragged(lb, sz, H, W)
    want_dense = torch.from_numpy(U.dense_ragged(gb, feats, sz, H, W))
    cb = gb.copy()
    cb[:, 5] = rng.integers(-1, C + 2, len(cb))                 # character ids: -1 and ids beyond the charset paint zeros
    want_hot = torch.from_numpy(U.onehot_ragged(cb, sz, H, W, C))
    ext_dev = sizes.to(torch.int32).to(DEV).contiguous()        # sizes already resident: taken as they are
    outside = torch.ones((B, H, W), dtype=torch.bool)
    for b, (h, w) in enumerate(sz):
        outside[b, :h, :w] = False
    assert bool(outside.any())
    for given in (sizes, ext_dev):
        owner, fbt, nf, labels = raster.owner_maps(gb, lb, B, H, W, DEV, sizes=given)
        torch.cuda.synchronize()
        assert nf == len(gb) and np.array_equal(owner.cpu().numpy(), want_owner)
        assert np.array_equal(labels.cpu().numpy(), want_lab)
        assert bool((owner.cpu()[outside] == -1).all()) and int(labels.cpu()[outside].abs().sum()) == 0
        for dtype, td in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            grid, lab2 = raster.rasterize_dense(gb, lb, feats, B, H, W, dtype, DEV, sizes=given)
            hot, lab3 = raster.rasterize(cb, lb, B, H, W, C, dtype, DEV, sizes=given)
            torch.cuda.synchronize()
            assert grid.dtype == td and torch.equal(grid[..., :C].cpu(), want_dense.to(td))        # bit for bit in the storage type
            assert torch.equal(hot[..., :C].cpu(), want_hot.to(td))
            assert float(grid[..., C:].float().abs().sum()) == 0.0 and float(hot[..., C:].float().abs().sum()) == 0.0
            assert float(grid.cpu()[outside].float().abs().max()) == 0.0 and float(hot.cpu()[outside].float().abs().max()) == 0.0
            assert np.array_equal(lab2.cpu().numpy(), want_lab) and np.array_equal(lab3.cpu().numpy(), want_lab)
    # the restatement differs from clipping to the canvas, which is what the painters do without sizes
    owner0, _, _, _ = raster.owner_maps(gb, lb, B, H, W, DEV)
    assert bool((owner0.cpu()[outside] >= 0).any())
    with pytest.raises(ValueError, match="1 <= h <= 48"):
        raster.owner_maps(gb, lb, B, H, W, DEV, sizes=[[49, 3]] * B)


# ---- 2. ragged step_boxes = the mean of the documents ---------------------------------------------------------------------------
def _step_boxes(m, gb, lb, B, H, W, feats, sizes=None, eng=None):
    eng = eng or TrainEngine(m, lr=0.0)
    loss = eng.step_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes)
    torch.cuda.synchronize()
    return float(loss), eng.flat_grad.clone().cpu(), eng


def test_fp32_ragged_step_boxes_is_the_mean_of_the_documents_and_never_paints_the_grid():
    rng = np.random.default_rng(7)
    shapes = DOCS + [(8, 6)]                                    # 8 x 6: one pixel at the bottleneck
    docs = [_box_doc(rng, h, w, 4 if h < 10 else 14, CH) for h, w in shapes]
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    m = _model(CH)
    loss, grad, _ = _step_boxes(m, gb, lb, len(docs), H, W, feats, sizes)
    plan = m._plan_for_shape(len(docs), H, W, DEV, True, ragged=True)
    assert plan._owner_keep is not None                         # the box-list instance ran: the grid was not painted
    losses, grads = [], []
    for fb1, lb1, h, w, f1 in docs:
        l1, g1, _ = _step_boxes(m, fb1, lb1, 1, h, w, f1)
        assert m._plan_for_shape(1, h, w, DEV, True)._owner_keep is not None
        losses.append(l1)
        grads.append(g1)
    ref_loss, ref_grad = sum(losses) / len(losses), sum(grads) / len(grads)
    print("ragged step_boxes against the documents alone: loss", loss, ref_loss, "gradient", _rel(grad, ref_grad))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert _rel(grad, ref_grad) <= 1e-4, _rel(grad, ref_grad)


# ---- 3. the same ragged batch three ways ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,C", [("fp32", 24), ("fp32", 33), ("fp32", 100), ("bf16", 24), ("bf16", 33), ("bf16", 100)])
def test_ragged_batch_box_fed_device_painted_and_host_painted_agree(dtype, C, monkeypatch):
    rng = np.random.default_rng(11)
    docs = [_box_doc(rng, h, w, 14, C) for h, w in DOCS] + [_box_doc(rng, 30, 44, 0, C)]      # the last document is empty
    docs[1][0][3, 5] = 0                                        # feature row 0 of document 1 is shared by two boxes
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    B = len(docs)
    x, labels, s2 = pack(_host_docs(docs), round_to=16)
    assert tuple(x.shape) == (B, C, H, W) and torch.equal(s2, sizes)
    res = {}
    for mode in ("owner", "painted", "host"):
        monkeypatch.setenv("MSAU_OWNER_CONV", "0" if mode == "painted" else "1")
        m = _model(C, dtype, deterministic=True)
        eng = TrainEngine(m)
        losses, first = [], None
        for k in range(3):
            if mode == "host":
                losses.append(float(eng.step(x.to(DEV), labels.to(DEV), sizes)))
            else:
                losses.append(float(eng.step_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes)))
            if k == 0:
                first = eng.flat_grad.float().cpu()             # the gradient of the FIRST step: the same parameters on every path
        torch.cuda.synchronize()
        plan = m._plan_for_shape(B, H, W, DEV, True, ragged=True)
        assert (getattr(plan, "_owner_keep", None) is not None) == (mode == "owner")
        c = next(op for op in plan.ops if getattr(op, "x1", None) is plan.x_in)
        wo, bo, n = plan.poff[c.wname], plan.poff[c.bname], int(np.prod(plan.pshape[c.wname]))
        g = eng.flat_grad.float().cpu()
        res[mode] = (losses, first, m.flat_parameters.float().cpu(), first[wo:wo + n].clone(), first[bo:bo + 8].clone(), g)
    bf = dtype == "bf16"
    tol = 2e-2 if bf else 1e-3
    for a, b in (("owner", "painted"), ("owner", "host"), ("painted", "host")):
        ra, rb = res[a], res[b]
        figs = dict(loss=max(abs(p - q) / abs(q) for p, q in zip(ra[0], rb[0])), w=_rel(ra[3], rb[3]), b=_rel(ra[4], rb[4]),
                    grad=_rel(ra[1], rb[1]), params=_rel(ra[2], rb[2]), grad_third_step=_rel(ra[5], rb[5]))
        print(dtype, C, a, "against", b, figs)
        assert float(rb[3].abs().max()) > 0 and float(rb[4].abs().max()) > 0
        assert figs["loss"] < (2e-3 if bf else 1e-5), (a, b, ra[0], rb[0])
        assert figs["w"] < tol and figs["b"] < tol and figs["grad"] < tol, (a, b, figs)
        assert figs["params"] < (1e-3 if bf else 1e-5), (a, b, figs)


# ---- 4. garbage outside the extents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner_conv", ["1", "0"])
def test_boxes_outside_their_document_change_nothing(owner_conv, monkeypatch):
    monkeypatch.setenv("MSAU_OWNER_CONV", owner_conv)
    rng = np.random.default_rng(13)
    docs = [_box_doc(rng, h, w, 12, CH, cross=True) for h, w in DOCS]
    for b, (h, w) in enumerate(DOCS):                           # wholly between the document and the canvas edge, and straddling it
        extra = [(0, 1, 6, w, 48, 0), (0, h, 48, 0, 9, 1), (0, h - 3, h + 4, w - 4, w + 5, 2), (0, h + 1, 47, w + 1, 47, 3)]
        extra = np.asarray(extra, np.int32)
        lab = extra.copy()
        lab[:, 5] = rng.integers(1, NCLS, len(extra))
        docs[b] = (np.concatenate([docs[b][0], extra]), np.concatenate([docs[b][1], lab]), h, w, docs[b][4])
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    assert (H, W) == (48, 48)

    def clipped(bx):                                            # the clean list: every box clipped to its document on the host
        out = bx.copy()
        hs, ws = sizes[:, 0].numpy()[bx[:, 0]], sizes[:, 1].numpy()[bx[:, 0]]
        out[:, 1], out[:, 2] = np.clip(bx[:, 1], 0, hs), np.clip(bx[:, 2], 0, hs)
        out[:, 3], out[:, 4] = np.clip(bx[:, 3], 0, ws), np.clip(bx[:, 4], 0, ws)
        return out
    gc, lc = clipped(gb), clipped(lb)
    assert not np.array_equal(gc, gb) and int(((gc[:, 2] <= gc[:, 1]) | (gc[:, 4] <= gc[:, 3])).sum()) >= 2 * len(DOCS)
    m = _model(CH, deterministic=True)
    l0, g0, eng = _step_boxes(m, gc, lc, len(docs), H, W, feats, sizes)
    l1, g1, _ = _step_boxes(m, gb, lb, len(docs), H, W, feats, sizes, eng=eng)
    plan = m._plan_for_shape(len(docs), H, W, DEV, True, ragged=True)
    assert (getattr(plan, "_owner_keep", None) is not None) == (owner_conv == "1")
    assert l0 == l1 and torch.equal(g0, g1) and float(g0.abs().max()) > 0
    # and without sizes the same list is another batch: the extra boxes are painted
    l2, g2, _ = _step_boxes(m, gb, lb, len(docs), H, W, feats)
    assert l2 != l0


# ---- 5. step_ids with sizes -----------------------------------------------------------------------------------------------------
def test_ragged_step_ids_equals_the_one_hot_canvas_bit_for_bit():
    docs = _docs(DOCS, seed=5)
    x, labels, sizes = pack(docs, round_to=16)
    masks = [torch.where(d["mask"][0].sum(0) > 0, d["mask"][0].argmax(0), torch.tensor(-1)).to(torch.int32) for d in docs]
    ids, s2 = pack_ids(masks, round_to=16)
    assert torch.equal(s2, sizes) and tuple(ids.shape) == (3, 48, 48)
    g = torch.Generator().manual_seed(6)
    junk = torch.randint(0, CH, ids.shape, generator=g, dtype=torch.int32)     # valid characters outside the documents: ignored
    lab_junk = torch.randint(1, NCLS, labels.shape, generator=g)
    lab2 = labels.clone()
    for b, (h, w) in enumerate(sizes.tolist()):
        keep, lkeep = ids[b, :h, :w].clone(), labels[b, :h, :w].clone()
        ids[b], lab2[b] = junk[b], lab_junk[b]
        ids[b, :h, :w], lab2[b, :h, :w] = keep, lkeep
    m = _model(CH, deterministic=True)
    eng = TrainEngine(m, lr=0.0)
    l0 = float(eng.step(x.to(DEV), labels.to(DEV), sizes))
    torch.cuda.synchronize()
    g0 = eng.flat_grad.clone().cpu()
    l1 = float(eng.step_ids(ids.to(DEV), lab2.to(DEV), sizes))
    torch.cuda.synchronize()
    g1 = eng.flat_grad.clone().cpu()
    assert l0 == l1 and torch.equal(g0, g1) and float(g0.abs().max()) > 0
    l2 = float(eng.step_ids(ids.to(DEV), lab2.to(DEV)))         # the dense step on the same canvas sees the junk
    assert l2 != l0


# ---- 6. evaluation from box lists -----------------------------------------------------------------------------------------------
def test_confusion_matrix_boxes(monkeypatch):
    rng = np.random.default_rng(17)
    C = 24
    docs = [_box_doc(rng, h, w, 14, C) for h, w in DOCS] + [_box_doc(rng, 30, 44, 0, C)]
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    B = len(docs)
    x, labels, _ = pack(_host_docs(docs), round_to=16)
    cms = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MSAU_OWNER_CONV", mode)
        m = _model(C).eval()
        want = m.confusion_matrix(x.to(DEV), labels.to(DEV), sizes=sizes).cpu()
        want_z = m.confusion_matrix(x.to(DEV), labels.to(DEV), sizes=sizes, zero_as=2).cpu()
        got = m.confusion_matrix_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes)
        assert got.dtype == torch.int64 and tuple(got.shape) == (NCLS, NCLS)
        again = m.confusion_matrix_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes, out=got)            # accumulates on the device
        assert again is got
        got_z = m.confusion_matrix_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes, zero_as=2).cpu()
        torch.cuda.synchronize()
        got = got.cpu()
        assert int(want.sum()) == int((labels > 0).sum()) > 0 and int(want[0].sum()) == 0
        assert torch.equal(got.sum(1), 2 * want.sum(1)) and int(got.sum()) == 2 * int(want.sum())      # label counts and the total
        assert torch.equal(got_z.sum(1), want_z.sum(1)) and int(got_z[:, 0].sum()) == 0
        if mode == "0":                                         # painted on the device: the same tensor enters the same kernels
            assert torch.equal(got, 2 * want) and torch.equal(got_z, want_z)
        else:                                                   # box-fed first conv: other order of the fp32 sums, near-ties may move
            moved = int((got - 2 * want).abs().sum()) // 4
            print("confusion_matrix_boxes, box-fed first conv: pixels counted in another column than on the painted grid:",
                  moved, "of", int(want.sum()))
        # the plan is left tensor-fed: the dense-grid entry point still gives its counts
        assert torch.equal(m.confusion_matrix(x.to(DEV), labels.to(DEV), sizes=sizes).cpu(), want)
        cms[mode] = want
    assert torch.equal(cms["0"], cms["1"])
    # dense batch (sizes None) and one-hot character boxes (feats None)
    m = _model(CH).eval()
    cdocs = [(d[0], d[1], d[2], d[3]) for d in (_box_doc(rng, h, w, 14, CH) for h, w in DOCS)]
    for d in cdocs:
        d[0][:, 5] = rng.integers(0, CH, len(d[0]))
    cb, clb, none, csizes, (Hc, Wc) = pack_boxes(cdocs)
    hot = torch.from_numpy(U.onehot_ragged(cb, csizes.tolist(), Hc, Wc, CH)).permute(0, 3, 1, 2).contiguous()
    clab = torch.from_numpy(U.labels_ragged(clb, csizes.tolist(), Hc, Wc))
    assert none is None and torch.equal(m.confusion_matrix_boxes(cb, clb, 3, Hc, Wc, sizes=csizes).cpu(),
                                        m.confusion_matrix(hot.to(DEV), clab.to(DEV), sizes=csizes).cpu())
    full = [[Hc, Wc]] * 3
    hot_d = torch.from_numpy(U.onehot_ragged(cb, full, Hc, Wc, CH)).permute(0, 3, 1, 2).contiguous()
    clab_d = torch.from_numpy(U.labels_ragged(clb, full, Hc, Wc))
    assert torch.equal(m.confusion_matrix_boxes(cb, clb, 3, Hc, Wc).cpu(), m.confusion_matrix(hot_d.to(DEV), clab_d.to(DEV)).cpu())


def test_predict_unfeeds_the_box_lists_a_confusion_count_left_in_the_plan(monkeypatch):
    """`confusion_matrix_boxes` leaves the forward-only plan's first conv on the box lists; `Plan.predict` of the same plan puts it back
    on the tensor itself and gives the bits of a model that never saw a box list"""
    monkeypatch.setenv("MSAU_OWNER_CONV", "1")
    rng = np.random.default_rng(23)
    C = 24
    docs = [_box_doc(rng, h, w, 14, C) for h, w in DOCS]
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    B = len(docs)
    assert (B, H, W) == (3, 48, 48)
    x = pack(_host_docs(docs), round_to=16)[0].to(DEV)
    m = _model(C).eval()
    m.confusion_matrix_boxes(gb, lb, B, H, W, feats=feats, sizes=sizes)
    plan = m._plan_for_shape(B, H, W, DEV, False, ragged=True)
    assert plan._owner_keep is not None                         # nobody un-fed it
    probs, amax = (t.clone() for t in m.predict_nhwc(inp=x, sizes=sizes))
    assert plan._owner_keep is None
    want_probs, want_amax = (t.clone() for t in _model(C).eval().predict_nhwc(inp=x, sizes=sizes))
    torch.cuda.synchronize()
    assert torch.equal(probs, want_probs) and torch.equal(amax, want_amax)
    assert float(want_probs.abs().max()) > 0


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_ragged_box_feeds_refuse_what_they_do_not_implement():
    rng = np.random.default_rng(19)
    docs = [_box_doc(rng, h, w, 6, CH) for h, w in DOCS]
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    m = _model(CH)
    with pytest.raises(RuntimeError, match="use_graph=False"):
        TrainEngine(m, use_graph=True).step_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes)
    eng = TrainEngine(m, lr=0.0)
    with pytest.raises(NotImplementedError, match="dense batches only"):
        eng.prefetch_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes)
    with pytest.raises(ValueError, match="1 <= h <= 48 and 1 <= w <= 48"):
        eng.step_boxes(gb, lb, 3, H, W, feats=feats, sizes=[[49, 3], [1, 1], [1, 1]])
    with pytest.raises(ValueError, match=r"shape \(3, 2\)"):
        eng.step_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes[:2])
    with pytest.raises(ValueError, match="1 <= h <= 48 and 1 <= w <= 48"):
        eng.step_ids(torch.zeros((3, H, W), dtype=torch.int32, device=DEV), torch.zeros((3, H, W), device=DEV), sizes=[[4, 50], [1, 1], [1, 1]])
    with pytest.raises(ValueError, match="1 <= h <= 48"):
        m.confusion_matrix_boxes(gb, lb, 3, H, W, feats=feats, sizes=[[0, 3], [1, 1], [1, 1]])
    from msau_amd.model_box import BMSAUWrapper
    mb = BMSAUWrapper(CH, NCLS, dict(scale_space_num=3, final_act="softmax", num_blocks=1, seed=0)).to(DEV)
    with pytest.raises(NotImplementedError, match="ragged"):
        TrainEngine(mb, lr=0.0).step_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes)
    with pytest.raises(NotImplementedError, match="ragged"):
        mb.confusion_matrix_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes)
    # nothing above left the engine unusable
    assert np.isfinite(float(eng.step_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes)))
