"""GPU: key-value validation on the device -- msau_unet_eval against the float64 host statement (tests/kv_eval_util.py) and against
the training kernel's loss, `MSAUWrapper.eval_unet` / `eval_kv` against the exported logits and UNetLoss, the ragged rule,
`TrainEngine.step_unet(stats=...)` and the epoch loop `KVTrainer.fit`."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import UNetLoss
from msau_amd.training import kv_data as D
from msau_amd.training.kv_trainer import KVTrainer, summarize
from tests import glyphs_util as U
from tests import kv_eval_util as E
from tests import kv_train_util as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = 60, T.N_CLASS
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
B, H, W = 3, 37, 29
EXTENTS = [(37, 29), (20, 11), (1, 1)]
TIES = [(0, 0, 3), (3, 10, 1), (19, 10, 2), (36, 28, 3)]                    # (y, x, label) in document 0: first and last rows included


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1: the kernel against the host statement ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(C, dtype, ragged):
    """-> (logits [2] of [B,H,W,Cs] in storage dtype, labels [2] int64, extents or None, class weights), CPU tensors, left unchanged.
    Document 1's final labels are all 0 (labelled = 0), the 1 x 1 document's final label is the zero-weight class 2, a few pixels of
    document 0 carry two equal top logits; ragged: outside the extents labels -1, logits garbage, one +inf"""
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    Cs = -(-C // 8) * 8
    g = torch.Generator().manual_seed(100 + C)
    logits = [(torch.randn(B, H, W, Cs, generator=g) * 2).to(td) for _ in range(2)]
    labs = [torch.randint(0, C, (B, H, W), generator=g) for _ in range(2)]
    for t in range(2):
        for y, x, lab in TIES:                                             # two equal maxima: the first one is the prediction
            lo, hi = (lab, lab + 1) if (y + t) % 2 else (lab - 1, lab)
            logits[t][0, y, x, lo], logits[t][0, y, x, hi] = 50.0, 50.0
            labs[t][0, y, x] = lab
    labs[0][1] = 0
    labs[0][2, 0, 0], labs[1][2, 0, 0] = 2, 3
    cw = torch.rand(C, generator=g) + 0.5
    cw[2] = 0.0
    ext = None
    if ragged:
        ext = EXTENTS
        for b, (h, w) in enumerate(EXTENTS):
            for t in range(2):
                keep_l, keep_x = labs[t][b, :h, :w].clone(), logits[t][b, :h, :w].clone()
                labs[t][b] = -1
                logits[t][b] = (torch.randn(H, W, Cs, generator=g) * 1e4).to(td)
                if h < H:
                    logits[t][b, h, 0] = float("inf")
                labs[t][b, :h, :w], logits[t][b, :h, :w] = keep_l, keep_x
    return logits, labs, ext, cw


def _run_eval(dt, lg_d, lab_d, ext_d, cw_d, with_aux, K, C, Cs):
    loss = torch.full((B, 2), 123.0, device=DEV)
    counts = torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
    ws = torch.full((int(L.load().msau_unet_eval_ws_bytes(B, K)),), 0xAB, dtype=torch.uint8, device=DEV)
    L.call("msau_unet_eval", _stream(), dt, lg_d[0].data_ptr(), lg_d[1].data_ptr() if with_aux else None, lab_d[0].data_ptr(),
           lab_d[1].data_ptr() if with_aux else None, ext_d.data_ptr() if ext_d is not None else None,
           cw_d.data_ptr() if cw_d is not None else None, K, loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
    torch.cuda.synchronize()
    return loss.cpu(), counts.cpu()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 12, 17, 40])
def test_kernel_equals_host_statement(C, dtype):
    Cs = -(-C // 8) * 8
    dt = L.F32 if dtype == "fp32" else L.BF16
    tol = 1e-5 if dtype == "fp32" else 1e-2
    for ragged in (True, False):
        logits, labs, ext, cw = _inputs(C, dtype, ragged)
        lg_d, lab_d = [x.to(DEV) for x in logits], [x.to(DEV) for x in labs]
        ext_d = torch.tensor(ext, dtype=torch.int32, device=DEV) if ragged else None
        for with_aux in (True, False):
            for weighted in (False, True):
                ref_loss, ref_counts, near = E.unet_eval_host(
                    logits[0].double().numpy()[..., :C], logits[1].double().numpy()[..., :C] if with_aux else None, labs[0].numpy(),
                    labs[1].numpy() if with_aux else None, ext, cw.tolist() if weighted else None)
                what = (C, dtype, ragged, with_aux, weighted)
                assert ref_counts[1, 0, 0] == 0 and ref_counts[0, 0, 0] > 0 and near[0, 0] >= len(TIES), what
                if ragged and weighted:
                    assert ref_loss[2, 0] == 0.0 and (not with_aux or ref_loss[2, 1] > 0), what      # D_b = 0, final head only
                for K in (1, 4, 7):
                    loss, counts = _run_eval(dt, lg_d, lab_d, ext_d, cw.to(DEV) if weighted else None, with_aux, K, C, Cs)
                    loss2, counts2 = _run_eval(dt, lg_d, lab_d, ext_d, cw.to(DEV) if weighted else None, with_aux, K, C, Cs)
                    err = float(np.max(np.abs(loss.double().numpy() - ref_loss) / np.maximum(np.abs(ref_loss), 1e-30)))
                    print(what, "K", K, "loss rel err", err, "counts", counts[:, 0].tolist())
                    assert np.array_equal(counts.numpy().astype(np.int64), ref_counts), (what, K, counts.tolist(), ref_counts.tolist())
                    assert bool(torch.isfinite(loss).all()) and err <= tol, (what, K, loss.tolist(), ref_loss.tolist())
                    assert torch.equal(loss, loss2) and torch.equal(counts, counts2), (what, K)
                    if not with_aux:
                        assert float(loss[:, 1].abs().max()) == 0.0 and int(counts[:, 1].abs().max()) == 0, (what, K)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_register_form_equals_cache_form(dtype):
    """the same 17 real logits stored at Cs = 24 (a pixel in registers) and zero-padded to Cs = 40 (a pixel read from the cache): the
    two forms share one statement of a pixel's log-sum-exp (loss.hip) -- the same loss bits and the same counts"""
    C = 17
    dt = L.F32 if dtype == "fp32" else L.BF16
    for ragged in (True, False):
        logits, labs, ext, cw = _inputs(C, dtype, ragged)
        lab_d = [x.to(DEV) for x in labs]
        ext_d = torch.tensor(ext, dtype=torch.int32, device=DEV) if ragged else None
        got = {}
        for Cs in (24, 40):
            lg_d = []
            for x in logits:
                p = torch.zeros(B, H, W, Cs, dtype=x.dtype)
                p[..., :C] = x[..., :C]
                lg_d.append(p.to(DEV))
            for with_aux in (True, False):
                for weighted in (False, True):
                    for K in (1, 4, 7):
                        got[(Cs, with_aux, weighted, K)] = _run_eval(dt, lg_d, lab_d, ext_d, cw.to(DEV) if weighted else None, with_aux, K, C, Cs)
        for (Cs, *what), (loss, counts) in got.items():
            if Cs != 24:
                continue
            wide_loss, wide_counts = got[(40, *what)]
            assert torch.equal(loss, wide_loss) and torch.equal(counts, wide_counts), (ragged, what, loss.tolist(), wide_loss.tolist())
            assert bool(torch.isfinite(loss).all()) and float(loss[0, 0]) > 0 and int(counts[0, 0, 0]) > 0, (ragged, what)


def test_kernel_refuses_bad_arguments():
    x = torch.zeros(64, device=DEV)
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    for K, Bn, Cs in ((0, 1, 8), (257, 1, 8), (1, 1025, 8), (1, 1, 12)):
        with pytest.raises(L.MsauHipError, match="unet_eval"):
            L.call("msau_unet_eval", _stream(), L.F32, x.data_ptr(), None, lab.data_ptr(), None, None, None, K, x.data_ptr(), x.data_ptr(),
                   x.data_ptr(), Bn, 1, 1, 5, Cs)


# ---- 2: the same loss as the training kernel ------------------------------------------------------------------------------------------
def test_mean_of_documents_is_the_training_loss():
    C, Cs, K = 17, 24, 4
    ws = torch.zeros(int(L.load().msau_unet_ce_ws_floats(B * H * W)), device=DEV)
    for ragged in (True, False):
        logits, labs, ext, cw = _inputs(C, "fp32", ragged)
        lg_d, lab_d = [x.to(DEV) for x in logits], [x.to(DEV) for x in labs]
        ext_d = torch.tensor(ext, dtype=torch.int32, device=DEV) if ragged else None
        for weighted in (False, True):
            cw_d = cw.to(DEV) if weighted else None
            hist = torch.zeros((2, B, K, C), dtype=torch.int32, device=DEV)
            if weighted:
                for t in range(2):
                    L.call("msau_label_hist", _stream(), lab_d[t].data_ptr(), ext_d.data_ptr() if ragged else None, hist[t].data_ptr(),
                           B, H, W, C, K)
            loss3 = torch.zeros(3, device=DEV)
            d = [torch.empty_like(x) for x in lg_d]
            L.call("msau_unet_ce", _stream(), L.F32, lg_d[0].data_ptr(), lg_d[1].data_ptr(), lab_d[0].data_ptr(), lab_d[1].data_ptr(),
                   ext_d.data_ptr() if ragged else None, cw_d.data_ptr() if weighted else None, hist.data_ptr() if weighted else None, K,
                   d[0].data_ptr(), d[1].data_ptr(), loss3.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
            loss, _counts = _run_eval(L.F32, lg_d, lab_d, ext_d, cw_d, True, K, C, Cs)
            got = loss.double().mean(dim=0).tolist()
            want = loss3.cpu().double().tolist()
            print((ragged, weighted), "eval", got, "training", want)
            for t in range(2):
                assert abs(got[t] - want[1 + t]) <= 1e-5 * abs(want[1 + t]), (ragged, weighted, t, got, want)
            assert abs(0.5 * got[0] + 0.5 * got[1] - want[0]) <= 1e-5 * abs(want[0])


# ---- 3 - 7: the model -----------------------------------------------------------------------------------------------------------------
def _model(dtype="fp32", **extra):
    return MSAUWrapper(CH, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


@pytest.fixture(scope="module")
def gold():
    return T.gold_tables(0)


@pytest.fixture(scope="module")
def canvases(gold):
    """the three golden documents on one canvas, as CPU tensors; shared and left unchanged"""
    ids, lab, aux, sizes = T.canvases_want(gold)
    return torch.from_numpy(ids), torch.from_numpy(lab), torch.from_numpy(aux), torch.from_numpy(sizes)


CWT = [0.0, 2.0] + [0.5 + 0.1 * c for c in range(NCLS - 2)]


def _one_hot(t, n):
    return F.one_hot(t.long().clamp(min=0), n).permute(0, 3, 1, 2).float().to(DEV)      # (-1 outside the documents: ignored there)


def _exports(m, ids, sizes):
    """the fp32 logits `forward` returns, as [B,H,W,C] float64 numpy"""
    with torch.no_grad():
        _, lg, ax = m(_one_hot(ids, CH), sizes)
    torch.cuda.synchronize()
    return [x.permute(0, 2, 3, 1).double().cpu().numpy() for x in (lg, ax)], (lg, ax)


def _rows(pair):
    torch.cuda.synchronize()
    return pair[0].cpu().clone(), pair[1].cpu().clone()


def _assert_rows(got, ref_loss, ref_counts, tol, what):
    loss, counts = got
    err = float(np.max(np.abs(loss.double().numpy() - ref_loss) / np.maximum(np.abs(ref_loss), 1e-30)))
    print(what, "loss rel err", err, "counts", counts[:, 0].tolist(), "ref", ref_counts[:, 0].tolist())
    assert np.array_equal(counts.numpy().astype(np.int64), ref_counts), (what, counts.tolist(), ref_counts.tolist())
    assert err <= tol, (what, loss.tolist(), ref_loss.tolist())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_unet_equals_host_statement_on_exported_logits(canvases, dtype):
    ids, lab, aux, sizes = canvases
    tol = 1e-5 if dtype == "fp32" else 1e-2
    m = _model(dtype)
    before = m._flat.clone()
    for cw in (None, CWT):
        got = _rows(m.eval_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw))
        (lg, ax), _ = _exports(m, ids, sizes)
        ref_loss, ref_counts, _near = E.unet_eval_host(lg, ax, lab.numpy(), aux.numpy(), sizes.tolist(), cw)
        assert ref_counts[:, :, 0].min() > 0
        _assert_rows(got, ref_loss, ref_counts, tol, (dtype, cw is not None))
    assert torch.equal(m._flat, before)
    assert m._plans and all(not key[3] for key in m._plans)               # no training plan for any shape
    assert all(p.grad is None for _, p in m._named)


def test_eval_unet_at_batch_one_is_unet_loss(canvases):
    ids, lab, aux, sizes = canvases
    h, w = sizes[0].tolist()
    ids1, lab1, aux1 = ids[:1, :h, :w].contiguous(), lab[:1, :h, :w].contiguous(), aux[:1, :h, :w].contiguous()
    m = _model()
    for cw in (None, CWT):
        s = summarize(*m.eval_unet(ids1.to(DEV), lab1.to(DEV), aux1.to(DEV), class_weights=cw))
        _, (lg, ax) = _exports(m, ids1, None)
        crit = UNetLoss({"class_weights": cw} if cw is not None else {}).to(DEV)
        acc, total, final = crit(lg, _one_hot(lab1, NCLS), {"aux_logits": ax, "aux_tgt": _one_hot(aux1, NCLS)})
        print("summarize", s, "UNetLoss", acc, float(total), float(final))
        assert s["documents"] == 1 and s["unlabelled"] == 0
        assert abs(s["acc"] - acc) < 1e-6
        assert abs(s["loss"] - float(total)) <= 1e-5 * abs(float(total))
        assert abs(s["final"] - float(final)) <= 1e-5 * abs(float(final))


def _near_bound(m, ids, lab, aux, sizes):
    """labelled pixels (both heads) whose top-2 margin is below 1e-4 in the documents' own forward, and all labelled pixels"""
    near = labelled = 0
    for b, (h, w) in enumerate(sizes.tolist()):
        (lg, ax), _ = _exports(m, ids[b:b + 1, :h, :w].contiguous(), None)
        _l, c, n = E.unet_eval_host(lg, ax, lab[b:b + 1, :h, :w].numpy(), aux[b:b + 1, :h, :w].numpy())
        near += int(n.sum())
        labelled += int(c[:, :, 0].sum())
    return near, labelled


def test_ragged_group_is_the_documents_alone(canvases):
    ids, lab, aux, sizes = canvases
    m = _model()
    loss, counts = _rows(m.eval_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=CWT))
    alone = []
    for b, (h, w) in enumerate(sizes.tolist()):
        alone.append(_rows(m.eval_unet(ids[b:b + 1, :h, :w].contiguous().to(DEV), lab[b:b + 1, :h, :w].contiguous().to(DEV),
                                       aux[b:b + 1, :h, :w].contiguous().to(DEV), class_weights=CWT)))
    loss1, counts1 = torch.cat([a[0] for a in alone]), torch.cat([a[1] for a in alone])
    near, labelled = _near_bound(m, ids, lab, aux, sizes)
    moved = int((counts.long() - counts1.long()).abs().sum())
    print("near", near, "of labelled", labelled, "moved", moved, "loss", loss.tolist(), "alone", loss1.tolist())
    assert labelled > 0 and near < 0.01 * labelled                        # otherwise the bound below proves nothing
    assert torch.equal(counts[:, :, 0], counts1[:, :, 0])                  # the labelled pixels are the documents' own
    assert moved <= 2 * near, (counts.tolist(), counts1.tolist(), near)
    for got, ref in zip(loss.reshape(-1).tolist(), loss1.reshape(-1).tolist()):
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_kv_gives_the_bits_of_eval_unet_on_the_canvases(gold, canvases, dtype):
    ids, lab, aux, sizes = canvases
    m = _model(dtype)
    a = _rows(m.eval_kv(gold, class_weights=CWT))
    b = _rows(m.eval_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=CWT))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].min()) > 0 and int(a[1][:, :, 0].min()) > 0


def test_step_with_stats_is_the_step_and_the_rows_are_eval_unet(canvases):
    ids, lab, aux, sizes = canvases
    dev = [t.to(DEV) for t in (ids, lab, aux)]
    a, b = TrainEngine(_model(deterministic=True)), TrainEngine(_model(deterministic=True))
    fresh = _model()
    assert torch.equal(a.model._flat, b.model._flat) and torch.equal(a.model._flat, fresh._flat)
    stats = (torch.full((3, 2), 123.0, device=DEV), torch.full((3, 2, 2), 77, dtype=torch.int32, device=DEV))
    la = a.step_unet(*dev, sizes=sizes, class_weights=CWT)
    lb = b.step_unet(*dev, sizes=sizes, class_weights=CWT, stats=stats)
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(a.flat_grad, b.flat_grad) and torch.equal(a.model._flat, b.model._flat)
    assert not torch.equal(a.model._flat, fresh._flat)
    got = _rows(stats)
    ref = _rows(fresh.eval_unet(*dev, sizes=sizes, class_weights=CWT))      # the weights before the step
    near, labelled = _near_bound(fresh, ids, lab, aux, sizes)
    moved = int((got[1].long() - ref[1].long()).abs().sum())
    print("near", near, "of labelled", labelled, "moved", moved, "rows", got[0].tolist(), "eval_unet", ref[0].tolist())
    assert near < 0.01 * labelled and moved <= 2 * near and torch.equal(got[1][:, :, 0], ref[1][:, :, 0])
    for g_, r in zip(got[0].reshape(-1).tolist(), ref[0].reshape(-1).tolist()):
        assert abs(g_ - r) <= 1e-5 * abs(r), (g_, r)
    # the step's own loss is the mean of the rows
    l3 = la.cpu().double().tolist()
    assert abs(float(got[0][:, 0].double().mean()) - l3[1]) <= 1e-5 * l3[1] and abs(float(got[0][:, 1].double().mean()) - l3[2]) <= 1e-5 * l3[2]


def test_fit_one_epoch(tmp_path, capsys):
    paths = [T.gold_path(di) for di in range(3)]
    batches = D.KVTrainBatches(paths, os.path.join(U.KV, "charset.txt"), NCLS, batch_size=3, seed=4)
    m = _model()
    start = m._flat.clone()
    tr = KVTrainer(m, batches, class_weights=CWT)
    hist = tr.fit(str(tmp_path), 1, 2)
    out = capsys.readouterr().out
    print(out)
    assert len(hist) == 1 and hist[0]["epoch"] == 1 and hist[0]["lr"] == 1e-3 and tr.engine.lr == 1e-3
    assert not torch.equal(m._flat, start)
    assert hist[0]["train"]["documents"] == 6 and hist[0]["val"]["documents"] == 3 and hist[0]["val"]["unlabelled"] == 0
    assert "TRAIN: Epoch 1, Acc: " in out and "VAL: Epoch 1, Acc: " in out and "Saving checkpoint" in out
    rows = [m.eval_kv(g_, class_weights=CWT) for g_ in batches.validation()]
    want = summarize(torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]))
    assert hist[0]["val"] == want and np.isfinite(want["loss"]) and want["loss"] > 0
    saved = os.path.join(str(tmp_path), "model1")
    assert hist[0]["saved"] == saved and os.path.exists(saved)
    m2 = _model()
    assert not torch.equal(m2._flat, m._flat)
    m2.load_weights(saved)
    assert torch.equal(m2._flat, m._flat)
    for g_, r in zip(batches.validation(), rows):
        again = m2.eval_kv(g_, class_weights=CWT)
        torch.cuda.synchronize()
        assert torch.equal(again[0], r[0]) and torch.equal(again[1], r[1])
