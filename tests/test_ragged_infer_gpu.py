"""GPU: the forward-only end of ragged batches -- the extent-aware id painter, the device confusion counts, predict_nhwc and
confusion_matrix on ragged canvases, KVModel.run_test in ragged groups and the training script's batched evaluation."""
import argparse
import json
import math
import os

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper
from msau_amd.data.ragged import pack, pack_ids
from msau_amd.inference import KVModel
from msau_amd.inference.generic_util import to_categorical
from oracle import msau_oracle as O
from tests.golden_util import GOLDEN, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KV = os.path.join(GOLDEN, "kv")
CH, NCLS = 13, 5
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
SIZES = [(37, 29), (40, 44), (21, 33)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _model(dtype="fp32", ch=CH, ncls=NCLS):
    return MSAUWrapper(ch, ncls, dict(KW, dtype=dtype)).to(DEV).eval()


def _inside(sizes, B, H, W):
    m = torch.zeros((B, H, W), dtype=torch.bool)
    for b, (h, w) in enumerate(torch.as_tensor(sizes).tolist()):
        m[b, :h, :w] = True
    return m


def _host_counts(logits_nhwc, labels, C, zero_as=None, inside=None):
    """bincount of (label, torch.argmax of the fp32 logits) over labels in [1, C) (and inside the documents)"""
    pred = logits_nhwc[..., :C].float().to(DEV).argmax(-1).cpu()
    keep = (labels >= 1) & (labels < C)
    if inside is not None:
        keep &= inside
    if zero_as is not None:
        pred = torch.where(pred == 0, torch.full_like(pred, zero_as), pred)
    return torch.bincount(labels[keep] * C + pred[keep], minlength=C * C).reshape(C, C)


def _margin(logits_nhwc, C):
    """top-2 gap of the first C channels"""
    top2 = logits_nhwc[..., :C].float().topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


# ---- kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [2, 5, 17, 64])
def test_eval_confusion_kernel_matches_host_argmax(dtype, C):
    g = torch.Generator().manual_seed(C)
    B, H, W = 3, 37, 29
    Cs = -(-C // 8) * 8 + 8                                              # padded channels beyond the real ones
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    lg = torch.randn((B, H, W, Cs), generator=g) * 2
    coarse = torch.randint(-2, 3, (B, H, W, Cs), generator=g).float() * 0.5
    lg[1] = coarse[1]                                                     # sample 1: exact ties everywhere
    lg[0, 3, :, :C] = 1.25                                                # a full tie: the first index wins
    lg[..., C:] = 100.0                                                   # padded channels are never candidates
    lg = lg.to(td)
    labels = torch.randint(0, C, (B, H, W), generator=g)
    sizes = torch.tensor([[37, 29], [20, 11], [5, 29]])
    inside = _inside(sizes, B, H, W)
    garbage = torch.randint(-5, C + 5, (B, H, W), generator=g)
    labels = torch.where(inside, labels, garbage)                         # outside the extents: anything
    ext = sizes.to(torch.int32).to(DEV).contiguous()
    dlg, dlab = lg.to(DEV).contiguous(), labels.to(DEV).contiguous()
    for use_ext in (False, True):
        for zero_as in (None, C - 1):
            counts = torch.zeros((C, C), dtype=torch.int64, device=DEV)
            for _ in range(2):                                            # two calls accumulate into one matrix
                L.call("msau_eval_confusion", _stream(), L.F32 if dtype == "fp32" else L.BF16, dlg.data_ptr(), dlab.data_ptr(),
                       counts.data_ptr(), B, H, W, C, Cs, -1 if zero_as is None else zero_as,
                       ext.data_ptr() if use_ext else None)
            want = 2 * _host_counts(lg, labels, C, zero_as, inside if use_ext else None)
            assert torch.equal(counts.cpu(), want), (use_ext, zero_as)
    with pytest.raises(L.MsauHipError):
        L.call("msau_eval_confusion", _stream(), L.F32, dlg.data_ptr(), dlab.data_ptr(), dlab.data_ptr(), B, H, W, 65, 72, -1, None)


@pytest.mark.parametrize("dtype,C", [("bf16", 17), ("fp32", 64)])
def test_eval_confusion_kernel_on_a_large_canvas(dtype, C):
    """more pixels than 512 workgroups x 256 lanes x 4: every lane loops over several pixels and every workgroup's histogram
    gathers many strides before it is flushed"""
    g = torch.Generator().manual_seed(100 + C)
    B, H, W = 16, 200, 180
    assert B * H * W > 512 * 256 * 4
    Cs = -(-C // 8) * 8
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    lg = (torch.randn((B, H, W, Cs), generator=g) * 2).to(td)
    lg[::3, ::2] = (torch.randint(-2, 3, lg[::3, ::2].shape, generator=g).float() * 0.5).to(td)     # exact ties
    sizes = torch.randint(1, H + 1, (B, 2), generator=g)
    sizes[:, 1] = torch.randint(1, W + 1, (B,), generator=g)
    sizes[0] = torch.tensor([H, W])
    inside = _inside(sizes, B, H, W)
    labels = torch.where(inside, torch.randint(0, C, (B, H, W), generator=g), torch.randint(-9, C + 9, (B, H, W), generator=g))
    ext = sizes.to(torch.int32).to(DEV).contiguous()
    dlg, dlab = lg.to(DEV).contiguous(), labels.to(DEV).contiguous()
    for use_ext, zero_as in ((True, None), (False, 1)):
        counts = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        L.call("msau_eval_confusion", _stream(), L.F32 if dtype == "fp32" else L.BF16, dlg.data_ptr(), dlab.data_ptr(),
               counts.data_ptr(), B, H, W, C, Cs, -1 if zero_as is None else zero_as, ext.data_ptr() if use_ext else None)
        want = _host_counts(lg, labels, C, zero_as, inside if use_ext else None)
        assert int(want.sum()) > 100000 and torch.equal(counts.cpu(), want), (use_ext, zero_as)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 60])
def test_onehot_ids_ext_zero_outside(dtype, C):
    g = torch.Generator().manual_seed(C)
    B, H, W = 3, 23, 31
    Cs = -(-C // 8) * 8
    ids = torch.randint(-1, C + 3, (B, H, W), generator=g, dtype=torch.int32)       # out-of-range ids paint nothing
    sizes = torch.tensor([[23, 31], [9, 30], [1, 1]])
    inside = _inside(sizes, B, H, W)
    t = torch.full((B, H, W, Cs), 7.0, dtype=torch.float32 if dtype == "fp32" else torch.bfloat16, device=DEV)
    dids, ext = ids.to(DEV), sizes.to(torch.int32).to(DEV)                         # (alive until the kernel has run)
    L.call("msau_onehot_ids_ext", _stream(), L.F32 if dtype == "fp32" else L.BF16, dids.data_ptr(), t.data_ptr(),
           B, H, W, C, Cs, ext.data_ptr())
    want = np.zeros((B, H, W, Cs), np.float32)
    ok = ((ids >= 0) & (ids < C) & inside).numpy()
    want[..., :C][ok] = to_categorical(ids.numpy()[ok], C)
    assert np.array_equal(t.float().cpu().numpy(), want)


# ---- predict_nhwc ----------------------------------------------------------------------------------------------------------
def _id_masks(sizes, ch, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in sizes:
        occ = torch.rand((h, w), generator=g) < 0.4
        out.append(torch.where(occ, torch.randint(0, ch, (h, w), generator=g), torch.zeros((h, w), dtype=torch.int64)).int())
    return out


def test_predict_nhwc_ragged_equals_each_document_alone():
    m = _model("fp32")
    masks = _id_masks(SIZES, CH)
    ids, sizes = pack_ids(masks)
    assert tuple(ids.shape) == (3, 48, 48)
    pr, am = (t.clone() for t in m.predict_nhwc(ids=ids.to(DEV), sizes=sizes))
    for b, mk in enumerate(masks):
        h, w = mk.shape
        p1, a1 = m.predict_nhwc(ids=mk[None].to(DEV))
        crop, cam = pr[b, :h, :w], am[b, :h, :w]
        assert _rel(crop, p1[0]) <= 1e-5, (b, _rel(crop, p1[0]))
        sure = _margin(p1[0], NCLS) > 1e-4
        assert torch.equal(cam[sure].cpu(), a1[0][sure].cpu())
    # the dense tensor on the same ragged plan: the same bits
    dense = torch.zeros((3, CH, 48, 48))
    for b, mk in enumerate(masks):
        dense[b, :, :mk.shape[0], :mk.shape[1]] = torch.from_numpy(to_categorical(mk.numpy(), CH)).permute(2, 0, 1)
    pd, ad = m.predict_nhwc(inp=dense.to(DEV), sizes=sizes)
    assert torch.equal(pd, pr) and torch.equal(ad, am)
    # garbage outside the documents leaves the crops bit-identical
    g = torch.Generator().manual_seed(9)
    noisy = torch.where(_inside(sizes, 3, 48, 48), ids, torch.randint(-3, CH + 3, ids.shape, generator=g, dtype=torch.int32))
    pn, an = (t.clone() for t in m.predict_nhwc(ids=noisy.to(DEV), sizes=sizes))
    noisy_dense = dense + (~_inside(sizes, 3, 48, 48))[:, None].float() * torch.rand(dense.shape, generator=g)
    pnd, _ = m.predict_nhwc(inp=noisy_dense.to(DEV), sizes=sizes)
    for b, (h, w) in enumerate(sizes.tolist()):
        assert torch.equal(pn[b, :h, :w], pr[b, :h, :w]) and torch.equal(an[b, :h, :w], am[b, :h, :w])
        assert torch.equal(pnd[b, :h, :w], pr[b, :h, :w])


def test_predict_nhwc_ragged_graph_replay():
    m = _model("fp32")
    s1 = [(37, 29), (40, 44), (21, 33)]
    s2 = [(48, 48), (17, 40), (33, 9)]                                    # the same 48 x 48 canvas
    for sz in (s1, s2, s1):
        ids, sizes = pack_ids(_id_masks(sz, CH, seed=len(sz) + sz[0][0]))
        assert tuple(ids.shape) == (3, 48, 48)
        pe, ae = (t.clone() for t in m.predict_nhwc(ids=ids.to(DEV), sizes=sizes))
        torch.cuda.synchronize()
        pg, ag = m.predict_nhwc(ids=ids.to(DEV), sizes=sizes, graph=True)
        for b, (h, w) in enumerate(sizes.tolist()):
            assert torch.equal(pg[b, :h, :w], pe[b, :h, :w]) and torch.equal(ag[b, :h, :w], ae[b, :h, :w])
    plan = m._plan_for_shape(3, 48, 48, DEV, False, ragged=True)
    assert list(plan._pgraphs) == ["ids"]                                # one graph per canvas and input kind


# ---- confusion_matrix --------------------------------------------------------------------------------------------------------
def _docs(shapes, seed=1, ch=CH, ncls=NCLS):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        occ = torch.rand((1, h, w), generator=g) < 0.3
        ids = torch.randint(0, ch, (1, h, w), generator=g)
        x = torch.zeros((1, ch, h, w))
        x.scatter_(1, ids.unsqueeze(1), occ.unsqueeze(1).float())
        lab = (occ * torch.randint(1, ncls, (1, h, w), generator=g)).long()
        out.append({"mask": x, "label": lab})
    return out


def _today_counts(m, docs, zero_as=None):
    """the arithmetic of the evaluate() this replaces: batch-1 forward, NCHW fp32 logits, torch argmax, .cpu()"""
    cm = np.zeros((m.n_class, m.n_class), np.int64)
    with torch.no_grad():
        for d in docs:
            lab = np.squeeze(d["label"].long().numpy())
            _, ypred, _ = m(d["mask"].float().to(DEV))
            idx = ypred.squeeze(0).argmax(0).cpu().numpy()
            idx, lab = idx[lab != 0], lab[lab != 0]
            if zero_as is not None:
                idx[idx == 0] = zero_as
            np.add.at(cm, (lab, idx), 1)
    return cm


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_confusion_matrix_dense_equals_todays_evaluate(dtype):
    m = _model(dtype)
    docs = _docs(SIZES)
    for zero_as in (None, 3):
        cm = torch.zeros((NCLS, NCLS), dtype=torch.int64, device=DEV)
        for d in docs:
            r = m.confusion_matrix(d["mask"].to(DEV), d["label"], zero_as=zero_as, out=cm)
            assert r is cm
        assert np.array_equal(cm.cpu().numpy(), _today_counts(m, docs, zero_as))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_confusion_matrix_ragged(dtype):
    m = _model(dtype)
    docs = _docs(SIZES)
    x, labels, sizes = pack(docs)
    B, _, H, W = x.shape
    inside = _inside(sizes, B, H, W)
    g = torch.Generator().manual_seed(5)
    noisy = torch.where(inside, labels, torch.randint(-3, NCLS + 3, labels.shape, generator=g))     # ignored outside
    cm = m.confusion_matrix(x.to(DEV), noisy.to(DEV), sizes=sizes).cpu()
    # exactly the host count over the same ragged forward's exported logits
    with torch.no_grad():
        _, lg, _ = m(x.to(DEV), sizes)
    nhwc = lg.permute(0, 2, 3, 1).cpu()
    assert torch.equal(cm, _host_counts(nhwc, labels, NCLS, None, inside))
    # against every document alone: only pixels whose top-2 margin is below 1e-4 may move
    alone = torch.from_numpy(_today_counts(m, docs))
    near = 0
    for b, d in enumerate(docs):
        with torch.no_grad():
            _, l1, _ = m(d["mask"].to(DEV))
        lab = d["label"][0]
        near += int(((_margin(l1[0].permute(1, 2, 0).cpu(), NCLS) < 1e-4) & (lab > 0)).sum())
    assert int((cm - alone).abs().sum()) <= 2 * near, (cm, alone, near)


# ---- KVModel -----------------------------------------------------------------------------------------------------------------
def _kv_model(dtype, tmp_path):
    meta = json.load(open(os.path.join(KV, "kv.json")))
    cfg, seed = meta["net"]["cfg"], meta["net"]["seed"]
    wpath = str(tmp_path / f"kv_weights_{dtype}.pt")
    torch.save(O.init_params(cfg, seed), wpath)
    km = KVModel()
    km.load(model_weight=wpath, charset=os.path.join(KV, "charset.txt"), n_class=meta["n_class"], dtype=dtype,
            model_kwargs=dict(featRoot=cfg["featRoot"], scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                              filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax"))
    return km


def test_kvmodel_run_test_batched_equals_batch_one(tmp_path, capsys):
    km = _kv_model("fp32", tmp_path)
    files = [os.path.join(KV, f"layout{i}.json") for i in range(3)]
    # ground truth for layouts 0 and 2 only: layout 1's missing label file is reported next to layout 1 at every batch size
    labels = tmp_path / "labels"
    labels.mkdir()
    for i in (0, 2):
        (labels / f"layout{i}.json").write_text(open(files[i]).read())
    r1 = km.run_test(files, str(tmp_path), label_dir=str(labels))
    e1 = json.loads(json.dumps(km.eval_results))
    out1 = capsys.readouterr().out
    lines = out1.splitlines()
    assert lines.index("layout1") == lines.index("layout0") + 3 and lines[lines.index("layout1") - 1].startswith("Error reading CA")
    assert sum(c["num_label"] for c in e1) > 0
    for bs in (3, 2):                                          # one full group; a group of 2 and a group of 1
        r = km.run_test(files, str(tmp_path), label_dir=str(labels), batch_size=bs)
        e = json.loads(json.dumps(km.eval_results))
        out = capsys.readouterr().out
        assert r == r1 and e == e1 and out == out1, bs


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kvmodel_batched_crop_matches_reference_prediction(dtype, tmp_path):
    g = np.load(os.path.join(KV, "kv.npz"))
    km = _kv_model(dtype, tmp_path)
    masks = [km._generate_masks_from_label(os.path.join(KV, f"layout{i}.json"))[0] for i in range(3)]
    assert np.array_equal(masks[0], g["d0.input_mask"])
    outs = km._run_net_batch(masks)
    a_pred, a_cls = outs[0]
    want = g["net.pred_nhwc"]
    assert a_pred.shape == want.shape and a_pred.dtype == np.float32
    assert rel_err(a_pred, want) < (2e-4 if dtype == "fp32" else 6e-2)
    assert np.array_equal(a_cls, np.argmax(a_pred, -1))
    for (p, c), mk in zip(outs, masks):
        assert p.shape[:2] == mk.shape and c.shape == mk.shape


# ---- the training script ---------------------------------------------------------------------------------------------------
def _script_args(tmp_path, **kw):
    a = dict(loop="engine", lr=1e-4, clip=1.0, num_epochs=1, batch_size=1, eval_batch_size=1, ckptdir=str(tmp_path / "ckpt"),
             bmname=None, hidden_dim=500, dataset="invoice", method="GCN", output_dim=NCLS)
    a.update(kw)
    os.makedirs(a["ckptdir"], exist_ok=True)
    return argparse.Namespace(**a)


def test_training_script_batched_evaluate_and_ragged_epoch(tmp_path, capsys):
    import train_chargrid_funsd_msau as T
    m = _model("fp32")
    docs = _docs([(30 + 7 * (i % 5), 20 + 9 * (i % 4)) for i in range(11)], seed=4)
    args = _script_args(tmp_path)
    labels_map = {"header": 0, "question": 1, "answer": 2, "other": 3}
    for kw in (dict(max_num_examples=6), dict(testing=True, labels_map=labels_map)):
        r1 = T.evaluate(docs, m, args, batch_size=1, **kw)
        r4 = T.evaluate(docs, m, args, batch_size=4, **kw)
        n = T.eval_count(len(docs), kw.get("max_num_examples"))
        near, total = 0, 0
        for d in docs[:n]:
            with torch.no_grad():
                _, l1, _ = m(d["mask"].to(DEV))
            lab = d["label"][0]
            near += int(((_margin(l1[0].permute(1, 2, 0).cpu(), NCLS) < 1e-4) & (lab > 0)).sum())
            total += int((lab > 0).sum())
        assert abs(r4["acc"] - r1["acc"]) * total <= near + 1e-6, (r1, r4, near)
        assert r1["prec"] == r1["recall"] == r1["acc"]
    out = capsys.readouterr().out
    assert "weighted avg" in out and "macro avg" in out
    # one ragged epoch of the engine loop
    args = _script_args(tmp_path, batch_size=4, eval_batch_size=4)
    T.train(docs, m, args, val_dataset=docs[:3], test_dataset=docs[3:6], labels_map=labels_map)
    out = capsys.readouterr().out
    loss = float(out.split("Avg loss: ")[1].split(";")[0])
    assert math.isfinite(loss) and loss > 0
    assert os.path.exists(os.path.join(args.ckptdir, f"invoice_GCN_h500_o{NCLS}.pth.tar"))      # the epoch-0 state_dict


@pytest.mark.parametrize("opts", [[], ["--batch-size", "2", "--eval-batch-size", "2"]])
def test_training_script_main_end_to_end(tmp_path, monkeypatch, capsys, opts):
    """the script as run from the command line: preprocessed pickles -> one epoch -> evaluation with the report -> checkpoints"""
    import pickle
    import train_chargrid_funsd_msau as T
    from msau_amd.data.funsd import get_preprocessed_list_word_msau
    monkeypatch.chdir(tmp_path)
    inv = None
    for split in ("train", "test"):                           # the test split takes the training split's charset
        docs, inv = get_preprocessed_list_word_msau(os.path.join(GOLDEN, "funsd", split), inv)
        with open(f"{split}.pkl", "wb") as fh:
            pickle.dump(docs, fh)
    T.main(["--train-pickle", "train.pkl", "--test-pickle", "test.pkl", "--num-epochs", "1", "--dtype", "fp32",
            "--ckptdir", "ck"] + opts)
    out = capsys.readouterr().out
    assert "Finished" in out and "Train  accuracy:" in out and "Test  accuracy:" in out and "weighted avg" in out
    loss = float(out.split("Avg loss: ")[1].split(";")[0])
    assert math.isfinite(loss) and loss > 0
    assert any(f.endswith(".pth.tar") for f in os.listdir("ck"))
