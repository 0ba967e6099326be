"""GPU: entity-level predictions by box vote -- direct calls of `msau_box_vote` on the case table of tests/box_vote_util.py against
`box_vote_host`, a cross-check against `msau_eval_confusion` that does not go through the oracle, and `MSAUWrapper.box_predictions`
/ `box_predictions_boxes` / the training script's --entity-level evaluation on the golden FUNSD documents.  Every comparison is
integer equality: the oracle takes the argmax of the very values the kernel reads (the fp32 export of bf16 logits is exact)."""
import argparse

import numpy as np
import pytest
import torch

from msau_amd import MSAUWrapper
from msau_amd import _lib as L
from msau_amd.data import entities as E
from msau_amd.data import raster
from msau_amd.data.ragged import pack, pack_boxes

from . import box_vote_util as U
from . import ragged_boxes_util as RU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _logits_dev(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t.bfloat16() if dtype == "bf16" else t).to(DEV).contiguous()        # the table's values are exact in bf16


def _vote(lg, dtype, bx, Cn, Cs, zero_as=None, owned=False, extent=None, hist=True, counts=None, count=True):
    """one call of msau_box_vote with guarded outputs -> (pred, votes, hist or None, counts tensor or None, owner map or None)"""
    n = len(bx)
    bt = torch.from_numpy(np.ascontiguousarray(bx, np.int32)).to(DEV)
    ext = None if extent is None else torch.from_numpy(np.ascontiguousarray(extent, np.int32)).to(DEV)
    owner = None
    if owned:                                                   # the map msau_raster_owner[_ext] writes for this list
        owner = torch.empty((U.B, U.H, U.W), dtype=torch.int32, device=DEV)
        raster._owner(_stream(), bt, n, owner, U.B, U.H, U.W, ext)
    shapes = {"pred": (n,), "votes": (n, 2), "hist": (n, Cn)}
    bufs = {k: torch.from_numpy(U.guarded(s)).to(DEV) for k, s in shapes.items()}
    at = lambda k: bufs[k].data_ptr() + 4 * U.GUARD
    if count and counts is None:
        counts = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
    L.call("msau_box_vote", _stream(), L.F32 if dtype == "f32" else L.BF16, lg.data_ptr(), bt.data_ptr(), n,
           owner.data_ptr() if owned else None, at("pred"), at("votes"), at("hist") if hist else None,
           counts.data_ptr() if count else None, U.B, U.H, U.W, Cn, Cs, -1 if zero_as is None else zero_as,
           ext.data_ptr() if ext is not None else None)
    torch.cuda.synchronize()
    back = {k: b.cpu().numpy() for k, b in bufs.items()}
    if not hist:
        assert (back["hist"] == U.SENTINEL).all()
    return (U.check_guarded(back["pred"], shapes["pred"], "pred"), U.check_guarded(back["votes"], shapes["votes"], "votes"),
            U.check_guarded(back["hist"], shapes["hist"], "hist") if hist else None, counts if count else None, owner)


def _out(got):
    return got[0], got[1], got[2], None if got[3] is None else got[3].cpu().numpy()


# ---- direct calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("Cn,Cs", U.COMBOS)
def test_box_vote_on_the_table(Cn, Cs, dtype):
    bx, _tie, _big = U.boxes(Cn)
    for kind in U.KINDS:
        x = U.logits(kind, Cn, Cs, dtype)
        lg = _logits_dev(x, dtype)
        for zero_as, extent, owned in U.settings():
            got = _vote(lg, dtype, bx, Cn, Cs, zero_as, owned, extent)
            owner = None
            if owned:
                owner = E.owner_host(bx, U.B, U.H, U.W, extent)
                assert np.array_equal(got[4].cpu().numpy(), owner)
            want = E.box_vote_host(x, bx, Cn, zero_as, owner, extent)
            U.assert_same(_out(got), want, f"{kind} {dtype} C={Cn} zero_as={zero_as} extent={extent is not None} owned={owned}")


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("Cn,Cs", U.COMBOS)
def test_histograms_of_owned_boxes_add_up_to_the_pixel_confusion_counts(Cn, Cs, dtype):
    """with the owner map every labelled pixel votes for the box that painted its label, so the histograms of the boxes of value v
    add up to row v of what msau_eval_confusion counts on the labels msau_raster_labels paints from the same map"""
    bx, _tie, _big = U.boxes(Cn)
    lg = _logits_dev(U.logits("random", Cn, Cs, dtype), dtype)
    for zero_as in (None, 1):
        for extent in (None, U.EXTENT):
            _pred, _votes, hist, _counts, owner = _vote(lg, dtype, bx, Cn, Cs, zero_as, True, extent)
            bt = torch.from_numpy(bx).to(DEV)
            labels = torch.empty((U.B, U.H, U.W), dtype=torch.int64, device=DEV)
            L.call("msau_raster_labels", _stream(), bt.data_ptr(), owner.data_ptr(), labels.data_ptr(), U.B, U.H, U.W)
            cm = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
            ext = None if extent is None else torch.from_numpy(extent).to(DEV)
            L.call("msau_eval_confusion", _stream(), L.F32 if dtype == "f32" else L.BF16, lg.data_ptr(), labels.data_ptr(), cm.data_ptr(),
                   U.B, U.H, U.W, Cn, Cs, -1 if zero_as is None else zero_as, ext.data_ptr() if ext is not None else None)
            torch.cuda.synchronize()
            cm = cm.cpu().numpy()
            rows = np.zeros((Cn, Cn), np.int64)
            for i, v in enumerate(bx[:, 5].tolist()):
                if 1 <= v < Cn:
                    rows[v] += hist[i]
            assert int(cm.sum()) > 0 and np.array_equal(rows, cm), (zero_as, extent is not None)


def test_optional_outputs_many_boxes_and_accumulation():
    Cn, Cs, dtype = 5, 8, "bf16"
    bx, _tie, _big = U.boxes(Cn)
    x = U.logits("random", Cn, Cs, dtype)
    lg = _logits_dev(x, dtype)
    want = E.box_vote_host(x, bx, Cn)
    U.assert_same(_out(_vote(lg, dtype, bx, Cn, Cs, hist=False)), want, "hist = NULL")
    U.assert_same(_out(_vote(lg, dtype, bx, Cn, Cs, count=False)), want, "counts = NULL")
    for cn, cs in ((5, 8), (64, 64)):                                   # more groups than the launch has workgroups
        xm = U.logits("random", cn, cs, "f32")
        many = U.many_boxes(cn)
        U.assert_same(_out(_vote(_logits_dev(xm, "f32"), "f32", many, cn, cs)), E.box_vote_host(xm, many, cn), f"5000 boxes, C={cn}")
    many = U.many_boxes(Cn)
    counts = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
    _vote(lg, dtype, bx, Cn, Cs, counts=counts)
    _vote(lg, dtype, many, Cn, Cs, zero_as=1, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), want[3] + E.box_vote_host(x, many, Cn, zero_as=1)[3])


def test_refused_arguments_and_the_empty_list():
    lib = L.load()
    lg = torch.zeros((U.B, U.H, U.W, 72), dtype=torch.float32, device=DEV)
    bt = torch.zeros((2, 6), dtype=torch.int32, device=DEV)
    pred = torch.full((2,), U.SENTINEL, dtype=torch.int32, device=DEV)
    votes = torch.full((2, 2), U.SENTINEL, dtype=torch.int32, device=DEV)

    def call(n=2, Cn=5, Cs=8, zero_as=-1, pr=pred, vt=votes):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.msau_box_vote(_stream(), L.F32, lg.data_ptr(), bt.data_ptr(), n, None, p(pr), p(vt), None, None, U.B, U.H, U.W, Cn, Cs,
                               zero_as, None)
        return rc, lib.msau_last_error().decode()

    for kw, word in ((dict(Cn=65, Cs=72), "C = 65"), (dict(zero_as=5), "zero_as = 5"), (dict(pr=None), "null")):
        rc, msg = call(**kw)
        assert rc == -1 and "box_vote" in msg and word in msg, (kw, rc, msg)
    assert call(n=0)[0] == 0 and call(n=0, pr=None, vt=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((pred == U.SENTINEL).all()) and bool((votes == U.SENTINEL).all())
    assert call()[0] == 0                                               # two empty boxes
    torch.cuda.synchronize()
    assert pred.tolist() == [-1, -1] and votes.tolist() == [[0, 0], [0, 0]]


# ---- end to end on the golden documents -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    docs, n_chars = RU.golden_documents(tmp_path_factory.mktemp("box_vote_golden"))
    out = []
    for dense, chars, i in docs:
        cb, lb, h, w = raster.document_boxes(chars.inp_list[i])
        item = chars[i]
        assert tuple(item["mask"].shape[2:]) == (h, w)
        out.append(dict(item, boxes=lb, chars=cb, words=raster.document_word_boxes(chars.inp_list[i]), h=h, w=w,
                        lines=raster.document_line_boxes(dense.inp_list[i]) + (np.asarray(dense.inp_list[i]["transformer_feature"], np.float32),)))
    n_class = 1 + max(int(d["boxes"][:, 5].max()) for d in out)
    return out, n_chars, n_class


def _want(m, x, boxes, sizes, zero_as, owned):
    """box_vote_host on the logits `forward` exports for the same input"""
    with torch.no_grad():
        _, logits, _ = m(x, sizes)
    nhwc = logits.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    B, H, W = nhwc.shape[:3]
    ext = None if sizes is None else np.asarray(sizes)
    owner = E.owner_host(boxes, B, H, W, ext) if owned else None
    return E.box_vote_host(nhwc, boxes, m.n_class, zero_as, owner, ext)


@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
def test_box_predictions_on_golden_documents(golden, dtype):
    docs, n_chars, n_class = golden
    m = MSAUWrapper(n_chars, n_class, dict(KW, dtype=dtype)).to(DEV).eval()
    x3, _lab, sizes = pack(docs[:3], round_to=16)
    cb3, lb3, none, sizes_b, (H, W) = pack_boxes([(d["chars"], d["boxes"], d["h"], d["w"]) for d in docs[:3]])
    _cb, wb3, _, _, _ = pack_boxes([(d["chars"], d["words"], d["h"], d["w"]) for d in docs[:3]])
    assert none is None and torch.equal(sizes, sizes_b) and tuple(x3.shape[2:]) == (H, W)
    d0 = docs[0]
    cases = [("dense", d0["mask"].float().to(DEV), None, d0["boxes"], d0["chars"], (1, d0["h"], d0["w"])),
             ("ragged", x3.to(DEV), sizes, lb3, cb3, (3, H, W)),
             ("ragged words", x3.to(DEV), sizes, wb3, cb3, (3, H, W))]
    for name, x, sz, boxes, chars, (B, Hc, Wc) in cases:
        for owned in (False, True):
            for zero_as in (None, 1):
                want = _want(m, x, boxes, sz, zero_as, owned)
                total = torch.zeros((n_class, n_class), dtype=torch.int64, device=DEV)
                pred, votes, hist = m.box_predictions(x, boxes, sizes=sz, zero_as=zero_as, owned=owned, out=total, hist=True)
                p2, v2, h2 = m.box_predictions(x, torch.from_numpy(boxes).to(DEV), sizes=sz, zero_as=zero_as, owned=owned, out=total)
                assert pred.dtype == votes.dtype == hist.dtype == torch.int32 and h2 is None
                assert tuple(votes.shape) == (len(boxes), 2) and tuple(hist.shape) == (len(boxes), n_class)
                U.assert_same((pred.cpu().numpy(), votes.cpu().numpy(), hist.cpu().numpy(), None), want, f"{name} owned={owned}")
                assert torch.equal(p2, pred) and torch.equal(v2, votes)
                assert np.array_equal(total.cpu().numpy(), 2 * want[3]), (name, owned, zero_as)         # two calls accumulate
                assert int(want[3].sum()) == len(boxes) - int((want[0] < 0).sum()) > 0
                # the box-list feed: the label boxes are the voted boxes (the grid is painted on the device: the same tensor
                # enters the same kernels)
                total.zero_()
                pb, vb, hb = m.box_predictions_boxes(chars, boxes, B, Hc, Wc, sizes=sz, zero_as=zero_as, owned=owned, out=total, hist=True)
                U.assert_same((pb.cpu().numpy(), vb.cpu().numpy(), hb.cpu().numpy(), total.cpu().numpy()), want, f"{name} boxes owned={owned}")
    none_pred = m.box_predictions(cases[0][1], np.zeros((0, 6), np.int32), hist=True)
    assert [tuple(t.shape) for t in none_pred] == [(0,), (0, 2), (0, n_class)]
    with pytest.raises(ValueError, match="zero_as"):
        m.box_predictions(cases[0][1], d0["boxes"], zero_as=n_class)
    with pytest.raises(ValueError, match="out must be"):
        m.box_predictions(cases[0][1], d0["boxes"], out=torch.zeros((n_class, n_class), dtype=torch.int32, device=DEV))


def test_box_predictions_boxes_with_a_feature_table(golden):
    """the dense (text-line embedding) feed: the first conv may read the box lists themselves, whose fp32 sums run in another order
    than on a painted grid, so the oracle takes the logits the plan holds -- the values the vote read"""
    docs, _n_chars, n_class = golden
    gb, lb, feats, sizes, (H, W) = pack_boxes([d["lines"] for d in docs[:3]])
    m = MSAUWrapper(feats.shape[1], n_class, dict(KW, dtype="bf16")).to(DEV).eval()
    ext = sizes.numpy()
    for owned in (False, True):
        total = torch.zeros((n_class, n_class), dtype=torch.int64, device=DEV)
        pred, votes, hist = m.box_predictions_boxes(gb, lb, 3, H, W, feats=feats, sizes=sizes, zero_as=1, owned=owned, out=total, hist=True)
        lg = m._plan_for_shape(3, H, W, DEV, False, ragged=True).logits
        nhwc = lg.data.reshape(3, H, W, lg.Cs).float().cpu().numpy()
        want = E.box_vote_host(nhwc, lb, n_class, 1, E.owner_host(lb, 3, H, W, ext) if owned else None, ext)
        U.assert_same((pred.cpu().numpy(), votes.cpu().numpy(), hist.cpu().numpy(), total.cpu().numpy()), want, f"owned={owned}")
        assert int(want[3].sum()) > 0


def test_training_script_entity_level_evaluate(golden, capsys):
    import train_chargrid_funsd_msau as T
    docs, n_chars, n_class = golden
    m = MSAUWrapper(n_chars, n_class, dict(KW, dtype="bf16")).to(DEV).eval()
    labels_map = {"l%d" % i: i for i in range(n_class - 2)}
    labels_map["other"] = n_class - 2
    zero_as = labels_map["other"]
    want = sum(_want(m, d["mask"].float().to(DEV), d["boxes"], None, zero_as, False)[3] for d in docs)
    plain = T.evaluate(docs, m, argparse.Namespace(eval_batch_size=1), testing=True, name="Test", labels_map=labels_map)
    quiet = capsys.readouterr().out
    assert "entity" not in quiet and set(plain) == {"prec", "recall", "acc"}
    for bs in (1, 3):
        res = T.evaluate(docs, m, argparse.Namespace(eval_batch_size=bs, entity_level=True), testing=True, name="Test", labels_map=labels_map)
        out = capsys.readouterr().out
        assert "Test  entity accuracy: " in out and out.count("weighted avg") == 2
        if bs == 1:                                             # the documents alone: the very forwards `want` was taken from
            assert out.startswith(quiet)                        # what the script prints without the flag, then the entity report
            assert np.array_equal(res["entity_matrix"], want)
            assert res["entity_acc"] == float(np.trace(want)) / int(want.sum())
        assert int(res["entity_matrix"].sum()) == int(want.sum()) > 0
