"""Host side of ragged inference and evaluation: the metrics from a confusion matrix against sklearn, pack_ids, the documents
the training script evaluates, and the refusals of predict_nhwc(sizes=...) / confusion_matrix without a GPU."""
import argparse
import warnings

import numpy as np
import pytest
import torch

from msau_amd import MSAUWrapper
from msau_amd.data.ragged import pack, pack_ids
from msau_amd.training.metrics import classification_report, scores

KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)


def _cm(labels, preds, C):
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (np.asarray(labels), np.asarray(preds)), 1)
    return cm


# ---- metrics ---------------------------------------------------------------------------------------------------------------
def test_report_hand_computed():
    # labels 1 1 2 2 2 3, predictions 1 2 2 2 0 3 (class 0 only predicted)
    cm = _cm([1, 1, 2, 2, 2, 3], [1, 2, 2, 2, 0, 3], 4)
    assert scores(cm) == {"prec": 4 / 6, "recall": 4 / 6, "acc": 4 / 6}
    want = ("              precision    recall  f1-score   support\n"
            "\n"
            "           o       0.00      0.00      0.00         0\n"
            "           a       1.00      0.50      0.67         2\n"
            "           b       0.67      0.67      0.67         3\n"
            "           c       1.00      1.00      1.00         1\n"
            "\n"
            "    accuracy                           0.67         6\n"
            "   macro avg       0.67      0.54      0.58         6\n"
            "weighted avg       0.83      0.67      0.72         6\n")
    assert classification_report(cm, ["o", "a", "b", "c"]) == want
    assert scores(np.zeros((3, 3), np.int64))["acc"] == 0.0


def test_report_name_mismatch_prints_indices():
    cm = _cm([1, 2, 2], [1, 2, 0], 4)                     # classes 0, 1, 2 occur: 3 of the 4 names
    rep = classification_report(cm, ["other", "a", "b", "c"])
    first, rest = rep.split("\n", 1)
    assert "3 classes" in first and "4 target names" in first
    assert rest == classification_report(cm, None)
    assert "other" not in rest and "\n           0 " in rest


def _sklearn_pairs(rng, t):
    C = int(rng.randint(1, 10))
    n = int(rng.randint(1, 80))
    lab = rng.randint(0, C, n)
    pred = rng.randint(0, C, n)
    if t % 4 == 1:
        pred[:] = rng.randint(0, C)                      # empty columns
    if t % 4 == 2:
        lab[:] = rng.randint(0, C)                       # empty rows (a single labelled class)
    if t % 7 == 3:
        pred = lab.copy()                                # perfect
    return C, lab, pred


def test_report_and_scores_match_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(0)
    for t in range(400):
        C, lab, pred = _sklearn_pairs(rng, t)
        cm = _cm(lab, pred, C)
        present = np.unique(np.concatenate([lab, pred]))
        names = ["cls%d" % c + "_" * (c % 5) for c in present]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for digits in (2, 4):
                want = metrics.classification_report(lab, pred, target_names=names, digits=digits)
                assert classification_report(cm, names, digits=digits) == want, (t, lab, pred)
            assert classification_report(cm) == metrics.classification_report(lab, pred)
            s = scores(cm)
            assert s["acc"] == metrics.accuracy_score(lab, pred)
            assert s["prec"] == metrics.precision_score(lab, pred, average="micro")
            assert s["recall"] == metrics.recall_score(lab, pred, average="micro")


def test_report_name_mismatch_is_an_error_in_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    lab, pred = [1, 2, 2], [1, 2, 0]
    with pytest.raises(ValueError):
        metrics.classification_report(lab, pred, target_names=["other", "a", "b", "c"])
    assert classification_report(_cm(lab, pred, 4), ["other", "a", "b", "c"]).startswith("classification_report: ")


# ---- pack_ids --------------------------------------------------------------------------------------------------------------
def test_pack_ids_round_trip_and_canvas():
    rng = np.random.RandomState(1)
    masks = [rng.randint(0, 60, size=s).astype(np.uint16) for s in ((70, 128), (33, 17), (49, 130))]
    ids, sizes = pack_ids(masks)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (3, 80, 144)
    assert sizes.tolist() == [[70, 128], [33, 17], [49, 130]] and sizes.dtype == torch.int64
    for b, m in enumerate(masks):
        h, w = m.shape
        assert np.array_equal(ids[b, :h, :w].numpy(), m.astype(np.int32))
        assert bool((ids[b, h:] == -1).all()) and bool((ids[b, :, w:] == -1).all())
    # the same canvas rounding as pack
    docs = [{"mask": torch.zeros((1, 2) + m.shape), "label": torch.zeros((1,) + m.shape)} for m in masks]
    x, _, s2 = pack(docs)
    assert tuple(x.shape[-2:]) == tuple(ids.shape[-2:]) and torch.equal(s2, sizes)
    ids7, _ = pack_ids([torch.ones((5, 9), dtype=torch.int64)], round_to=7)
    assert tuple(ids7.shape) == (1, 7, 14)
    with pytest.raises(ValueError):
        pack_ids([])
    with pytest.raises(ValueError):
        pack_ids([np.zeros((3, 3, 2), np.int32)])


# ---- the training script's evaluation ------------------------------------------------------------------------------------
class _Recorder:
    """a stand-in for MSAUWrapper in evaluate(): records the documents each confusion_matrix call sees"""

    def __init__(self, n_class=5):
        self.n_class = n_class
        self.flat_parameters = torch.zeros(1)
        self.seen, self.zero_as = [], set()

    def eval(self):
        return self

    def confusion_matrix(self, inp, labels, sizes=None, zero_as=None, out=None):
        B = int(inp.shape[0])
        if sizes is None:
            assert B == 1
        else:
            assert tuple(sizes.shape) == (B, 2)
        self.seen += [int(inp[b, 0, 0, 0]) for b in range(B)]
        self.zero_as.add(zero_as)
        out[1, 1] += B
        return out


def test_evaluate_selects_the_same_documents_at_any_batch_size():
    import train_chargrid_funsd_msau as T
    docs = []
    for i in range(130):
        h, w = 20 + (i * 7) % 50, 15 + (i * 11) % 40
        x = torch.zeros((1, 3, h, w))
        x[0, 0, 0, 0] = i
        docs.append({"mask": x, "label": torch.zeros((1, h, w), dtype=torch.int64)})
    args = argparse.Namespace(batch_size=8, eval_batch_size=1)
    assert T.eval_count(130, 100) == 101 and T.eval_count(50, 100) == 50 and T.eval_count(7, None) == 7
    for bs in (1, 4, 16):
        r = _Recorder()
        res = T.evaluate(docs, r, args, name="Train", max_num_examples=100, batch_size=bs)
        assert sorted(r.seen) == list(range(101)), bs
        assert res == {"prec": 1.0, "recall": 1.0, "acc": 1.0} and r.zero_as == {None}
        r = _Recorder()
        T.evaluate(docs[:20], r, args, name="Test", testing=True, labels_map={"a": 0, "other": 3}, batch_size=bs)
        assert sorted(r.seen) == list(range(20)) and r.zero_as == {3}
    r = _Recorder()
    T.evaluate(docs[:9], r, argparse.Namespace(batch_size=1, eval_batch_size=4), name="Validation")
    assert sorted(r.seen) == list(range(9))
    assert T.canvases(docs[:3], 1) == {(1, 20, 15), (1, 27, 26), (1, 34, 37)}
    assert T.canvases(docs[:3], 4) == {(3, 48, 48)}


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_ragged_inference_refusals_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = MSAUWrapper(13, 5, dict(KW))
    ids = torch.zeros((2, 32, 48), dtype=torch.int32)
    x = torch.zeros((2, 13, 32, 48))
    lab = torch.zeros((2, 32, 48), dtype=torch.int64)
    good = torch.tensor([[32, 40], [10, 48]])
    for bad in (torch.tensor([[33, 40], [10, 48]]), torch.tensor([[32, 40]]), torch.tensor([[0, 4], [1, 1]]),
                torch.tensor([[3.0, 4.0], [1.0, 1.0]])):
        with pytest.raises(ValueError):
            m.predict_nhwc(ids=ids, sizes=bad)
        with pytest.raises(ValueError):
            m.confusion_matrix(x, lab, sizes=bad)
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        m.confusion_matrix(x, torch.full((2, 32, 48), 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        m.confusion_matrix(x, torch.full((2, 32, 48), -1, dtype=torch.int64), sizes=good)
    with pytest.raises(ValueError):
        m.confusion_matrix(x, lab, zero_as=5)
    with pytest.raises(ValueError, match="64"):
        MSAUWrapper(13, 65, dict(KW)).confusion_matrix(x, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_nhwc(ids=ids, sizes=good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_nhwc(inp=x, sizes=good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.confusion_matrix(x, lab, sizes=good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.confusion_matrix(x, lab)


# ---- the training script's command line --------------------------------------------------------------------------------------
def test_training_script_command_line():
    import train_chargrid_funsd_msau as T
    a = T.parse_args([])
    assert (a.batch_size, a.eval_batch_size, a.num_epochs, a.loop, a.dtype) == (1, 1, 300, "engine", "bf16")
    assert (a.bmname, a.hidden_dim, a.dataset, a.method) == (None, 500, "invoice", "GCN")
    a = T.parse_args(["--batch-size", "4", "--eval-batch-size", "16", "--loop", "reference", "--num-epochs", "2"])
    assert (a.batch_size, a.eval_batch_size, a.loop, a.num_epochs) == (4, 16, "reference", 2)
    assert (a.bmname, a.hidden_dim, a.dataset, a.method) == (None, 500, "invoice", "GCN")
    for bad in (["--batch-size", "0"], ["--eval-batch-size", "-2"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_training_script_main_refuses_without_gpu(tmp_path, monkeypatch):
    """main() gets past its argument setup and the data loading to the model (which needs the GPU) -- on a GPU host this is
    tests/test_ragged_infer_gpu.py::test_training_script_main_end_to_end"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import os
    import pickle
    import train_chargrid_funsd_msau as T
    from msau_amd.data.funsd import get_preprocessed_list_word_msau
    from tests.golden_util import GOLDEN
    monkeypatch.chdir(tmp_path)
    inv = None
    for split in ("train", "test"):                           # the test split takes the training split's charset
        docs, inv = get_preprocessed_list_word_msau(os.path.join(GOLDEN, "funsd", split), inv)
        with open(f"{split}.pkl", "wb") as fh:
            pickle.dump(docs, fh)
    with pytest.raises((RuntimeError, AssertionError)):          # torch: no GPU to move the model to
        T.main(["--train-pickle", "train.pkl", "--test-pickle", "test.pkl", "--num-epochs", "1", "--batch-size", "2"])
    assert os.path.exists("model_kwargs.json")
