"""Key-value validation on the CPU: the C ABI of msau_unet_eval, the host statement `unet_eval_host` (tests/kv_eval_util.py) against
the values the reference's own UNetLoss produced (tests/golden/train/unet_loss*.npz: acc, loss, final -- the values
msau_amd/training/cost.py::UNetLoss is pinned to on the GPU), `summarize` on hand-made rows, and `KVTrainer.fit` against a stub model
and engine: the learning rates, which epochs save, the printed lines, the history."""
import os
import re

import numpy as np
import pytest
import torch

from tests import kv_eval_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- 1: the C ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_eval_symbols_and_version_stays():
    from msau_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name, proto in (("msau_unet_eval", "int msau_unet_eval("), ("msau_unet_eval_ws_bytes", "int64_t msau_unet_eval_ws_bytes(")):
        assert name in L.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
        assert proto in header, name
    # the prototype's parameters, one ctypes entry each, pointers as pointers
    proto = re.search(r"int msau_unet_eval\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in proto.replace("\n", " ").split(",")]
    res, args = L._SIGNATURES["msau_unet_eval"]
    assert len(params) == len(args) == 17
    for p, a in zip(params, args):
        assert ("*" in p) == (a is L.vp), (p, a)
    assert L._SIGNATURES["msau_unet_eval_ws_bytes"] == (L.i64, [L.C.c_int, L.C.c_int])
    assert lib.msau_version() == 11
    # the argument checks come before any launch: K, B and the stored channel count
    for K, B, Cs in ((0, 1, 8), (257, 1, 8), (1, 1025, 8), (1, 1, 12)):
        assert lib.msau_unet_eval(None, L.F32, 1, None, 1, None, None, None, K, 1, 1, 1, B, 1, 1, 5, Cs) != 0
        assert "unet_eval" in lib.msau_last_error().decode()
    one = lib.msau_unet_eval_ws_bytes(1, 1)
    assert one >= 32 and lib.msau_unet_eval_ws_bytes(3, 7) == 21 * one and lib.msau_unet_eval_ws_bytes(0, 4) == 0


# ---- 2: the host statement against the reference's values -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unet_loss.npz", "unet_loss_weighted.npz"])
def test_host_statement_equals_the_reference(name):
    """the fixture's batch is ONE document for the reference's loss (a mean over all its pixels): its samples stacked"""
    g = np.load(os.path.join(GOLDEN, "train", name))
    seen_aux = set()
    for tag in ("a", "b", "c"):
        lg = g[f"{tag}.logits"]                                                # [B, C, H, W]
        B, C, H, W = lg.shape
        doc = lambda x: np.transpose(x, (0, 2, 3, 1)).reshape(1, B * H, W, C)
        lab = g[f"{tag}.label"].reshape(1, B * H, W)
        with_aux = f"{tag}.aux" in g.files
        seen_aux.add(with_aux)
        cw = [float(v) for v in g[f"{tag}.class_weights"]] if f"{tag}.class_weights" in g.files else None
        loss, counts, _near = E.unet_eval_host(doc(lg), doc(g[f"{tag}.aux"]) if with_aux else None, lab, lab if with_aux else None, None, cw)
        acc, total, final = E.summary_host(loss, counts, has_aux=with_aux)
        assert counts[0, 0, 0] > 0 and abs(acc - float(g[f"{tag}.acc"])) < 1e-6, (tag, acc)
        assert abs(total - float(g[f"{tag}.loss"])) < 1e-5 * abs(float(g[f"{tag}.loss"])), (tag, total)
        if with_aux:
            assert abs(final - float(g[f"{tag}.final"])) < 1e-5 * abs(float(g[f"{tag}.final"])), (tag, final)
        else:
            assert (loss[:, 1] == 0).all() and (counts[:, 1] == 0).all()
    assert seen_aux == {True, False}


def test_host_statement_rules():
    """extents, labels outside [0, C), a zero weight, the first maximum, a document without weight"""
    C = 3
    lg = np.zeros((2, 2, 3, 8))
    lg[0, 0, 0, :C] = (1.0, 1.0, 0.0)                                          # a tie: class 0 predicted, label 1 -> wrong
    lg[0, 0, 1, :C] = (0.0, 2.0, 2.0)                                          # a tie: class 1 predicted, label 1 -> right
    lg[0, 1, :, :] = 1e9                                                       # outside the extent
    lg[0, :, :, C:] = 50.0                                                     # padded channels are not classes
    lab = np.array([[[1, 1, -1], [2, 2, 2]], [[2, 2, 5], [0, 0, 0]]])
    loss, counts, near = E.unet_eval_host(lg, None, lab, None, [(1, 3), (2, 3)], [1.0, 1.0, 0.0])
    assert counts[0, 0].tolist() == [2, 1] and near[0, 0] == 2
    want = 0.5 * ((np.log(2 * np.e + 1) - 1.0) + (np.log(2 * np.exp(2.0) + 1) - 2.0))
    assert abs(loss[0, 0] - want) < 1e-12
    assert counts[1, 0].tolist() == [2, 0]                                     # label 5 is no class; the zero-weight pixels still count
    assert abs(loss[1, 0] - np.log(3.0)) < 1e-12                               # only the three label-0 pixels carry weight
    loss, counts, _ = E.unet_eval_host(lg, None, lab, None, [(1, 3), (1, 2)], [1.0, 1.0, 0.0])
    assert loss[1, 0] == 0.0 and counts[1, 0].tolist() == [2, 0]               # D_b = 0
    assert (loss[:, 1] == 0).all() and (counts[:, 1] == 0).all()


# ---- 3: summarize -------------------------------------------------------------------------------------------------------------------
def test_summarize_on_hand_made_rows():
    from msau_amd.training.kv_trainer import summarize
    loss = torch.tensor([[1.0, 3.0], [2.0, 2.0], [0.5, 0.25]])
    counts = torch.tensor([[[10, 5], [4, 4]], [[0, 0], [7, 1]], [[4, 3], [0, 0]]], dtype=torch.int32)
    s = summarize(loss, counts)
    assert s["documents"] == 3 and s["unlabelled"] == 1
    assert s["acc"] == pytest.approx((0.5 + 0.75) / 2) and s["final"] == pytest.approx(3.5 / 3) and s["aux"] == pytest.approx(5.25 / 3)
    assert s["loss"] == pytest.approx(0.5 * 3.5 / 3 + 0.5 * 5.25 / 3)
    # no auxiliary head: its rows are zeros, the loss is the final head's
    s = summarize(torch.tensor([[1.0, 0.0], [2.0, 0.0]]), torch.tensor([[[2, 1], [0, 0]], [[2, 2], [0, 0]]], dtype=torch.int32))
    assert s["loss"] == pytest.approx(1.5) and s["final"] == pytest.approx(1.5) and s["aux"] == 0.0 and s["acc"] == pytest.approx(0.75)
    # nothing labelled anywhere: the accuracy is NaN and says so in `unlabelled`
    s = summarize(torch.tensor([[1.0, 1.0]]), torch.zeros((1, 2, 2), dtype=torch.int32))
    assert np.isnan(s["acc"]) and s["unlabelled"] == 1 and s["loss"] == pytest.approx(1.0)
    from msau_amd import training
    assert training.summarize is summarize and training.KVTrainer is not None


# ---- 4: the epoch loop against a stub ------------------------------------------------------------------------------------------------
class _StubBatches:
    batch_size = 2

    def __next__(self):
        return ["t0", "t1"]

    def validation(self):
        return [["v0", "v1"], ["v2"]]


class _StubModel:
    """validation losses per epoch from a script; every document of an epoch has that loss"""

    def __init__(self, script):
        self.script, self.epoch, self.saved, self.loaded = script, 0, [], []
        self.flat_parameters = torch.zeros(1)

    def eval_kv(self, tables, class_weights=None):
        v = self.script[self.epoch]
        rows = torch.tensor([[v, v]] * len(tables)), torch.tensor([[[4, 2], [4, 1]]] * len(tables), dtype=torch.int32)
        if tables[-1] == "v2":
            self.epoch += 1
        return rows

    def save(self, path):
        self.saved.append(os.path.basename(path))

    def load_weights(self, path):
        self.loaded.append(path)


class _StubEngine:
    def __init__(self):
        self.lr, self.lrs = None, []

    def step_kv(self, tables, class_weights=None, stats=None):
        self.lrs.append(self.lr)
        stats[0].copy_(torch.tensor([[0.5, 1.5]] * len(tables)))
        stats[1].copy_(torch.tensor([[[8, 6], [8, 2]]] * len(tables), dtype=torch.int32))


def test_fit_schedule_saves_lines_and_history(tmp_path, capsys):
    from msau_amd.training.kv_trainer import KVTrainer

    class Stubbed(KVTrainer):
        def _engine(self, kwargs):
            assert kwargs == {"max_norm": 2.0}
            return _StubEngine()

    epochs = 21
    script = [5.0, 4.0, 4.5, 4.5, 3.0, 3.5, 3.5, 3.5, 3.5, 3.5, 2.0] + [2.5] * 10
    model = _StubModel(script)
    tr = Stubbed(model, _StubBatches(), engine_kwargs={"max_norm": 2.0})
    hist = tr.fit(str(tmp_path / "out"), epochs, 3, restore_path="ckpt")
    out = capsys.readouterr().out
    assert model.loaded == ["ckpt"] and os.path.isdir(str(tmp_path / "out"))
    # learning rates: one per step, 1e-3 * 0.95^(epoch // 10)
    lrs = tr.engine.lrs
    assert len(lrs) == 3 * epochs
    for epoch, want in ((0, 1e-3), (9, 1e-3), (10, 0.95e-3), (20, 0.9025e-3)):
        assert lrs[3 * epoch] == pytest.approx(want, rel=1e-12) and hist[epoch]["lr"] == lrs[3 * epoch], epoch
    # saves: improvements (epochs 1, 2, 5, 11) and every 8th (8, 16)
    assert model.saved == ["model1", "model2", "model5", "model8", "model11", "model16"]
    assert [h["epoch"] for h in hist if h["saved"]] == [1, 2, 5, 8, 11, 16]
    assert out.count("Saving checkpoint") == 6 and "Best Val Loss: 2.0" in out
    # the printed lines
    tl = re.findall(r"^TRAIN: Epoch (\d+), Acc: ([\d.]+), Average loss: ([\d.]+) final: ([\d.]+), training samples shown: (\d+), "
                    r"learning rate: ([\d.]+), time used: ([\d.]+)$", out, re.M)
    vl = re.findall(r"^VAL: Epoch (\d+), Acc: ([\d.]+), Average loss: ([\d.]+) final: ([\d.]+), time used: ([\d.]+)$", out, re.M)
    assert len(tl) == len(vl) == epochs
    assert [int(t[0]) for t in tl] == list(range(1, epochs + 1)) and [int(t[4]) for t in tl] == [6 * (e + 1) for e in range(epochs)]
    assert all((float(t[1]), float(t[2]), float(t[3])) == (0.75, 1.0, 0.5) for t in tl)
    assert [float(v[2]) for v in vl] == script and all(float(v[1]) == 0.5 for v in vl)
    # the history
    assert len(hist) == epochs
    for h, v in zip(hist, script):
        assert h["val"]["loss"] == v and h["val"]["final"] == v and h["val"]["documents"] == 3 and h["val"]["acc"] == 0.5
        assert h["train"]["loss"] == 1.0 and h["train"]["final"] == 0.5 and h["train"]["documents"] == 6 and h["train"]["acc"] == 0.75
    assert Stubbed(model, _StubBatches(), engine_kwargs={"max_norm": 2.0}).fit(None, 0, 3) == []
