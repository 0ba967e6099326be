"""The reference's epoch loop (model/training/trainer.py:56-126) for the key-value model on the device path: training steps from
table groups (`TrainEngine.step_kv`), then every validation document forward-only (`MSAUWrapper.eval_kv`), the TRAIN / VAL lines of
msau_amd/training/trainer.py, lr = 1e-3 * 0.95^(epoch // 10), a checkpoint `<output_path>/model<epoch>` whenever the validation
loss improves or every 8th epoch.  Per document rows (loss and accuracy counts, msau_unet_eval) are collected on the device and
read twice per epoch: once after the training steps, once after the validation."""
from __future__ import annotations

import os
import time
from typing import List

import torch


def summarize(doc_loss: torch.Tensor, doc_counts: torch.Tensor) -> dict:
    """Rows of `MSAUWrapper.eval_unet` (fp32 [N, 2], int32 [N, 2, 2]; any number of groups concatenated) -> the reference's epoch
    figures, which are means over documents because the reference runs batch 1: `loss` = mean of 0.5 final + 0.5 aux (of final
    alone when the model has no auxiliary head, i.e. every auxiliary row is zero), `final`, `aux`, `acc` = mean over the documents
    WITH labelled pixels of correct / labelled on the final head, `documents`, `unlabelled` = documents without a labelled pixel
    (the reference's accuracy is NaN for them; here they are left out of `acc` and counted).  One host read."""
    n = int(doc_loss.shape[0])
    both = torch.cat([doc_loss.detach().double().reshape(n, 2), doc_counts.detach().double().reshape(n, 4)], dim=1).cpu()
    loss, counts = both[:, :2], both[:, 2:].reshape(n, 2, 2)
    has_aux = bool((loss[:, 1] != 0).any() or (counts[:, 1] != 0).any())
    final, aux = loss[:, 0], loss[:, 1]
    total = 0.5 * final + 0.5 * aux if has_aux else final
    labelled, correct = counts[:, 0, 0], counts[:, 0, 1]
    seen = labelled > 0
    mean = lambda v: float(v.mean()) if n else float("nan")
    return {"loss": mean(total), "final": mean(final), "aux": mean(aux) if has_aux else 0.0,
            "acc": float((correct[seen] / labelled[seen]).mean()) if bool(seen.any()) else float("nan"),
            "documents": n, "unlabelled": int((~seen).sum())}


class _Rows:
    """per-document rows of an epoch phase, kept on the device until `read`"""

    def __init__(self):
        self.loss: List[torch.Tensor] = []
        self.counts: List[torch.Tensor] = []

    def add(self, pair):
        self.loss.append(pair[0])
        self.counts.append(pair[1])

    def read(self) -> dict:
        if not self.loss:
            return summarize(torch.zeros((0, 2)), torch.zeros((0, 2, 2), dtype=torch.int32))
        return summarize(torch.cat(self.loss), torch.cat(self.counts))


class KVTrainer:
    """`KVTrainer(model, batches).fit(output_path, epochs, steps_per_epoch)`: `model` a MSAUWrapper on the GPU, `batches` a
    KVTrainBatches (its iterator gives the training groups, its `validation()` the validation groups), `class_weights` as
    `TrainEngine.step_unet` takes them, `engine_kwargs` for the TrainEngine.  `opt_kwargs` (a dict, `{}` included): the options of
    the reference's `get_optimizer`; the engine is then `TrainEngine.from_opt_kwargs(model, opt_kwargs, **engine_kwargs)`, the
    reference `Trainer`'s optimiser -- RMSprop at 1e-3 by default, no gradient clipping.  None: the engine's own default (clip +
    Adam).  `cost_kwargs`: the `cost` of `TrainEngine.step_unet` ({"cost_name": "focal", "gamma": 2.0}, {"cost_name": "dice",
    "smooth": 1.0}; None: the cross entropy), checked here and given to every training step AND every validation call: the
    TRAIN / VAL lines and the checkpoint rule run on the loss that is trained.  Eager only; under data parallelism every rank
    would validate every document."""

    def __init__(self, model, batches, class_weights=None, engine_kwargs={}, opt_kwargs=None, cost_kwargs=None):
        from ..plan import unet_cost
        self.model, self.batches, self.class_weights = model, batches, class_weights
        self.cost = unet_cost(cost_kwargs)
        self._cost_kw = {} if self.cost is None else {"cost": self.cost}      # the cross entropy: the calls as they always were
        self.engine = self._engine(dict(engine_kwargs)) if opt_kwargs is None else self._engine_from_opt(dict(opt_kwargs), dict(engine_kwargs))

    def _engine(self, kwargs):
        from ..model import TrainEngine
        return TrainEngine(self.model, **kwargs)

    def _engine_from_opt(self, opt_kwargs, kwargs):
        from ..model import TrainEngine
        return TrainEngine.from_opt_kwargs(self.model, opt_kwargs, **kwargs)

    def _stats(self, n: int):
        dev = self.model.flat_parameters.device
        return (torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty((n, 2, 2), dtype=torch.int32, device=dev))

    def validate(self) -> dict:
        """every group of `batches.validation()` through `eval_kv`; one read"""
        rows = _Rows()
        for group in self.batches.validation():
            rows.add(self.model.eval_kv(group, class_weights=self.class_weights, **self._cost_kw))
        return rows.read()

    def fit(self, output_path, epochs: int, steps_per_epoch: int, restore_path=None) -> List[dict]:
        """-> per epoch {"epoch", "lr", "train": summarize(...), "val": summarize(...), "saved": path or None}"""
        print("Epochs: " + str(epochs))
        print("Batch Size Train: " + str(self.batches.batch_size))
        print("Batchsteps per Epoch: " + str(steps_per_epoch))
        history: List[dict] = []
        if epochs == 0:
            return history
        save_path = None
        if output_path is not None:
            os.makedirs(os.path.abspath(output_path), exist_ok=True)
            save_path = os.path.join(output_path, "model")
        if restore_path is not None:
            print("Loading Checkpoint.")
            self.model.load_weights(restore_path)
        best, shown = 100000.0, 0
        for epoch in range(epochs):
            lr = 0.001 * (0.95 ** (epoch // 10))
            self.engine.lr = lr                          # a by-value argument of every optimiser launch (eager steps only)
            t0 = time.time()
            rows = _Rows()
            for _ in range(steps_per_epoch):
                group = next(self.batches)
                stats = self._stats(len(group))
                self.engine.step_kv(group, class_weights=self.class_weights, stats=stats, **self._cost_kw)
                rows.add(stats)
                shown += len(group)
            train = rows.read()
            print("TRAIN: Epoch {:}, Acc: {:.6f}, Average loss: {:.6f} final: {:.6f}, training samples shown: {:}, "
                  "learning rate: {:.6f}, time used: {:.2f}".format(epoch + 1, train["acc"], train["loss"], train["final"], shown, lr,
                                                                    time.time() - t0))
            t0 = time.time()
            val = self.validate()
            print("VAL: Epoch {:}, Acc: {:.6f}, Average loss: {:.6f} final: {:.6f}, time used: {:.2f}".format(
                epoch + 1, val["acc"], val["loss"], val["final"], time.time() - t0))
            saved = None
            if save_path is not None and (val["loss"] < best or (epoch + 1) % 8 == 0):
                best = min(best, val["loss"])
                print("Saving checkpoint")
                saved = save_path + str(epoch + 1)
                self.model.save(saved)
            history.append({"epoch": epoch + 1, "lr": lr, "train": train, "val": val, "saved": saved})
        print("Optimization Finished!")
        print("Best Val Loss: " + str(best))
        return history
