"""`UNetLoss` counterpart (reference: model/training/cost.py:6-65): plain cross entropy over every pixel on
one-hot targets, 0.5 * final + 0.5 * auxiliary when auxiliary logits are given, accuracy over pixels whose
target class is not 0.  The CE and its gradient are one HIP kernel (`msau_softmax_ce`).  Beyond the reference, which promises
a Dice cost and returns the prediction for it: `cost_name` "focal" (`gamma`, default 2) and "dice" (`smooth`, default 1) are the
focal and the soft Dice loss of DESIGN.md 5e, each sample of the batch a document of its own (`msau_unet_cost`)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from ..plan import unet_cost
from ..plan_loss import NCHW_HIST_K, nchw_loss


class _SoftmaxCE(torch.autograd.Function):
    """mean over all B*H*W pixels of -log softmax(logits)[target] on NCHW fp32 logits"""

    @staticmethod
    def forward(ctx, logits, target):
        loss = torch.zeros((1,), dtype=torch.float32, device=logits.device)

        def kernel(nhwc, dn, label, hist, B, H, W, C, Cs, s):
            ws = torch.zeros((int(L.load().msau_ce_ws_floats(B * H * W)),), dtype=torch.float32, device=logits.device)
            L.call("msau_softmax_ce", s, L.F32, nhwc[0], label, dn[0], loss.data_ptr(), ws.data_ptr(), B, H * W, C, Cs, 1.0 / (B * H * W))

        ctx.save_for_backward(*nchw_loss((logits,), target, kernel))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        return g * go, None


class _WeightedSoftmaxCE(torch.autograd.Function):
    """torch.nn.CrossEntropyLoss(weight) on NCHW fp32 logits (model/training/cost.py:24-31): sum_p w[t_p] nll_p / sum_p w[t_p].
    One pass writes the un-normalised gradient and both sums (`msau_softmax_ce_weighted`); the denominator, known only after
    it, is applied where autograd multiplies by the incoming gradient anyway."""

    @staticmethod
    def forward(ctx, logits, target, class_w):
        sums = torch.zeros((2,), dtype=torch.float32, device=logits.device)

        def kernel(nhwc, dn, label, hist, B, H, W, C, Cs, s):
            ws = torch.zeros((int(L.load().msau_ce_ws_floats(B * H * W)),), dtype=torch.float32, device=logits.device)
            L.call("msau_softmax_ce_weighted", s, L.F32, nhwc[0], label, class_w.data_ptr(), dn[0], sums.data_ptr(), ws.data_ptr(),
                   B, H * W, C, Cs)

        ctx.save_for_backward(*nchw_loss((logits,), target, kernel), sums)
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, go):
        g, sums = ctx.saved_tensors
        return g * (go / sums[1]), None, None


class _UnetCost(torch.autograd.Function):
    """the focal or the soft Dice loss of one head on NCHW fp32 logits (`msau_unet_cost`): every sample is its own document, the
    loss is the mean of the samples' losses; `cost` a checked msau_amd.plan.UnetCost, `class_w` fp32 [C] on the device or None"""

    @staticmethod
    def forward(ctx, logits, target, cost, class_w):
        loss3 = torch.empty((3,), dtype=torch.float32, device=logits.device)

        def kernel(nhwc, dn, label, hist, B, H, W, C, Cs, s):
            ws = torch.empty((int(L.load().msau_unet_cost_ws_floats(cost.kind, B, H, W, C)),), dtype=torch.float32, device=logits.device)
            L.call("msau_unet_cost", s, L.F32, cost.kind, cost.param, nhwc[0], None, label, None, None,
                   class_w.data_ptr() if class_w is not None else None, hist, NCHW_HIST_K, dn[0], None, loss3.data_ptr(), ws.data_ptr(),
                   B, H, W, C, Cs)

        ctx.save_for_backward(*nchw_loss((logits,), target, kernel, hist=class_w is not None or cost.kind == L.COST_DICE))
        return loss3[0].clone()

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        return g * go, None, None, None


class UNetLoss(torch.nn.Module):
    def __init__(self, kwargs):
        super().__init__()
        self.cost_name = kwargs.get("cost_name", "cross_entropy")
        self.act_name = kwargs.get("act_name", "softmax")
        self.class_weights = kwargs.get("class_weights", None)
        self.cost = unet_cost(kwargs) if self.cost_name in ("focal", "dice") else None
        if self.class_weights is not None and self.cost_name in ("cross_entropy", "focal", "dice"):
            # the reference keeps them as a CPU tensor inside torch.nn.CrossEntropyLoss (cost.py:26-29); here a buffer that
            # follows the module to the device
            self.register_buffer("class_weights_torch", torch.from_numpy(np.array(self.class_weights, dtype=np.float32)))

    def _ce(self, logits, tgt_idx):
        """the head's loss under `cost_name` (the cross entropy, or `_UnetCost`)"""
        cw = None
        if self.class_weights is not None:
            cw = self.class_weights_torch.to(logits.device).contiguous()
            assert cw.numel() == logits.shape[1], "class_weights: one weight per class"
        if self.cost is not None:
            return _UnetCost.apply(logits, tgt_idx, self.cost, cw)
        if cw is None:
            return _SoftmaxCE.apply(logits, tgt_idx)
        return _WeightedSoftmaxCE.apply(logits, tgt_idx, cw)

    def forward(self, logits, tgt, kwargs):
        """-> (acc, loss, final_loss) exactly as the reference; `tgt` / `aux_tgt` are one-hot [B,C,H,W]"""
        aux_logits = kwargs.get("aux_logits", None)
        aux_tgt = kwargs.get("aux_tgt", None)
        if self.cost_name not in ("cross_entropy", "focal", "dice"):
            return torch.softmax(logits, dim=1) if self.act_name == "softmax" else logits
        tgt = torch.argmax(tgt, dim=1)
        with torch.no_grad():
            pred = torch.argmax(logits, dim=1)
            nz = tgt != 0
            acc = float((pred[nz] == tgt[nz]).sum()) / max(int(nz.sum()), 1) if bool(nz.any()) else float("nan")
        loss_map = self._ce(logits, tgt)
        if aux_logits is not None:
            aux = self._ce(aux_logits, torch.argmax(aux_tgt, dim=1))
            return acc, 0.5 * loss_map + 0.5 * aux, loss_map
        return acc, loss_map, None
