"""Drop-in counterpart of the reference's model API (model/model.py:399-459 `MSAUWrapper`).

Same constructor, `forward -> (pred, logits, aux_logits)`, `loss`, `save`, `load_weights`, the same
`state_dict` keys / shapes (fp32, OIHW / IOHW), but the network itself runs as a static plan of
hand-written HIP kernels (msau_amd/plan.py, msau_amd/csrc/*).  There is no PyTorch-op fallback: on a
machine without the HIP library or without a GPU the compute entry points raise.

Two ways to train:
  * reference style -- `model(x)`, `model.loss(...)`, `loss.backward()`, `clip_grad_norm_`, `Adam.step()`
    (train_chargrid_funsd_msau.py:46-59): the whole net is ONE autograd node;
  * `TrainEngine.step(x, labels)` -- the same kernels plus fused masked-CE, RCCL gradient
    all-reduce and a fused clip+Adam over the flat parameter buffer, optionally replayed as a HIP graph.
"""
from __future__ import annotations

import os
import weakref

import math

import numpy as np
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from .plan import Plan, unet_cost
from .plan_loss import NCHW_HIST_K, nchw_loss

DTYPES = {"fp32": L.F32, "float32": L.F32, "bf16": L.BF16, "bfloat16": L.BF16}


def param_shapes(cfg: dict) -> "OrderedDict[str, Tuple[int, ...]]":
    """state_dict key -> shape in the reference's registration order
    (model/model.py:98-127 encoder, :197-222 decoder, :356-376 stages and end convs)."""
    S, R, Fr = cfg["scale_space_num"], cfg["res_depth"], cfg["featRoot"]
    k, nb = cfg["filter_size"], cfg.get("num_blocks", 3)
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(prefix, co, ci, kk):
        out[prefix + ".weight"] = (co, ci, kk, kk)
        out[prefix + ".bias"] = (co,)

    if cfg.get("variant") == "box":
        # model/model_box.py: the residual 3x3 blocks are MultiBoxConvBlocks (:9-59): num_box_convs x [BoxConv2d with four
        # [c, F] parameters x_min / x_max / y_min / y_max, then a 1x1 conv F*c -> c]; everything else as the plain net
        n, Fn = cfg["num_box_convs"], cfg["num_box_per_channels"]

        def block(prefix, c):
            for i in range(n):
                for nm in ("x_min", "x_max", "y_min", "y_max"):
                    out[f"{prefix}.conv_list.{2 * i}.{nm}"] = (c, Fn)
                conv(f"{prefix}.conv_list.{2 * i + 1}.custom_conv", c, Fn * c, 1)

        for b in range(nb):
            cin = cfg["channels"] if b == 0 else cfg["n_class"]
            pd = f"msau_net.blocks.{b}.downsamplingblock"
            pu = f"msau_net.blocks.{b}.upsamplingblock"
            for l in range(S):
                block(f"{pd}.conv_box_list.{l}", Fr * 2 ** l)
            last = cin
            for l in range(S):
                conv(f"{pd}.conv1s.{l}.conv", Fr * 2 ** l, last, k)
                last = Fr * 2 ** l
            if b > 0:
                for l in range(S):
                    conv(f"{pd}.conv1_1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, 1)
            Cb = Fr * 2 ** (S - 1)
            for nm, co in (("f", Cb // 8), ("g", Cb // 8), ("h", Cb)):
                conv(f"{pd}.layer_attentions.attention_block.{nm}.conv", co, Cb, 1)
            for l in range(S - 1):
                conv(f"{pu}.conv1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, k)
            if b > 0:
                for l in range(S - 1):
                    conv(f"{pu}.conv1_1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, 1)
            for l in range(S - 1):
                c = Fr * 2 ** l
                out[f"{pu}.deconvs.{l}.conv.weight"] = (2 * c, c, k, k)
                out[f"{pu}.deconvs.{l}.conv.bias"] = (c,)
            for l in range(S - 1):
                block(f"{pu}.conv_box_list.{l}", Fr * 2 ** l)
        for b in range(nb):
            conv(f"msau_net.end_convs.{b}.custom_conv", cfg["n_class"], Fr, 4)
        return out

    for b in range(nb):
        cin = cfg["channels"] if b == 0 else cfg["n_class"]
        pd = f"msau_net.blocks.{b}.downsamplingblock"
        pu = f"msau_net.blocks.{b}.upsamplingblock"
        for l in range(S):
            for r in range(R):
                conv(f"{pd}.conv_res_list.{l}.conv_res_list.{r}.custom_conv", Fr * 2 ** l, Fr * 2 ** l, k)
        last = cin
        for l in range(S):
            conv(f"{pd}.conv1s.{l}.conv", Fr * 2 ** l, last, k)
            last = Fr * 2 ** l
        if b > 0:
            for l in range(S):
                conv(f"{pd}.conv1_1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, 1)
        Cb = Fr * 2 ** (S - 1)
        for nm, co in (("f", Cb // 8), ("g", Cb // 8), ("h", Cb)):
            conv(f"{pd}.layer_attentions.attention_block.{nm}.conv", co, Cb, 1)
        for l in range(S - 1):
            for r in range(R):
                conv(f"{pu}.conv_res_list.{l}.conv_res_list.{r}.custom_conv", Fr * 2 ** l, Fr * 2 ** l, k)
        for l in range(S - 1):
            conv(f"{pu}.conv1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, k)
        if b > 0:
            for l in range(S - 1):
                conv(f"{pu}.conv1_1s.{l}.custom_conv", Fr * 2 ** l, 2 * Fr * 2 ** l, 1)
        for l in range(S - 1):
            c = Fr * 2 ** l
            out[f"{pu}.deconvs.{l}.conv.weight"] = (2 * c, c, k, k)        # ConvTranspose2d: [in, out, k, k]
            out[f"{pu}.deconvs.{l}.conv.bias"] = (c,)
    for b in range(nb):
        conv(f"msau_net.end_convs.{b}.custom_conv", cfg["n_class"], Fr, 4)
    return out


def _init_param(key: str, shape, gen: Optional[torch.Generator], fan_in: int = 0) -> torch.Tensor:
    """Reference initialisation statistics: W ~ N(0, sqrt(2/(kh*kw*K2+K3))), b ~ N(0.1, 1e-5)
    (layers.py:33-36,59-60,111-114,130-131,216,227-228); attention 1x1 convs keep torch's Conv2d
    default (attention.py:19-21)."""
    if ".attention_block." in key:
        # kaiming_uniform(a=sqrt(5)) weights and U(-1/sqrt(fan_in), +) biases share the same bound
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=gen) * 2 - 1) * bound
    if len(shape) == 1:
        return 0.1 + 1e-5 * torch.randn(shape, generator=gen)
    std = math.sqrt(2.0 / (shape[2] * shape[3] * shape[1] + shape[0]))
    return std * torch.randn(shape, generator=gen)


class _Node(nn.Module):
    """Name-only container used to reproduce the reference's module tree (and thereby its state_dict keys)."""


class _MSAUFunction(torch.autograd.Function):
    """The whole network as one autograd node: forward / backward are the plan's kernel sequences."""

    @staticmethod
    def forward(ctx, wrapper, x, sizes, *params):
        plan = wrapper._plan_for(x, training=True, ragged=sizes is not None)
        plan.set_extents(sizes)
        # The saved activations are the plan's own buffers: a second grad-mode forward of the same shape overwrites them.
        # backward() checks that it still belongs to the latest forward instead of returning silently wrong gradients.
        plan.generation += 1
        logits, aux = plan.forward(wrapper._flat, x)
        ctx.wrapper, ctx.plan, ctx.generation = wrapper, plan, plan.generation
        outs = (logits.clone(), aux.clone() if aux is not None else None)
        ctx.has_aux = aux is not None
        return outs if aux is not None else (outs[0],)

    @staticmethod
    def backward(ctx, *gouts):
        w, plan = ctx.wrapper, ctx.plan
        if plan.generation != ctx.generation:
            raise RuntimeError("MSAUWrapper: backward() of a forward whose saved activations were overwritten by a later "
                               f"forward of the same input shape {(plan.B, plan.H, plan.W)} (gradient accumulation over "
                               "micro-batches: call backward() before the next forward, or use TrainEngine)")
        g_logits = gouts[0]
        g_aux = gouts[1] if ctx.has_aux else None
        plan.set_external_grads(g_logits, g_aux)
        flat_g = torch.zeros_like(w._flat)               # fresh buffer: no aliasing between backward calls
        plan.backward(flat_g)
        grads = []
        for key, p in w._named:
            off, n = w._poff[key], p.numel()
            grads.append(flat_g[off:off + n].view(p.shape) if key not in w._dead else None)
        return (None, None, None, *grads)


class _MaskedCEFunction(torch.autograd.Function):
    """MSAUWrapper.loss (model/model.py:446-459) on NCHW fp32 logits, batch rule of SURVEY 8(e)."""

    @staticmethod
    def forward(ctx, logits, aux, label):
        B, C, H, W = logits.shape
        dev = logits.device
        s = torch.cuda.current_stream().cuda_stream
        label = label.reshape(B, H, W).contiguous().long()
        counts = torch.zeros((B,), dtype=torch.int32, device=dev)
        L.call("msau_label_counts", s, label.data_ptr(), counts.data_ptr(), B, H * W)
        loss = torch.zeros((1,), dtype=torch.float32, device=dev)
        ws = torch.zeros((int(L.load().msau_ce_ws_floats(B * H * W)),), dtype=torch.float32, device=dev)

        def kernel(nhwc, dn, label, hist, B, H, W, C, Cs, s):
            L.call("msau_masked_ce", s, L.F32, nhwc[0], label, counts.data_ptr(), dn[0], loss.data_ptr(), ws.data_ptr(),
                   B, H * W, C, Cs, 1.0 / B)

        # head by head (conversion, CE, conversion back): both add to `loss`
        ctx.save_for_backward(*[nchw_loss((t,), label, kernel)[0] for t in (logits, aux) if t is not None])
        ctx.has_aux = aux is not None
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        saved = ctx.saved_tensors
        return saved[0] * go, saved[1] * go if ctx.has_aux else None, None


class _MaskedCostFunction(torch.autograd.Function):
    """MSAUWrapper.loss under a cost and class weights on NCHW fp32 logits: one msau_masked_cost for both heads, every
    sample a document of its own; `kind` / `param` a checked cost's, `class_w` fp32 [C] on the device or None.  The conversion
    launches are those of training/cost.py's _UnetCost (msau_amd.plan_loss.nchw_loss)."""

    @staticmethod
    def forward(ctx, logits, aux, label, kind, param, class_w):
        loss3 = torch.empty((3,), dtype=torch.float32, device=logits.device)
        two = aux is not None

        def kernel(nhwc, dn, label, hist, B, H, W, C, Cs, s):
            ws = torch.empty((int(L.load().msau_masked_cost_ws_floats(kind, B, H, W, C)),), dtype=torch.float32, device=logits.device)
            L.call("msau_masked_cost", s, L.F32, kind, param, nhwc[0], nhwc[1] if two else None, label, None,
                   class_w.data_ptr() if class_w is not None else None, hist, NCHW_HIST_K, dn[0], dn[1] if two else None,
                   loss3.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)

        ctx.save_for_backward(*nchw_loss((logits, aux) if two else (logits,), label, kernel,
                                         hist=class_w is not None or kind == L.COST_DICE))
        ctx.has_aux = two
        return loss3[0].clone()

    @staticmethod
    def backward(ctx, go):
        saved = ctx.saved_tensors
        return saved[0] * go, saved[1] * go if ctx.has_aux else None, None, None, None, None


def _device_class_weights(holder, class_weights, n_class: int, device) -> Optional[torch.Tensor]:
    """the class weights on the device, uploaded again only when they change; `holder` (a TrainEngine, a MSAUWrapper) keeps the
    last upload in `_cw`"""
    if class_weights is None:
        return None
    host = torch.as_tensor(class_weights).detach().to(device="cpu", dtype=torch.float32).reshape(-1).contiguous() \
        if not (isinstance(class_weights, torch.Tensor) and class_weights.is_cuda) else None
    n = host.numel() if host is not None else class_weights.numel()
    if n != n_class:
        raise ValueError(f"class_weights must hold n_class = {n_class} values, got {n}")
    if host is None:                                 # already on the device: the caller keeps it current
        return class_weights.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    kept = getattr(holder, "_cw", None)
    if kept is None or kept[1].device != torch.device(device) or not torch.equal(kept[0], host):
        holder._cw = (host.clone(), host.to(device))
    return holder._cw[1]


class MSAUWrapper(nn.Module):
    """API-compatible with model/model.py:399-459.  Extra model_kwargs: `num_blocks` (stages,
    reference hard-codes 3: model.py:355) and `dtype` ("fp32" | "bf16" activation/weight storage)."""

    def __init__(self, channels=1, n_class=2, model_kwargs={}):
        super().__init__()
        self.n_class = n_class
        self.channels = channels
        kw = dict(model_kwargs)
        self.scale_space_num = kw.get("scale_space_num", 6)
        self.res_depth = kw.get("res_depth", 3)
        self.featRoot = kw.get("featRoot", 8)
        self.filter_size = kw.get("filter_size", 3)
        self.pool_size = kw.get("pool_size", 2)
        self.activation_name = kw.get("activation_name", "relu")
        if self.activation_name not in ("relu", "elu"):
            # (the reference's constructor leaves `self.activation` unset for any other name and fails with AttributeError two lines on)
            raise ValueError("activation_name must be 'relu' or 'elu' (model/model.py:412-416)")
        self.model = kw.get("model", "msau")
        self.num_scales = kw.get("num_scales", 3)
        self.final_act = kw.get("final_act", "softmax")
        if self.final_act not in ("softmax", "identity"):
            # the reference's default "sigmoid" raises TypeError in its own constructor (model.py:429)
            raise ValueError("final_act must be 'softmax' or 'identity'")
        self.num_blocks = kw.get("num_blocks", 3)
        self.dtype_name = kw.get("dtype", "fp32")
        self._dtype = DTYPES[self.dtype_name]
        if self.pool_size != 2 or self.filter_size % 2 != 1:
            raise NotImplementedError("pool_size must be 2 and filter_size odd")
        widest = self.featRoot * 2 ** (self.scale_space_num - 1)
        if widest > 256:
            # 256 = the reference's constructor defaults (6 scales from 8 channels, dilation 32: model/model.py:406-408); the
            # attention kernels are instantiated up to (32, 256) and the LRN fast path up to 256 channels
            raise NotImplementedError(f"featRoot * 2^(scale_space_num-1) = {widest} channels: the HIP kernels support up to 256")
        self.cfg = dict(channels=channels, n_class=n_class, scale_space_num=self.scale_space_num,
                        res_depth=self.res_depth, featRoot=self.featRoot, filter_size=self.filter_size,
                        pool_size=self.pool_size, num_blocks=self.num_blocks, activation=self.activation_name)
        self.cfg.update(self._variant_cfg(kw))
        for opt in ("reuse_activations", "overlap_wgrad", "overlap_max_pix", "deterministic"):      # execution options of the plan
            if opt in kw:
                self.cfg[opt] = kw[opt]

        shapes = param_shapes(self.cfg)
        self._poff: Dict[str, int] = {}
        self._pshape: Dict[str, Tuple[int, ...]] = dict(shapes)
        off = 0
        for k, shp in shapes.items():
            self._poff[k] = off
            off += _ru4(int(math.prod(shp)))
        self._total = off
        self._flat = torch.zeros(self._total, dtype=torch.float32)
        gen = torch.Generator().manual_seed(int(kw.get("seed", torch.initial_seed() % (2 ** 31))))
        self._named = []
        self.msau_net = _Node()
        boxes: Dict[tuple, tuple] = {}
        for k, shp in shapes.items():
            n = int(math.prod(shp))
            leaf = k.rsplit(".", 1)[1]
            if leaf in ("x_min", "x_max", "y_min", "y_max"):
                # BoxConv2d boxes in units of the max box size: a random centre in the middle half, a random half extent of
                # 1/28 .. 1/4 (the third-party package's own initialiser is unavailable: unpinned, oracle/box_oracle.py)
                axis = (k.rsplit(".", 1)[0], leaf[0])
                if axis not in boxes:
                    centre = (torch.rand(shp, generator=gen) - 0.5) * 0.5
                    half = 1.0 / 28 + torch.rand(shp, generator=gen) * (0.25 - 1.0 / 28)
                    boxes[axis] = (centre - half, centre + half)
                val = boxes[axis][0 if leaf.endswith("min") else 1]
            else:
                wshp = shapes[k[:-4] + "weight"] if k.endswith(".bias") else shp
                val = _init_param(k, shp, gen, wshp[1] * wshp[2] * wshp[3])
            self._flat[self._poff[k]:self._poff[k] + n] = val.reshape(-1)
            p = nn.Parameter(self._flat[self._poff[k]:self._poff[k] + n].view(shp))
            self._named.append((k, p))
            node = self
            parts = k.split(".")
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, _Node())
                node = node._modules[part]
            node.register_parameter(parts[-1], p)
        # parameters that never receive a gradient: the last stage's attention (model.py:149-150)
        self._dead = {k for k in shapes
                      if f"blocks.{self.num_blocks - 1}.downsamplingblock.layer_attentions" in k}
        self.predictor = nn.Softmax(dim=1) if self.final_act == "softmax" else nn.Sequential()
        self.criterion = nn.CrossEntropyLoss()
        self._plans: "OrderedDict[tuple, Plan]" = OrderedDict()
        self.max_cached_plans = 4               # LRU bounds: number of plans and bytes of their activation buffers
        self.max_plan_bytes = 64 << 30

    def _variant_cfg(self, kw: dict) -> dict:
        """extra plan / parameter configuration of a network variant (BMSAUWrapper: the box-convolution blocks)"""
        return {}

    # ---- flat parameter storage ---------------------------------------------------------------
    def _rebind(self):
        for k, p in self._named:
            n = p.numel()
            p.data = self._flat[self._poff[k]:self._poff[k] + n].view(self._pshape[k])
            p.grad = None
        self._plans.clear()

    def _apply(self, fn, recurse=True):
        new_flat = fn(self._flat)
        if new_flat.dtype != torch.float32:
            raise TypeError("MSAUWrapper keeps fp32 master parameters; choose bf16 storage with model_kwargs['dtype']")
        self._flat = new_flat
        self._rebind()
        return self

    @property
    def flat_parameters(self) -> torch.Tensor:
        return self._flat

    # ---- plans ----------------------------------------------------------------------------------
    def _need_gpu(self, inp: Optional[torch.Tensor] = None):
        """the refusal of CPU inputs: of the tensor `inp`, or (None) of a model that is not on the GPU"""
        if not (self._flat if inp is None else inp).is_cuda:
            what = "the model must be on the GPU" if inp is None else "input must be a CUDA/HIP tensor"
            raise RuntimeError(f"MSAUWrapper runs on an MI355X through libmsau_hip.so; {what} (there is no CPU fallback)")

    def _plan_for(self, x: torch.Tensor, training: bool, ragged: bool = False) -> Plan:
        self._need_gpu(x)
        B, C, H, W = x.shape
        if C != self.channels:
            raise ValueError(f"expected {self.channels} input channels, got {C}")
        return self._plan_for_shape(B, H, W, x.device, training, ragged)

    def _plan_for_shape(self, B: int, H: int, W: int, device, training: bool, ragged: bool = False) -> Plan:
        if self._flat.device != device:
            raise RuntimeError(f"model is on {self._flat.device}, input on {device}")
        key = (B, H, W, training, bool(ragged))
        plan = self._plans.get(key)
        if plan is None:
            plan = Plan(self.cfg, B, H, W, self._dtype, device, self._poff, self._pshape, training=training, ragged=ragged)
            plan.generation = 0                 # bumped by every grad-mode forward (see _MSAUFunction)
            self._plans[key] = plan
            while len(self._plans) > 1 and (len(self._plans) > self.max_cached_plans or
                                            sum(p.activation_bytes() for p in self._plans.values()) > self.max_plan_bytes):
                self._plans.popitem(last=False)     # captured graphs live on the plan object and go with it
        else:
            self._plans.move_to_end(key)
        return plan

    def _plan(self, B: int, H: int, W: int, device, training: bool, sizes) -> Plan:
        """the plan of an eager batch given by its canvas: ragged when it has `sizes`, whose extents go to the device here"""
        plan = self._plan_for_shape(B, H, W, device, training, ragged=sizes is not None)
        plan.set_extents(sizes)
        return plan

    # ---- reference API ----------------------------------------------------------------------------
    def forward(self, inp, sizes=None):
        """`sizes` (ragged batch): a CPU integer tensor [B, 2] of every document's (h, w), placed at the origin of the H x W canvas
        of `inp`; each sample then computes what the document alone would (its crop of the outputs), and the outputs are 0
        outside the documents.  None: the dense batch."""
        x = inp.contiguous().float()
        if sizes is not None:
            sizes = self._check_sizes(x, sizes)
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for _, p in self._named)
        if need_grad:
            outs = _MSAUFunction.apply(self, x, sizes, *[p for _, p in self._named])
            logits = outs[0]
            aux = outs[1] if len(outs) > 1 else None
        else:
            plan = self._plan_for(x, training=False, ragged=sizes is not None)
            plan.set_extents(sizes)
            lg, ax = plan.forward(self._flat, x)
            logits, aux = lg.clone(), (ax.clone() if ax is not None else None)
        if self.final_act == "softmax":
            with torch.no_grad():
                B, C, H, W = logits.shape
                pred = torch.empty_like(logits)
                L.call("msau_softmax_channels_nchw", torch.cuda.current_stream().cuda_stream, logits.data_ptr(),
                       pred.data_ptr(), B, C, H * W)
        else:
            pred = logits
        return pred, logits, aux

    def _check_sizes(self, x: torch.Tensor, sizes) -> torch.Tensor:
        """host-side check of a ragged batch's sizes against the canvas of x (no device sync)"""
        B, _, H, W = x.shape
        return Plan.check_sizes(sizes, B, H, W)

    def _check_sizes_for(self, sizes, B: int, H: int, W: int) -> Optional[torch.Tensor]:
        """`_check_sizes` for the entry points that have a canvas shape and no input tensor (box lists, id masks); None stays None"""
        return None if sizes is None else self._check_sizes(torch.empty((B, 0, H, W)), sizes)

    @staticmethod
    def _check_ids(ids: torch.Tensor, device=None) -> torch.Tensor:
        """a character-id mask as the kernels take it: int32 [B,H,W], contiguous (moved to `device` when one is given)"""
        if ids.dim() != 3:
            raise ValueError("ids must be [B,H,W]")
        return ids.to(device=device, dtype=torch.int32).contiguous()

    @torch.no_grad()
    def predict_nhwc(self, inp: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None, graph: bool = False,
                     sizes=None):
        """Forward-only path for `KVModel.predict` (inference/kv_model.py:305-313): one of
          inp float [B,C,H,W]   -- the dense grid the reference builds with to_categorical, or
          ids int   [B,H,W]     -- the character-id mask itself; the one-hot grid is painted on the device
        -> (pred fp32 [B,H,W,n_class] = softmax over classes, already in the NHWC order `_extract_value` wants,
            argmax uint8 [B,H,W] = np.argmax(pred, -1)).
        No activations are kept (buffers are reused by liveness) and softmax + argmax run in the last conv's epilogue.
        The returned tensors are the plan's buffers: copy them before the next call if they must survive it.
        graph=True replays the sweep as a HIP graph (captured per shape on first use, on a dedicated stream): at
        batch 1 the ~120 launches are host-bound and the replay is what sets the latency.
        `sizes` (ragged batch): the CPU integer [B, 2] of `forward` -- every document's (h, w) at the origin of the canvas.
        Inside each document the outputs are what the document alone produces; outside them they are unspecified (crop them).
        The ragged plan runs the stand-alone head (msau_softmax_argmax_nhwc); with graph=True one graph per canvas and input
        kind is captured and the extents are refreshed before every replay."""
        if (inp is None) == (ids is None):
            raise ValueError("give exactly one of inp / ids")
        if self.final_act != "softmax":
            raise ValueError("predict_nhwc is the softmax head; final_act is %r" % (self.final_act,))
        if self.n_class > 255:
            raise ValueError("the argmax map is uint8: at most 255 classes")
        if ids is not None:
            ref = ids = self._check_ids(ids, self._flat.device)
            B, H, W = ids.shape
        else:
            ref = inp = inp.contiguous().float()
            B, C, H, W = inp.shape
        if sizes is not None:
            sizes = Plan.check_sizes(sizes, B, H, W)
        self._need_gpu(ref)
        ragged = sizes is not None
        plan = self._plan_for(inp, False, ragged) if ids is None else self._plan_for_shape(B, H, W, ref.device, False, ragged)
        if not graph:
            plan.set_extents(sizes)
            return plan.predict(self._flat, x_nchw=inp, ids=ids)
        kind = "ids" if ids is not None else "dense"
        if getattr(self, "_pstream", None) is None:
            self._pstream = torch.cuda.Stream(device=ref.device)      # never replay into the NULL stream (see TrainEngine)
        cur, gs = torch.cuda.current_stream(), self._pstream
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            plan.set_extents(sizes)                                   # read by the captured sweep at every replay
            cache = plan.__dict__.setdefault("_pgraphs", {})
            if kind not in cache:
                static = ref.clone()
                kw = dict(ids=static) if ids is not None else dict(x_nchw=static)
                plan.predict(self._flat, **kw)                        # warm-up outside capture
                torch.cuda.synchronize()
                g = _keep_graph(torch.cuda.CUDAGraph())
                with _capture_section():
                    with torch.cuda.graph(g, stream=gs):
                        plan.predict(self._flat, **kw)
                cache[kind] = (g, static)
            g, static = cache[kind]
            static.copy_(ref, non_blocking=True)
            g.replay()
        cur.wait_stream(gs)
        return plan.head_probs, plan.head_argmax

    @torch.no_grad()
    def predict_regions(self, inp: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None, sizes=None, *,
                        line_ids: torch.Tensor, char_pos: torch.Tensor, boxes, cap_regions: Optional[int] = None,
                        cap_pairs: Optional[int] = None, large: bool = False, scores: bool = False):
        """`predict_nhwc` followed, on the same stream, by the region kernel (csrc/regions.hip) on the class map the head wrote:
        nothing per pixel comes back to the host.  inp / ids / sizes as in `predict_nhwc`; line_ids / char_pos: 16-bit integer
        [B, H, W] tensors on the canvas of the input, zero outside the documents (msau_amd.data.ragged.pack_masks), moved to the
        device here if they are not there; boxes: per document the [x1, y1, x2, y2] of its text lines in grid coordinates.
        -> (tables, flags, argmax): per document its region table (msau_amd.inference.regions) or None, per document the
        overflow flags (0 = the table is complete; otherwise run `regions_host` on that document's crop of `argmax`), and the
        plan's uint8 [B, H, W] class map on the device.  large=True: documents beyond the LDS form's pixel limit get their table
        from the large form of the kernel (`regions_device`).  Eager only: there is no captured-graph form of the region stage.
        scores=True: the scored form of the kernel reads the head's probabilities where they are (the plan's `head_probs`)
        -> (tables, flags, argmax, scores), scores as `regions_device(..., probs=)` returns them (None for a flagged document);
        `self.last_head_probs` is then that fp32 [B, H, W, n_class] buffer, for the caller that has to redo a flagged document on
        the host (`regions_host(..., probs=)` on its crop).  Like `argmax` it is the plan's own: valid until the next call."""
        from .inference.regions import regions_device
        probs, amax = self.predict_nhwc(inp=inp, ids=ids, sizes=sizes)
        dev = amax.device
        kw = dict(sizes=None if sizes is None else torch.as_tensor(sizes).tolist(), cap_regions=cap_regions, cap_pairs=cap_pairs,
                  large=large)
        if scores:
            self.last_head_probs = probs
            tables, flags, sums = regions_device(amax, line_ids.to(dev), char_pos.to(dev), boxes, self.n_class, probs=probs, **kw)
            return tables, flags, amax, sums
        tables, flags = regions_device(amax, line_ids.to(dev), char_pos.to(dev), boxes, self.n_class, **kw)
        return tables, flags, amax

    @torch.no_grad()
    def confusion_matrix(self, inp: torch.Tensor, labels: torch.Tensor, sizes=None, zero_as: Optional[int] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Evaluation counts on the device: int64 [n_class, n_class], rows = labels, columns = predictions, over the pixels whose
        label is in [1, n_class) (and, with `sizes`, that lie inside their document).  The prediction is the first maximum of the
        logits, exactly `argmax(0)` of the fp32 NCHW logits `forward` returns; with `zero_as`, a predicted 0 counts as that class
        (the reference's test-split remap, train_chargrid_funsd_msau.py:140).  inp float [B,C,H,W], labels int [B,H,W] (or
        [B,1,H,W]); `sizes` as in `forward`.  Runs the forward-only plan without exporting the logits and adds into `out` when
        given (batches of an epoch accumulate on the device; read the matrix once)."""
        x = inp.contiguous().float()
        if x.dim() != 4:
            raise ValueError("inp must be [B,C,H,W]")
        B, Cin, H, W = x.shape
        if int(labels.numel()) != B * H * W:
            raise ValueError(f"labels must hold [B,H,W] = {(B, H, W)} values, got shape {tuple(labels.shape)}")
        out = self._confusion_args(zero_as, out, x.device)
        if sizes is not None:
            sizes = self._check_sizes(x, sizes)
        if labels.device.type == "cpu" and labels.numel() and \
                bool((labels < 0).any() or (labels >= self.n_class).any()):
            raise ValueError(f"labels must lie in [0, {self.n_class})")
        self._need_gpu(x)
        lab = labels.to(device=x.device, dtype=torch.int64).reshape(B, H, W).contiguous()
        plan = self._plan_for(x, training=False, ragged=sizes is not None)
        plan.set_extents(sizes)
        plan.forward(self._flat, x, export=False)
        return self._count_confusion(plan, lab, zero_as, out)

    @torch.no_grad()
    def confusion_matrix_boxes(self, grid_boxes, label_boxes, B: int, H: int, W: int, feats=None, sizes=None,
                               zero_as: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`confusion_matrix` without a dense grid: the batch comes as BOX LISTS (and, for the embedding grid, a feature table), as
        `TrainEngine.step_boxes` takes them -- int32 [n][6] = sample, y0, y1, x0, x1, value; numpy arrays or device tensors.  The label
        mask is painted on the device; with `feats` and a box-list instance of the first conv (MSAU_CONV_OWNER) the grid is never
        painted, otherwise it is painted into the forward-only plan's input buffer.  `sizes` (ragged batch): the CPU integer [B, 2]
        of `forward`, every document's boxes in its own coordinates (msau_amd.data.ragged.pack_boxes).  Counts, `zero_as` and `out`
        as in `confusion_matrix`: rows = painted labels in [1, n_class), columns = first maximum of the logits."""
        dev = self._flat.device
        out = self._confusion_args(zero_as, out, dev)
        sizes = self._check_sizes_for(sizes, B, H, W)
        self._need_gpu()
        plan = self._plan(B, H, W, dev, False, sizes)
        feed, lab = self._paint_boxes(plan, grid_boxes, label_boxes, feats)
        plan.forward(self._flat, None, export=False, **feed)
        return self._count_confusion(plan, lab, zero_as, out)

    def _confusion_args(self, zero_as, out: Optional[torch.Tensor], dev, new: bool = True) -> Optional[torch.Tensor]:
        """the checks `confusion_matrix`, `confusion_matrix_boxes` and the box votes share -> `out`, a new matrix on `dev` when it is
        None (new=False: None stays None, the box votes count into a matrix only when they are given one)"""
        C = self.n_class
        if C > 64:
            raise ValueError(f"confusion_matrix counts at most 64 classes, the model has {C}")
        if zero_as is not None and not (0 <= int(zero_as) < C):
            raise ValueError(f"zero_as must be a class in [0, {C}), got {zero_as}")
        if out is None:
            return torch.zeros((C, C), dtype=torch.int64, device=dev) if new else None
        if out.dtype != torch.int64 or tuple(out.shape) != (C, C) or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 [{C}, {C}] tensor on {dev}")
        return out

    def _count_confusion(self, plan: Plan, lab: torch.Tensor, zero_as, out: torch.Tensor) -> torch.Tensor:
        """add the counts of the logits `plan` holds against the labels `lab` (int64 [B,H,W] on the device) into `out`"""
        lg = plan.logits
        L.call("msau_eval_confusion", torch.cuda.current_stream().cuda_stream, plan.dtype, lg.data.data_ptr(), lab.data_ptr(),
               out.data_ptr(), plan.B, plan.H, plan.W, lg.C, lg.Cs, -1 if zero_as is None else int(zero_as),
               plan.extent_ptr(lg) if plan.ragged else None)
        return out

    @torch.no_grad()
    def box_predictions(self, inp: torch.Tensor, boxes, sizes=None, zero_as: Optional[int] = None, owned: bool = False,
                        out: Optional[torch.Tensor] = None, hist: bool = False):
        """Entity-level predictions on the device: every box of `boxes` (int32 [n][6] = sample, y0, y1, x0, x1, value; a numpy array
        or a device tensor; an entity list such as the label boxes of msau_amd.data.raster.document_boxes, or its
        document_word_boxes) gets the class most of its pixels vote for.  A pixel's class is the first maximum of the logits,
        exactly `argmax(0)` of the fp32 NCHW logits `forward` returns, with `zero_as` as in `confusion_matrix`; boxes are clipped to
        the canvas, or with `sizes` (as in `forward`; boxes in their own document's coordinates) to their document.  owned=False:
        the whole clipped box votes; owned=True: only the pixels the box owns after the list is painted in order (a later box
        takes the pixels it shares with an earlier one), so every pixel votes for one box.
        -> (pred int32 [n]: the smallest class among the most voted, -1 for a box without a voting pixel; votes int32 [n, 2] =
        (votes of the winner, voting pixels); the per-class votes int32 [n, n_class] with hist=True, else None), on the device.
        `out`: an int64 [n_class, n_class] matrix on the device that gets out[value, pred] += 1 for every box with a value in
        [1, n_class) and a prediction (batches of an epoch accumulate; msau_amd.training.metrics.classification_report takes it).
        Runs the forward-only plan without exporting the logits; nothing waits for the device."""
        x = inp.contiguous().float()
        if x.dim() != 4:
            raise ValueError("inp must be [B,C,H,W]")
        out = self._confusion_args(zero_as, out, x.device, new=False)
        if sizes is not None:
            sizes = self._check_sizes(x, sizes)
        self._need_gpu(x)
        from .data import raster
        bt, n = raster._dev_boxes(boxes, x.device)
        plan = self._plan_for(x, training=False, ragged=sizes is not None)
        plan.set_extents(sizes)
        plan.forward(self._flat, x, export=False)
        owner = None
        if owned and n:
            owner = torch.empty((plan.B, plan.H, plan.W), dtype=torch.int32, device=x.device)
            raster._owner(torch.cuda.current_stream(x.device).cuda_stream, bt, n, owner, plan.B, plan.H, plan.W,
                          plan.extents[0] if plan.ragged else None)
        return self._vote_boxes(plan, bt, n, owner, zero_as, out, hist)

    @torch.no_grad()
    def box_predictions_boxes(self, grid_boxes, label_boxes, B: int, H: int, W: int, feats=None, sizes=None,
                              zero_as: Optional[int] = None, owned: bool = False, out: Optional[torch.Tensor] = None,
                              hist: bool = False):
        """`box_predictions` for a batch that comes as BOX LISTS, fed as `confusion_matrix_boxes` feeds it: the voted boxes are the
        label boxes.  owned=True votes with the owner map the label painter has made of them anyway (nothing is painted twice)."""
        dev = self._flat.device
        out = self._confusion_args(zero_as, out, dev, new=False)
        sizes = self._check_sizes_for(sizes, B, H, W)
        self._need_gpu()
        plan = self._plan(B, H, W, dev, False, sizes)
        feed, _lab, (owner, bt, n) = self._paint_boxes(plan, grid_boxes, label_boxes, feats, label_owner=True)
        plan.forward(self._flat, None, export=False, **feed)
        return self._vote_boxes(plan, bt, n, owner if owned and n else None, zero_as, out, hist)

    def _vote_boxes(self, plan: Plan, bt: Optional[torch.Tensor], n: int, owner: Optional[torch.Tensor], zero_as,
                    out: Optional[torch.Tensor], hist: bool):
        """msau_box_vote on the logits `plan` holds: the n boxes of the device list `bt` (None when n == 0), `owner` their owner map
        or None -> (pred, votes, hist or None) on the device; counts go into `out` when it is given"""
        lg, dev = plan.logits, self._flat.device
        stream = torch.cuda.current_stream(dev)
        pred = torch.empty((n,), dtype=torch.int32, device=dev)
        votes = torch.empty((n, 2), dtype=torch.int32, device=dev)
        hs = torch.empty((n, lg.C), dtype=torch.int32, device=dev) if hist else None
        L.call("msau_box_vote", stream.cuda_stream, plan.dtype, lg.data.data_ptr(), bt.data_ptr() if n else None, n,
               owner.data_ptr() if owner is not None else None, pred.data_ptr(), votes.data_ptr(),
               hs.data_ptr() if hs is not None else None, out.data_ptr() if out is not None else None, plan.B, plan.H, plan.W,
               lg.C, lg.Cs, -1 if zero_as is None else int(zero_as), plan.extent_ptr(lg) if plan.ragged else None)
        # an uploaded box list and the owner map must outlive the launch that reads them (see msau_amd/data/raster.py)
        for t in (bt, owner):
            if t is not None:
                t.record_stream(stream)
        return pred, votes, hs

    def _paint_boxes(self, plan: Plan, grid_boxes, label_boxes, feats, out: Optional[torch.Tensor] = None, label_owner: bool = False):
        """A batch of box lists (as `TrainEngine.step_boxes` takes them) on the canvas of `plan` -> (the keywords that make
        `Plan.forward` read it, labels int64 [B,H,W]).  With a feature table and a box-list instance of the first conv
        (MSAU_CONV_OWNER, csrc/ownerconv.hip) only the owner map is painted: the embedding grid is piecewise constant, the conv and
        its weight gradient work from the per-pixel box index and the table.  Otherwise the grid goes into the plan's input buffer
        -- or into `out`, another buffer of that shape (`TrainEngine.prefetch_boxes`; never the box-list conv then).  On a ragged plan
        the painters clip to the plan's own level-0 extents: owner map, grid and labels are empty / zero outside the documents as
        they enter, nothing has to be zeroed afterwards.  label_owner=True: a third result, the label painter's (owner map, label
        boxes on the device or None, their number) for `_vote_boxes`."""
        from .data import raster
        B, H, W, dev = plan.B, plan.H, plan.W, self._flat.device
        ext = plan.extents[0] if plan.ragged else None
        if feats is not None and out is None and plan._feed_owner(None):
            ft = feats if isinstance(feats, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(dev)
            owner, fb, nf, labels, *lown = raster.owner_maps(grid_boxes, label_boxes, B, H, W, dev, sizes=ext, label_owner=label_owner)
            return (dict(owner=(owner, fb, nf, ft)), labels, *lown)
        buf = plan.input_nhwc if out is None else out
        if feats is None:
            _, labels, *lown = raster.rasterize(grid_boxes, label_boxes, B, H, W, self.channels, self.dtype_name, dev, out=buf, sizes=ext,
                                                label_owner=label_owner)
        else:
            _, labels, *lown = raster.rasterize_dense(grid_boxes, label_boxes, feats, B, H, W, self.dtype_name, dev, out=buf, sizes=ext,
                                                      label_owner=label_owner)
        return (dict(nhwc_ready=True, nhwc_clean=True), labels, *lown)

    @torch.no_grad()
    def eval_unet(self, ids: torch.Tensor, labels: torch.Tensor, aux_labels: torch.Tensor, sizes=None, class_weights=None, cost=None):
        """Validation of a group of documents on the device: the forward-only plan fed with the character-id mask (`ids` int32
        [B,H,W], as `TrainEngine.step_ids` takes it), then UNetLoss and the reference's accuracy per document in one launch
        (msau_unet_eval) on the logits both heads left in the plan -- nothing is exported, no one-hot tensor exists and nothing
        waits for the device.  `labels` / `aux_labels` int64 [B,H,W] (each head against its own map), `sizes` and `class_weights`
        as `TrainEngine.step_unet` takes them.  -> (doc_loss fp32 [B, 2], doc_counts int32 [B, 2, 2]) on the device: per document
        and head (0 = final, 1 = auxiliary; zeros without an auxiliary head) the loss the document has alone, and (labelled,
        correct) over its pixels with a label in [1, n_class), the prediction being `argmax` of the fp32 logits `forward` returns.
        msau_amd.training.kv_trainer.summarize turns rows into the reference's epoch figures.  No training plan is built or
        touched, parameters and gradients are left alone.  `cost` as `TrainEngine.step_unet` takes it: the documents' losses are
        then those of that cost (msau_unet_cost_eval) -- validate with the loss that is trained."""
        cost = unet_cost(cost)
        cw = _device_class_weights(self, class_weights, self.n_class, self._flat.device)
        ids = self._check_ids(ids)
        B, H, W = ids.shape
        sizes = self._check_sizes_for(sizes, B, H, W)
        self._need_gpu(ids)
        labels = labels.reshape(B, H, W).contiguous().long()
        plan = self._plan(B, H, W, ids.device, False, sizes)
        aux_labels = aux_labels.reshape(B, H, W).contiguous().long() if plan.aux is not None else None
        plan.forward(self._flat, None, export=False, ids=ids)
        return plan.eval_unet(labels, aux_labels, cw, cost=cost)

    def eval_kv(self, tables, class_weights=None, round_to: int = 16, cost=None):
        """`eval_unet` on a group of key-value documents given as their training tables (`KVTrainBatches.validation()`): one
        upload of the packed tables, one painter launch (kv_data.paint_train_device; a table that is not `ok` is painted on the
        host, as in `TrainEngine.step_kv`), the forward and the evaluation launch."""
        cost = unet_cost(cost)
        from .training import kv_data
        ids, labels, aux_labels, sizes = kv_data.paint_train_device(tables, round_to=round_to, device=self._flat.device)
        return self.eval_unet(ids, labels, aux_labels, sizes=sizes, class_weights=class_weights, cost=cost)

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load_weights(self, path):
        self.load_state_dict(torch.load(path, map_location=self._flat.device))

    def loss(self, out_grid, out_grid_aux, label_mask, cost=None, class_weights=None):
        """Masked CE of final + aux logits over pixels with label != 0 (model/model.py:446-459).
        Accepts label_mask [B,H,W] (the reference: B = 1): per-sample masked mean, then mean over B.
        `cost` (msau_amd.plan.unet_cost: {"cost_name": "focal", "gamma": 2.0}, {"cost_name": "dice", "smooth": 1.0}) and
        `class_weights` (n_class values): the masked loss under that cost and with those weights, what
        `TrainEngine(cost=..., class_weights=...)` trains.  Neither: the masked CE as ever."""
        cost = unet_cost(cost)
        if cost is None and class_weights is None:
            return _MaskedCEFunction.apply(out_grid, out_grid_aux, label_mask)
        cw = _device_class_weights(self, class_weights, self.n_class, out_grid.device)
        kind, param = (cost.kind, cost.param) if cost is not None else (L.COST_CE, 0.0)
        return _MaskedCostFunction.apply(out_grid, out_grid_aux, label_mask, kind, param, cw)

    @torch.no_grad()
    def eval_loss(self, inp, labels, sizes=None, *, cost=None, class_weights=None):
        """Validation of the masked loss on the device: the forward-only plan fed with `inp` (NCHW, as `forward` takes it; `sizes`
        for a ragged batch), then per document the loss of `loss` / `TrainEngine.step` under `cost` and `class_weights` and the
        accuracy counts, in one call (msau_masked_cost_eval) on the logits both heads left in the plan.  -> (doc_loss fp32 [B, 2],
        doc_counts int32 [B, 2, 2]) on the device, as `eval_unet` returns them: head 0 = final, 1 = auxiliary, counts = (labelled,
        correct).  Nothing is exported and nothing waits for the device.  `cost=None`: the masked CE's per-document loss."""
        cost = unet_cost(cost)
        cw = _device_class_weights(self, class_weights, self.n_class, self._flat.device)
        self._need_gpu(inp)
        x = inp.contiguous().float()
        B, _, H, W = x.shape
        if sizes is not None:
            sizes = self._check_sizes(x, sizes)
        labels = labels.reshape(B, H, W).contiguous().long()
        plan = self._plan_for(x, training=False, ragged=sizes is not None)
        plan.set_extents(sizes)
        plan.forward(self._flat, x, export=False)
        return plan.eval_masked(labels, cw, cost=cost)


# A stream capture is in "global" mode: a device synchronisation (or a graph's destruction) from ANY Python context while it runs --
# e.g. the finaliser of another engine, whenever the garbage collector gets to it -- makes hipStreamEndCapture abort the process
# (seen once in four full GPU test runs, 2026-10-04).  Graphs whose engine dies during a capture wait in _graveyard until the next
# safe point (TrainEngine.step / _drop_graphs outside a capture).
_capturing = 0
_graveyard: list = []
# FINDING (MI355X / ROCm 7.2 / torch 2.10; rounds 3-4).  Destroying a captured graph (torch.cuda.CUDAGraph's destructor ->
# hipGraphExecDestroy / hipGraphDestroy) and capturing another one crashed the process -- abort inside the destruction or inside
# hipStreamEndCapture, a segmentation fault, once a hang -- in half of the stand-alone runs of tests/test_train_gpu.py.  Round 4 narrowed
# it down (tools/repro/, profiles/r04_graph_destroy.md): a stand-alone HIP program and a torch-only script that capture TWO-stream
# sweeps (fork / join by events from a reused pool, eager sweeps in between), destroy and re-capture pass 240 / 120 cycles; this code
# base with graph destruction crashes 4 of 8 runs when the captured backward forks its weight gradients onto the side stream and
# 0 of 8 when the same sweep is captured on ONE stream.  So a captured sweep is single-stream (Plan.backward(single_stream=True): graph
# mode is the slower, opt-in mode anyway, section 2 of DESIGN.md), graphs are ordinary objects again, and nothing is leaked: the
# round-3 remedy (one immortal reference per captured graph) is gone.
def _keep_graph(g):
    return g


class _capture_section:
    def __enter__(self):
        global _capturing
        _capturing += 1

    def __exit__(self, *exc):
        global _capturing
        _capturing -= 1
        return False


def _bury_graphs():
    """destroy the graphs of dead engines: not while a replay may still be running (ROCm 7.2: the process segfaults), not during a capture"""
    if _graveyard and not _capturing:
        torch.cuda.synchronize()
        _graveyard.clear()          # (the graphs, their private pools and the static input copies go)


def _ru4(n: int) -> int:
    return -(-n // 4) * 4          # keep every parameter 16-byte aligned inside the flat buffer


OPTIMIZERS = {"adam": L.OPTIM_ADAM, "rmsprop": L.OPTIM_RMSPROP, "momentum": L.OPTIM_MOMENTUM}
# the name of a kind's state buffers in TrainEngine.state_dict() and in torch.optim's state (state_a, state_b of msau_optim_step)
OPTIM_BUFFERS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "momentum": ("momentum_buffer",)}


def torch_optim_kind(sd: dict) -> str:
    """which of the engine's optimisers a `torch.optim.*.state_dict()` belongs to, by the options of its parameter group:
    Adam has `betas`, RMSprop `alpha`, SGD `nesterov`.  The variants msau_optim_step does not implement are refused."""
    g0 = sd["param_groups"][0]
    if "betas" in g0:
        return "adam"
    if "alpha" in g0:
        if g0.get("momentum", 0) != 0 or g0.get("centered", False):
            raise ValueError("RMSprop state with momentum or centered=True: the engine implements plain RMSprop only")
        return "rmsprop"
    if "nesterov" in g0:
        if g0.get("nesterov", False) or g0.get("dampening", 0) != 0:
            raise ValueError("SGD state with Nesterov momentum or dampening: the engine implements plain momentum only")
        return "momentum"
    raise ValueError(f"optimizer state of an unknown kind (options {sorted(g0)})")


def torch_optim_state_to_flat(sd: dict, named, poff: Dict[str, int], total: int, kind: str):
    """`torch.optim.{Adam,RMSprop,SGD}.state_dict()` over the model's parameters in registration order -> (step, [flat fp32 CPU
    tensor of `total` elements per buffer of OPTIM_BUFFERS[kind]], the first parameter group).  `named`: [(key, numel)] of the
    parameters the optimiser was built over, `poff` their offsets in the flat buffer.  Parameters the optimiser never stepped
    (no gradient: the dead last-stage attention) have no entry and keep zero state.  ValueError when the state is another
    kind's or does not fit the parameters.  CPU tensors in, CPU tensors out."""
    have = torch_optim_kind(sd)
    if have != kind:
        raise ValueError(f"optimizer state is {have}'s, the engine runs {kind}")
    groups, state = sd["param_groups"], sd["state"]
    order = [pid for g in groups for pid in g["params"]]
    if len(order) != len(named):
        raise ValueError(f"optimizer state covers {len(order)} parameters, the model has {len(named)}")
    names = OPTIM_BUFFERS[kind]
    flats = [torch.zeros(total, dtype=torch.float32) for _ in names]
    step = 0
    for pid, (key, n) in zip(order, named):
        st = state.get(pid)
        if st is None:
            continue
        for name, flat in zip(names, flats):
            buf = st.get(name)
            if buf is None:                      # (SGD before its first step with a gradient)
                continue
            if buf.numel() != n:
                raise ValueError(f"optimizer state of {key}: {buf.numel()} elements, parameter has {n}")
            flat[poff[key]:poff[key] + n] = buf.detach().reshape(-1).to(device="cpu", dtype=torch.float32)
        if "step" in st:
            step = max(step, int(round(float(st["step"]))))
    return step, flats, groups[0]


def skip_ranges(dead, poff: Dict[str, int], numel: Dict[str, int]):
    """the half-open element ranges of the flat buffer that the parameters `dead` occupy (alignment padding included), ascending,
    adjacent ones merged: the `skip` argument of msau_optim_step"""
    out = []
    for b, e in sorted((poff[k], poff[k] + _ru4(numel[k])) for k in dead):
        if out and out[-1][1] == b:
            out[-1][1] = e
        else:
            out.append([b, e])
    return [tuple(r) for r in out]


class TrainEngine:
    """Fused training step on one GPU (one process per GPU under data parallelism).

    forward -> masked CE (+grad) -> backward -> [RCCL all-reduce of the flat gradient] ->
    global-norm clip + Adam, all on the flat fp32 parameter buffer of `model`
    (train_chargrid_funsd_msau.py:46-59 with lr 1e-4, clip 1.0).

    `optimizer` "adam" | "rmsprop" | "momentum", `weight_decay`, `alpha` (RMSprop), `momentum` (SGD) and `max_norm=None` (or
    <= 0: no clipping) give the optimisers of the reference's `get_optimizer` (model/training/optimizer.py; `from_opt_kwargs`
    takes its options): torch.optim's arithmetic in one fused launch (msau_optim_step), two with clipping or under Adam.  The
    default -- Adam, no weight decay -- is msau_clip_adam_step as ever.

    `cost` (msau_amd.plan.unet_cost: {"cost_name": "focal", "gamma": 2.0}, {"cost_name": "dice", "smooth": 1.0}) and `class_weights`
    (n_class values) put the masked loss of `step` / `step_ids` / `step_nhwc` / `step_boxes` / `step_prefetched` under that cost and
    those weights (`set_cost` changes them); the default is the masked CE, launch for launch."""

    def __init__(self, model: MSAUWrapper, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_norm: Optional[float] = 1.0, process_group=None, use_graph: bool = False, *, optimizer: str = "adam",
                 weight_decay: float = 0.0, alpha: float = 0.99, momentum: float = 0.9, cost=None, class_weights=None):
        self._cost = unet_cost(cost)                     # (checked first thing: a bad cost is a ValueError before a GPU is needed)
        self._cost_cw = None
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer {optimizer!r}: TrainEngine knows {sorted(OPTIMIZERS)}")
        self.model, self.lr, self.betas, self.eps, self.max_norm = model, lr, betas, eps, max_norm
        self.optimizer, self.weight_decay, self.alpha, self.momentum = optimizer, float(weight_decay), float(alpha), float(momentum)
        flat = model._flat
        if not flat.is_cuda:
            raise RuntimeError("TrainEngine needs the model on a GPU (model.cuda())")
        self.flat_grad = torch.zeros_like(flat)
        # only the state buffers the kind uses: Adam's two moments, RMSprop's square_avg, SGD's momentum_buffer
        self.m = self.v = self.square_avg = self.momentum_buffer = None
        if optimizer == "adam":
            self.m = torch.zeros_like(flat)
            self.v = torch.zeros_like(flat)
        elif optimizer == "rmsprop":
            self.square_avg = torch.zeros_like(flat)
        else:
            self.momentum_buffer = torch.zeros_like(flat)
        self.state = torch.zeros(8, dtype=torch.float32, device=flat.device)
        # the workspace of both entry points (msau_clip_adam_step: the default; msau_optim_step: everything else), so that
        # set_hyper may move the engine from one to the other; a few hundred floats
        lib = L.load()
        self.adam_ws = torch.zeros(int(max(lib.msau_adam_ws_floats(flat.numel()), lib.msau_optim_ws_floats(flat.numel()))),
                                   dtype=torch.float32, device=flat.device)
        # parameters that never receive a gradient (torch.optim leaves a parameter whose .grad is None alone: no weight decay either)
        import ctypes as C
        ranges = skip_ranges(model._dead, model._poff, {k: p.numel() for k, p in model._named})
        if len(ranges) > L.OPTIM_MAX_SKIP:
            raise RuntimeError(f"{len(ranges)} separate ranges of parameters without a gradient, msau_optim_step takes {L.OPTIM_MAX_SKIP}")
        self._skip = ranges
        self._skip_arr = (C.c_int64 * max(2 * len(ranges), 1))(*[v for r in ranges for v in r])
        from .dp import GradSync, stage_buckets
        self.pg = process_group
        self.sync = GradSync(self.flat_grad, stage_buckets(model._poff, model._total, model.num_blocks), process_group)
        self.world = self.sync.world
        self.use_graph = use_graph
        self._ar_native = self._ar_started = False       # how the last _fwd_bwd left the gradient exchange (see _allreduce)
        self._prefetched, self._pf_last = [], 1          # prefetch_boxes: the queue (at most two) and the buffer of the last step
        self._comm = None
        self._init_native_comm(process_group)
        # Graph replays run on a dedicated non-default stream.  Replaying on the legacy NULL stream after the
        # host had synchronised produced corrupted steps on ROCm 7.2 / gfx950 (nodes of consecutive launches
        # overlapping; found 2026-10-03 with tools/loss_trace.py) -- never launch these graphs into stream 0.
        self._gstream = torch.cuda.Stream(device=flat.device)
        # Captured graphs are filed on the plan under this token.  It is never re-used (id(self) is, once an engine is
        # freed: a second engine for the same model -- an lr sweep, a resume -- could then replay the dead engine's graphs,
        # whose kernel arguments point at ITS freed moments and carry ITS hyper-parameters), and it changes whenever a
        # by-value kernel argument of the captured optimiser step changes (_invalidate_graphs).
        TrainEngine._tokens += 1
        self._token = TrainEngine._tokens
        weakref.finalize(self, TrainEngine._drop_graphs, weakref.ref(model), self._token)
        self._cost_cw = _device_class_weights(self, class_weights, model.n_class, flat.device)

    _tokens = 0

    @staticmethod
    def _drop_graphs(model_ref, token):
        model = model_ref()
        if model is not None:
            doomed = [plan._tgraphs.pop(token) for plan in model._plans.values() if token in plan.__dict__.get("_tgraphs", {})]
            if doomed:
                _graveyard.extend(doomed)            # (this may be a finaliser running in the middle of somebody's stream capture)
                del doomed
                _bury_graphs()

    def _invalidate_graphs(self):
        """lr / betas / eps / max_norm are by-value arguments of msau_clip_adam_step, frozen into a captured optimiser graph:
        after changing them (load_state_dict, set_lr) the graphs of this engine are dropped and re-captured on the next step"""
        TrainEngine._drop_graphs(weakref.ref(self.model), self._token)
        TrainEngine._tokens += 1
        self._token = TrainEngine._tokens

    def set_hyper(self, lr=None, betas=None, eps=None, max_norm=None, weight_decay=None, alpha=None, momentum=None):
        """change optimiser hyper-parameters between steps (the lr schedule of model/training/trainer.py:124); max_norm <= 0
        switches the clipping off"""
        if lr is not None: self.lr = float(lr)
        if betas is not None: self.betas = tuple(betas)
        if eps is not None: self.eps = float(eps)
        if max_norm is not None: self.max_norm = float(max_norm)
        if weight_decay is not None: self.weight_decay = float(weight_decay)
        if alpha is not None: self.alpha = float(alpha)
        if momentum is not None: self.momentum = float(momentum)
        self._invalidate_graphs()

    def set_cost(self, cost, class_weights=None):
        """The cost and the class weights of the masked loss -- of `step` (eager and captured), `step_ids`, `step_nhwc`,
        `step_boxes` and `step_prefetched`: `cost` as `msau_amd.plan.unet_cost` takes it (None or {"cost_name": "cross_entropy"}
        without weights: the masked CE, launch for launch), `class_weights` a sequence or tensor of n_class values (uploaded here) or
        None.  DESIGN.md 5d.  The cost's parameter and the workspace pointers are frozen into a captured sweep: the engine's graphs
        are dropped.  `step_unet*` / `step_kv` keep their own per-call `cost`.  Configuration, not state: `state_dict` does not
        hold it."""
        cost = unet_cost(cost)
        cw = None
        if class_weights is not None:
            cw = _device_class_weights(self, class_weights, self.model.n_class, self.model._flat.device)
        self._cost, self._cost_cw = cost, cw
        self._invalidate_graphs()

    @classmethod
    def from_opt_kwargs(cls, model: MSAUWrapper, opt_kwargs={}, **engine_kwargs) -> "TrainEngine":
        """The engine with the optimiser the reference's `get_optimizer(model, opt_kwargs)` builds (model/training/optimizer.py:
        RMSprop at 1e-3 by default, "momentum" = SGD with momentum 0.9, any other name Adam, `lr_decay_rate` handed over as weight
        decay) and no gradient clipping, as `Trainer.train` never clips.  Prints the reference's two lines.  `engine_kwargs`
        (process_group, use_graph, ...) go to the constructor and win over the mapped options."""
        from .training.optimizer import engine_options
        opt = engine_options(opt_kwargs)
        shown = opt.pop("shown")
        print(f"Optimizer: {shown[0]}")
        print(f"Learning Rate: {shown[1]}")
        return cls(model, **{**opt, **engine_kwargs})

    def _clip(self) -> float:
        """max_norm as the kernels take it: 0 = no clipping"""
        return float(self.max_norm) if self.max_norm is not None and self.max_norm > 0 else 0.0

    def _default_step(self) -> bool:
        """clip + Adam without weight decay: msau_clip_adam_step, the launch of the default engine and of bench.py"""
        return self.optimizer == "adam" and self.weight_decay == 0.0 and self._clip() > 0.0

    def _has_norm(self) -> bool:
        return self.optimizer == "adam" or self._clip() > 0.0

    def optim_launches(self):
        """[(key, algorithmic bytes)] of the optimiser launches this engine's step ends in, in order (the plan's boundary record
        states the default's: Plan._boundary_launches)"""
        nparam = sum(p.numel() for _, p in self.model._named)
        if self._default_step():
            return [("msau_clip_adam_step", nparam * 4 * 8)]             # g twice, p, m, v read; p, m, v written
        nbuf = len(OPTIM_BUFFERS[self.optimizer])
        out = [("msau_optim_step<sqsum>", nparam * 4)] if self._has_norm() else []
        return out + [(f"msau_optim_step<{self.optimizer}>", nparam * 4 * (2 + 2 * nbuf + 1))]    # g, p, state read; p, state written

    def _init_native_comm(self, group):
        """The gradient exchange through the C ABI (msau_allreduce_bucket over RCCL, csrc/comm.hip) when the process group is an
        RCCL one: rank 0 draws the communicator id, the group broadcasts it, every rank joins.  Then the all-reduce of each
        stage's bucket is a record of the native backward sequence (Plan.set_native_dp) -- no torch.distributed call, no
        Python between the launches.  gloo groups (CPU tests, several ranks on one card) and MSAU_DP_NATIVE=0 keep
        msau_amd/dp.py::GradSync."""
        import torch.distributed as dist
        # Opt-in (MSAU_DP_NATIVE=1) since round 4: the path has only ever run at world size 1 on the one-GPU boxes this tree is
        # measured on (tests/test_dp_gpu.py: bit-equal to the torch.distributed path there, where an all-reduce is the identity);
        # until a run with >= 2 RCCL ranks has shown the same, a multi-GPU job takes the GradSync path that the 2-rank tests cover.
        if not self.sync.active or self.use_graph or os.environ.get("MSAU_DP_NATIVE", "0") != "1":
            return
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend(group) != "nccl":
            return
        if not L.load().msau_comm_available():
            return
        import ctypes as C
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        ident = torch.zeros(128, dtype=torch.uint8, device=self.model._flat.device)
        if rank == 0:
            buf = (C.c_ubyte * 128)()
            L.call("msau_comm_unique_id", buf, 128)
            ident.copy_(torch.tensor(list(buf), dtype=torch.uint8))
        dist.broadcast(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = bytes(ident.cpu().tolist())
        comm = C.c_void_p()
        L.call("msau_comm_init", C.byref(comm), world, rank, raw, 128)
        self._comm = comm.value
        self._comm_stream = L.concurrent_stream(self.model._flat.device, index=1)
        weakref.finalize(self, L.load().msau_comm_destroy, self._comm)

    # -- pieces (each is a fixed launch sequence on the current stream) --
    def _fwd_bwd(self, plan: Plan, x, labels, ids=None, nhwc_ready=False, owner=None, nhwc_clean=False, loss_grads=None):
        plan.forward(self.model._flat, x, export=False, ids=ids, nhwc_ready=nhwc_ready, owner=owner, single_stream=self.use_graph,
                     nhwc_clean=nhwc_clean)
        # the engine's cost and class weights (set_cost): the default issues today's launches.  (step_unet: another loss, same sweeps)
        loss = plan.loss_grads(labels, self._cost, self._cost_cw) if loss_grads is None else loss_grads(plan)
        # MSAU_DP_BUCKETS=1: ONE all-reduce of the whole flat gradient after the backward instead of a bucket per stage
        # issued while the earlier stages' backward still runs (fewer launches and joins, no overlap)
        self._ar_native = False
        # the native sequence needs one bucket per backward segment + the end-conv tail (stage_buckets drops EMPTY buckets: then
        # the counts differ and the exchange stays with GradSync), and a profiled sweep runs its records one by one on one stream
        native = self._comm is not None and self.sync.active and plan.overlap_wgrad and L._profiler is None \
            and len(self.sync.buckets) == len(plan._bwd_segs) + 1
        if native:
            if getattr(plan, "_dp_flat", None) != self.flat_grad.data_ptr() or getattr(plan, "_dp_comm", None) != self._comm:
                plan.set_native_dp(self._comm, self._comm_stream, self.sync.buckets, self.flat_grad)
                plan._dp_comm = self._comm
            plan.backward(self.flat_grad, native_dp=True)      # stage buckets exchanged inside the native sequence, joined at its end
            self._ar_started = False
            self._ar_native = True
        elif self.sync.active and not self.use_graph and os.environ.get("MSAU_DP_BUCKETS", "stage") != "1":
            # bucket i of GradSync = [end convs, last stage, ..., stage 0]; a stage's bucket is reduced over RCCL as
            # soon as that stage's slab reduction is enqueued, while the earlier stages' backward still runs
            nb = self.model.num_blocks
            plan.backward(self.flat_grad, on_stage_done=lambda b, side: self.sync.start(nb - b, after=side))
            self._ar_started = True
        else:
            plan.backward(self.flat_grad, single_stream=self.use_graph)      # (a captured sweep stays on one stream: see _keep_graph)
            self._ar_started = False
        return loss

    def _optim(self):
        n = self.model._flat.numel()
        if self._default_step():
            b1, b2 = self.betas
            L.call("msau_clip_adam_step", torch.cuda.current_stream().cuda_stream, self.model._flat.data_ptr(),
                   self.flat_grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.state.data_ptr(),
                   self.adam_ws.data_ptr(), n, self.lr, b1, b2, self.eps, self.max_norm, 1.0 / self.world)
            return
        if self.optimizer == "adam":
            a, b, (c1, c2) = self.m, self.v.data_ptr(), self.betas
        elif self.optimizer == "rmsprop":
            a, b, c1, c2 = self.square_avg, None, self.alpha, 0.0
        else:
            a, b, c1, c2 = self.momentum_buffer, None, self.momentum, 0.0
        L.call("msau_optim_step", torch.cuda.current_stream().cuda_stream, OPTIMIZERS[self.optimizer], self.model._flat.data_ptr(),
               self.flat_grad.data_ptr(), a.data_ptr(), b, self.state.data_ptr(), self.adam_ws.data_ptr(), n, self.lr, c1, c2,
               self.eps, self.weight_decay, self._clip(), 1.0 / self.world, self._skip_arr, len(self._skip))

    def _allreduce(self):
        if self._ar_native:
            return                                       # already in the backward sequence (msau_run_ops_dp)
        if self.sync.active:
            if self._ar_started:
                self.sync.start(0)                       # the end-conv tail: final once every stage is done
            elif os.environ.get("MSAU_DP_BUCKETS", "stage") == "1":
                self.sync.start_whole()
            else:
                self.sync.start_all()
            self.sync.finish()

    def _step(self, plan: Plan, labels, x=None, **feed) -> torch.Tensor:
        """the tail of every eager step: both sweeps (`feed`: the keywords of `_fwd_bwd`), gradient exchange, optimiser -> the loss"""
        loss = self._fwd_bwd(plan, x, labels, **feed)
        self._allreduce()
        self._optim()
        return loss

    def _eager(self, name: str):
        """the entry points without a captured-graph form refuse first thing, before they read anything else of the engine"""
        if self.use_graph:
            raise RuntimeError(f"{name} is an eager path (use_graph=False)")

    def step(self, x: torch.Tensor, labels: torch.Tensor, sizes=None) -> torch.Tensor:
        """One optimisation step.  Returns the (local) loss as a 1-element device tensor (no host sync).
        `sizes` (ragged batch): CPU integer [B, 2] of every document's (h, w) at the origin of the canvas; the loss is then the
        mean of the per-document losses and the gradient the mean of the per-document gradients.  None: the dense batch."""
        x = x.contiguous().float()
        labels = labels.reshape(x.shape[0], x.shape[2], x.shape[3]).contiguous().long()
        if sizes is not None:
            sizes = self.model._check_sizes(x, sizes)
        plan = self.model._plan_for(x, training=True, ragged=sizes is not None)
        if not self.use_graph:
            plan.set_extents(sizes)
            return self._step(plan, labels, x)
        # The captured graphs hold the plan's buffer addresses: they are stored ON the plan (as predict_nhwc does), so
        # that an evicted / rebuilt plan can never be replayed through a stale graph.
        _bury_graphs()
        graphs = plan.__dict__.setdefault("_tgraphs", {})
        key = self._token
        cur = torch.cuda.current_stream()
        gs = self._gstream
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            plan.set_extents(sizes)              # (one graph per canvas: the extents buffer is refreshed before every replay)
            if key not in graphs:
                sx, sl = x.clone(), labels.clone()
                # warm up outside capture (hipFuncSetAttribute calls, lazy allocations)
                self._fwd_bwd(plan, sx, sl)
                torch.cuda.synchronize()
                g1 = _keep_graph(torch.cuda.CUDAGraph())
                with _capture_section():
                    with torch.cuda.graph(g1, stream=gs):
                        loss = self._fwd_bwd(plan, sx, sl)
                g2 = _keep_graph(torch.cuda.CUDAGraph())
                with _capture_section():
                    with torch.cuda.graph(g2, stream=gs):
                        self._optim()
                graphs[key] = (g1, g2, loss, sx, sl)
            g1, g2, loss, sx, sl = graphs[key]
            sx.copy_(x, non_blocking=True)
            sl.copy_(labels, non_blocking=True)
            g1.replay()
            self._allreduce()
            g2.replay()
        cur.wait_stream(gs)
        return loss

    def step_ids(self, ids: torch.Tensor, labels: torch.Tensor, sizes=None) -> torch.Tensor:
        """One optimisation step fed with the character-id mask int32 [B,H,W] (-1 or any id outside [0, channels) = empty
        pixel) instead of the dense one-hot float tensor: what `to_categorical` / the chargrid painter would have produced
        is painted straight into the NHWC input on the device -- 4 B per pixel cross the boundary instead
        of 4*C, and the 352 MB NCHW -> NHWC conversion of cfg 2 disappears.  Same kernels after that: bit-identical to
        `step(one_hot(ids), labels)`.  Eager only.
        `sizes` (ragged batch, msau_amd.data.ragged.pack_ids): CPU integer [B, 2] of every document's (h, w) at the origin of the
        canvas; ids and labels outside the documents are ignored, loss and gradient are those of `step(one_hot(ids), labels, sizes)`."""
        self._eager("step_ids")
        ids = self.model._check_ids(ids)
        B, H, W = ids.shape
        sizes = self.model._check_sizes_for(sizes, B, H, W)
        labels = labels.reshape(B, H, W).contiguous().long()
        plan = self.model._plan(B, H, W, ids.device, True, sizes)
        return self._step(plan, labels, ids=ids)

    def _class_weights(self, class_weights, n_class: int) -> Optional[torch.Tensor]:
        """the class weights on the device, uploaded again only when they change"""
        return _device_class_weights(self, class_weights, n_class, self.model._flat.device)

    def step_unet(self, ids: torch.Tensor, labels: torch.Tensor, aux_labels: torch.Tensor, sizes=None, class_weights=None,
                  stats=None, cost=None) -> torch.Tensor:
        """`step_ids` with the loss the reference trains the key-value model with (model/training/cost.py `UNetLoss`): cross entropy
        over EVERY pixel of a document, class 0 counted, 0.5 * final + 0.5 * auxiliary, each head against its OWN label map
        (`labels` for the last stage, `aux_labels` for the auxiliary one; int64 [B,H,W]), optional `class_weights` (a sequence or
        tensor of n_class floats).  Returns the 3-float device tensor (total, final, auxiliary), no host sync.
        `sizes` as `step_ids` takes them: ids and labels outside the documents are ignored, every document computes what it
        computes alone and loss and gradient are the means over the documents.  Without `sizes` every sample is its whole canvas: at
        B = 1 exactly UNetLoss.  Backward, gradient exchange and optimiser are those of `step_ids`.  Eager only.
        `stats`: a pair of device tensors (fp32 [B, 2], int32 [B, 2, 2]); the rows of `MSAUWrapper.eval_unet` -- per document the
        losses and (labelled, correct) of this step's forward, the training accuracy of the reference's epoch print -- are then
        written into it by one more launch between the forward and the loss kernel.  None: no such launch.
        `cost` (msau_amd.plan.unet_cost checks it; ValueError for an unknown name or a bad parameter): None or
        {"cost_name": "cross_entropy"} is the loss above; {"cost_name": "focal", "gamma": 2.0} and {"cost_name": "dice", "smooth": 1.0}
        train the focal and the soft Dice loss under the same rules, and `stats` then holds that loss."""
        self._eager("step_unet")
        cost = unet_cost(cost)
        cw = self._class_weights(class_weights, self.model.n_class)
        ids = self.model._check_ids(ids)
        B, H, W = ids.shape
        sizes = self.model._check_sizes_for(sizes, B, H, W)
        plan = self.model._plan(B, H, W, ids.device, True, sizes)
        return self._step_unet(plan, labels, aux_labels, cw, stats, cost, ids=ids)

    def _step_unet(self, plan: Plan, labels, aux_labels, cw, stats, cost, **feed) -> torch.Tensor:
        """the tail `step_unet` and `step_unet_nhwc` share: the label maps as the loss kernel takes them, UNetLoss, `_step`"""
        B, H, W = plan.B, plan.H, plan.W
        labels = labels.reshape(B, H, W).contiguous().long()
        aux_labels = aux_labels.reshape(B, H, W).contiguous().long() if plan.aux is not None else None
        if stats is None:
            loss_grads = lambda p: p.loss_grads_unet(labels, aux_labels, cw, cost=cost)
        else:
            def loss_grads(p):
                p.eval_unet(labels, aux_labels, cw, out=stats, cost=cost)
                return p.loss_grads_unet(labels, aux_labels, cw, cost=cost)
        return self._step(plan, None, loss_grads=loss_grads, **feed)

    def step_unet_nhwc(self, grid: torch.Tensor, labels: torch.Tensor, aux_labels: torch.Tensor, sizes=None, class_weights=None,
                       stats=None, cost=None) -> torch.Tensor:
        """`step_unet` for an input that is ALREADY on the device in the kernels' layout ([B][H][W][Cs], storage dtype, as
        `step_nhwc` takes it): a one-hot, multi-hot or zero-hot grid, e.g. what the warp kernel leaves (msau_kv_warp_train).  When
        `grid` is the plan's own input buffer nothing is copied; otherwise one device copy.  `labels`,
        `aux_labels`, `sizes`, `class_weights`, `stats` and `cost` as in `step_unet`; with `sizes` the buffer is zeroed outside the documents
        before the sweep.  On the one-hot grid of an id canvas the step is bit-identical to `step_unet` on the ids.  Eager only."""
        self._eager("step_unet_nhwc")
        cost = unet_cost(cost)
        cw = self._class_weights(class_weights, self.model.n_class)
        B, H, W, _ = grid.shape
        sizes = self.model._check_sizes_for(sizes, B, H, W)
        plan = self.model._plan(B, H, W, grid.device, True, sizes)
        buf = plan.input_nhwc
        if tuple(grid.shape) != tuple(buf.shape) or grid.dtype != buf.dtype:
            raise ValueError(f"step_unet_nhwc wants {tuple(buf.shape)} {buf.dtype} (channels padded to a multiple of 8), got "
                             f"{tuple(grid.shape)} {grid.dtype}")
        if grid.data_ptr() != buf.data_ptr():
            buf.copy_(grid)
        return self._step_unet(plan, labels, aux_labels, cw, stats, cost, nhwc_ready=True)

    def step_kv(self, tables, class_weights=None, round_to: int = 16, stats=None, cost=None) -> torch.Tensor:
        """One optimisation step on a group of key-value documents given as their training tables
        (msau_amd.training.kv_data.train_table / KVTrainBatches): one upload of the packed tables, one launch that paints the id
        canvas and both label canvases (msau_kv_paint_train), then `step_unet` on them with the documents' sizes.  No per-pixel
        array is built on the host and nothing waits for the device -- except for a document whose table is not `ok`, which is
        painted on the host and uploaded (kv_data.STATS counts them).  `stats` and `cost` as in `step_unet`.
        When a table carries a `warp` (the generator's affine or rotation augmentation: kv_warp.py, `KVTrainBatches(kwargs_dat=...)`)
        the painted canvases are resampled on the device: paint -> msau_kv_warp_train, which writes the multi-hot input straight
        into the plan's input buffer and the two warped label maps -> the tail of `step_unet_nhwc`, on the warped sizes and their
        canvas (rounded up to `round_to`).  Tables without a warp in such a group take the identity.  The launch leaves one flag
        per document, which the host reads before the sweep (the one wait of this path); a flagged document is warped by
        `kv_warp.warp_host` and uploaded (kv_data.STATS["host_warped"]).  A group without warps takes the path above, launch for
        launch.  A group whose warps are `kv_warp.Elastic` (the generator's elastic augmentation, `KVTrainBatches(...,
        imresize="pillow")`) takes the same route through msau_kv_elastic_train, tables without a warp as `identity_elastic`, a
        flagged document through `kv_warp.elastic_host`; a group that mixes the two kinds is a ValueError."""
        self._eager("step_kv")
        cost = unet_cost(cost)
        from .training import kv_data, kv_warp
        elastic = any(isinstance(t.warp, kv_warp.Elastic) for t in tables)
        if elastic and any(isinstance(t.warp, kv_warp.Warp) for t in tables):         # (on the host, before anything is launched)
            raise ValueError("step_kv: a group mixes affine / rotation warps with elastic ones; a group takes one kind (and tables without)")
        dev = self.model._flat.device
        ids, labels, aux_labels, sizes = kv_data.paint_train_device(tables, round_to=round_to, device=dev)
        if all(t.warp is None for t in tables):
            return self.step_unet(ids, labels, aux_labels, sizes=sizes, class_weights=class_weights, stats=stats, cost=cost)
        m = self.model
        cw = self._class_weights(class_weights, m.n_class)
        identity, launch, upload = ((kv_warp.identity_elastic, kv_warp.elastic_train_device, kv_warp.upload_host_elastic) if elastic else
                                    (kv_warp.identity_warp, kv_warp.warp_train_device, kv_warp.upload_host_warp))
        warps = [identity(t.shape) if t.warp is None else t.warp for t in tables]
        wsizes, (Ho, Wo) = kv_warp.warped_canvas(warps, round_to=round_to)
        B = len(tables)
        plan = m._plan(B, Ho, Wo, dev, True, m._check_sizes_for(torch.from_numpy(wsizes), B, Ho, Wo))
        grid = plan.input_nhwc
        wl, wa, flags = launch(ids, labels, aux_labels, sizes, warps, grid, m.channels, m.n_class, plan.dtype)
        for b in torch.nonzero(flags.cpu()).reshape(-1).tolist():
            upload(b, tables[b], warps[b], grid, wl, wa, m.channels, m.n_class)
            kv_data.STATS["host_warped"] += 1
        # (the kernel and the host warp leave zeros outside the warped extents: nothing to clear)
        return self._step_unet(plan, wl, wa, cw, stats, cost, nhwc_ready=True, nhwc_clean=True)

    def input_nhwc(self, B: int, H: int, W: int) -> torch.Tensor:
        """The training plan's own input buffer for this shape, [B][H][W][Cs] in the storage dtype: the zero-copy target of
        a device-side producer (msau_amd.data.raster: `rasterize(..., out=...)`, `rasterize_dense(..., out=...)`)."""
        return self.model._plan_for_shape(B, H, W, self.model._flat.device, True).input_nhwc

    def step_nhwc(self, grid: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """One optimisation step on a chargrid that is ALREADY on the device in the kernels' layout ([B][H][W][Cs], storage
        dtype) -- what the device painters produce (data_generator_funsd_bert.py:64-93,240).  When `grid` is
        the plan's own buffer (`input_nhwc(B, H, W)`) nothing is copied or converted; otherwise one device copy.  `step(x, l)`
        on the same grid as fp32 NCHW spends a quarter of the 768-channel step (cfg 4) converting 4.2 GB: identical result."""
        self._eager("step_nhwc")
        B, H, W, Cs = grid.shape
        plan = self.model._plan_for_shape(B, H, W, grid.device, True)
        buf = plan.input_nhwc
        if tuple(grid.shape) != tuple(buf.shape) or grid.dtype != buf.dtype:
            raise ValueError(f"step_nhwc wants {tuple(buf.shape)} {buf.dtype} (channels padded to a multiple of 8), got {tuple(grid.shape)} {grid.dtype}")
        if grid.data_ptr() != buf.data_ptr():
            buf.copy_(grid)
        labels = labels.reshape(B, H, W).contiguous().long()
        return self._step(plan, labels, nhwc_ready=True)

    def step_boxes(self, grid_boxes, label_boxes, B: int, H: int, W: int, feats=None, sizes=None) -> torch.Tensor:
        """One optimisation step from BOX LISTS (int32 [n][6] = sample, y0, y1, x0, x1, value; msau_amd/data/raster.py): the
        one-hot grid (feats None: value = character id) or the dense embedding grid (feats fp32 [n_vectors][channels]: value
        = row of feats) and the label mask are painted on the device, the grid straight into the plan's input buffer.
        Only the lists (KBs) and the feature table cross PCIe.  Arguments may be numpy arrays or device tensors.
        `sizes` (ragged batch, msau_amd.data.ragged.pack_boxes): CPU integer [B, 2] of every document's (h, w) at the origin of the
        H x W canvas, every document's boxes in its own coordinates.  Each box is clipped at its own document's edge, the loss is
        the mean of the documents' losses as `step(x, labels, sizes)` defines it, and with `feats` the grid is still never
        painted (the box-list instance of the first conv implements the extents).  Eager only."""
        self._eager("step_boxes")
        m = self.model
        sizes = m._check_sizes_for(sizes, B, H, W)
        plan = m._plan(B, H, W, m._flat.device, True, sizes)
        feed, labels = m._paint_boxes(plan, grid_boxes, label_boxes, feats)
        return self._step(plan, labels, **feed)

    def prefetch_boxes(self, grid_boxes, label_boxes, B: int, H: int, W: int, feats=None, sizes=None):
        """Paint the NEXT batch (arguments as `step_boxes`) while the current step runs: the grid goes into the input buffer the
        current step does not read (the plan keeps two), on the plan's side stream -- idle during the forward sweep, which is
        when the painter's store (2.1 GB per batch at 768 channels) is absorbed.  `step_prefetched()` then trains on it.  The
        data-loader counterpart of the reference's generator thread (data_generator_funsd_bert.py:216-240)."""
        self._eager("prefetch_boxes")
        if sizes is not None:
            raise NotImplementedError("prefetch_boxes paints dense batches only: a ragged batch (sizes=...) goes through "
                                      "step_boxes(..., sizes=sizes)")
        plan = self.model._plan_for_shape(B, H, W, self.model._flat.device, True)
        q = self._prefetched
        if len(q) >= 2:
            # the plan keeps TWO input buffers: a third batch would be painted over one that is still queued, unread
            raise RuntimeError("prefetch_boxes: two batches are already queued (the plan has two input buffers); call "
                               "step_prefetched() before painting another one")
        k = (q[-1][1] + 1) % 2 if q else (self._pf_last + 1) % 2
        buf = plan.input_buffer(k)
        cur = torch.cuda.current_stream()
        if plan._side is None:
            plan._side = L.concurrent_stream(plan.device)
        side = plan._side
        side.wait_stream(cur)                    # the buffer's last readers (two steps back) are behind everything enqueued so far
        with torch.cuda.stream(side):
            _, labels = self.model._paint_boxes(plan, grid_boxes, label_boxes, feats, out=buf)
            ev = torch.cuda.Event()
            ev.record(side)
        labels.record_stream(cur)
        q.append((plan, k, labels, ev))

    def step_prefetched(self) -> torch.Tensor:
        """One optimisation step on the oldest batch `prefetch_boxes` painted."""
        plan, k, labels, ev = self._prefetched.pop(0)
        self._pf_last = k
        torch.cuda.current_stream().wait_event(ev)
        plan.use_input(k)
        return self._step(plan, labels, nhwc_ready=True)

    @property
    def grad_norm(self) -> torch.Tensor:
        if not self._has_norm():
            raise RuntimeError(f"grad_norm: {self.optimizer} without clipping (max_norm {self.max_norm}) is one launch that never "
                               f"computes the gradient's norm; build the engine with max_norm > 0 to have it")
        return self.state[1]

    # -- optimiser state (resume): the counterpart of torch.optim.*.state_dict() for the flat buffers --
    def _buffers(self):
        return {"adam": (self.m, self.v), "rmsprop": (self.square_avg,), "momentum": (self.momentum_buffer,)}[self.optimizer]

    def state_dict(self) -> dict:
        """Adam: {"engine": 1, "step", "exp_avg", "exp_avg_sq" (flat fp32, the model's parameter order), hyper-parameters}, plus
        "weight_decay" when there is one.  RMSprop / momentum SGD: "optimizer": "rmsprop" / "momentum" as well, the buffer under
        torch's name ("square_avg" / "momentum_buffer"), "alpha" / "momentum", "weight_decay".  max_norm 0.0: no clipping."""
        sd = {"engine": 1, "step": int(round(float(self.state[0])))}
        for name, buf in zip(OPTIM_BUFFERS[self.optimizer], self._buffers()):
            sd[name] = buf.detach().clone()
        sd["lr"] = self.lr
        if self.optimizer == "adam":
            sd.update(betas=tuple(self.betas), eps=self.eps, max_norm=self.max_norm if self.max_norm is not None else 0.0,
                      numel=int(self.m.numel()))
            if self.weight_decay != 0.0:
                sd["weight_decay"] = self.weight_decay
            return sd
        sd.update(optimizer=self.optimizer, eps=self.eps, weight_decay=self.weight_decay, max_norm=self._clip(),
                  numel=int(self.flat_grad.numel()))
        sd["alpha" if self.optimizer == "rmsprop" else "momentum"] = self.alpha if self.optimizer == "rmsprop" else self.momentum
        return sd

    def load_state_dict(self, sd: dict):
        """Accepts `TrainEngine.state_dict()` or a `torch.optim.{Adam,RMSprop,SGD}.state_dict()` over the model's parameters in
        registration order (what the reference's `save_checkpoint` stores: utils/io_utils.py:83-105); parameters the optimiser
        never stepped (the dead last-stage attention) have no entry and keep zero state.  ValueError when the state is
        another optimiser's than this engine's."""
        bufs = self._buffers()
        if sd.get("engine") == 1:
            have = sd.get("optimizer", "adam")
            if have != self.optimizer:
                raise ValueError(f"optimizer state is {have}'s, the engine runs {self.optimizer}")
            if int(sd["numel"]) != self.flat_grad.numel():
                raise ValueError(f"optimizer state is for {sd['numel']} parameters, the model has {self.flat_grad.numel()}")
            for name, buf in zip(OPTIM_BUFFERS[self.optimizer], bufs):
                buf.copy_(sd[name])
            self.state.zero_()
            self.state[0] = float(sd["step"])
            self.lr, self.eps = float(sd["lr"]), float(sd["eps"])
            if self.optimizer == "adam":
                self.betas = tuple(sd["betas"])
            self.max_norm = float(sd.get("max_norm", self.max_norm))
            self.weight_decay = float(sd.get("weight_decay", 0.0))
            self.alpha, self.momentum = float(sd.get("alpha", self.alpha)), float(sd.get("momentum", self.momentum))
            self._invalidate_graphs()
            return
        named = [(k, p.numel()) for k, p in self.model._named if p.requires_grad]
        step, flats, g0 = torch_optim_state_to_flat(sd, named, self.model._poff, self.flat_grad.numel(), self.optimizer)
        for buf, flat in zip(bufs, flats):
            buf.copy_(flat)
        self.state.zero_()
        self.state[0] = float(step)
        self.lr, self.weight_decay = float(g0["lr"]), float(g0.get("weight_decay", 0.0))
        if self.optimizer == "adam":
            self.betas, self.eps = tuple(g0["betas"]), float(g0["eps"])
        elif self.optimizer == "rmsprop":
            self.alpha, self.eps = float(g0["alpha"]), float(g0["eps"])
        else:
            self.momentum = float(g0["momentum"])
        self._invalidate_graphs()
