"""The host side of the loss kernels (csrc/loss.hip), stated once: `LossSite`, the loss end of a Plan -- the checks of its four
entry points, their buffers, their launches and their accounting -- and `nchw_loss`, the NCHW adapter of the autograd functions
(msau_amd/model.py, msau_amd/training/cost.py).  The masked loss and its costs: DESIGN.md 5d; UNetLoss: 5e."""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib as L
from .plan import Launch, UnetCost, _env_on, _ptr, _ru, unet_cost

NCHW_HIST_K = 4         # rows per sample of the label histogram the autograd functions take


def cost_hist_k(B: int, dice: bool) -> int:
    """rows per document of the label histograms a cost takes (msau_label_hist's K).  Dice: K is also the slabs per document of
    its reduction pass.  Two workgroups per compute unit were the best of three choices in ONE measurement: B = 16 on 320 x 256,
    256 compute units (profiles/unet_cost.md: K = 16 / 32 / 64 -> 163 / 146 / 150 us in bf16).  Any other B or canvas size is
    unmeasured, and what bounds that pass has not been profiled."""
    return max(1, min(32, 512 // B)) if dice else max(1, min(16, 256 // B))


class LossSite:
    """The loss end of a plan: what `Plan.loss_grads`, `loss_grads_unet`, `eval_masked` and `eval_unet` forward to, and the launch
    lists that state them.  Built by `Plan._finish` before the boundary launches are stated (they ask `masked_launches` for the
    default rows); a training plan gets the buffers of the default masked CE there, every other buffer comes at its first use."""

    def __init__(self, plan):
        self.p = plan
        self._bufs = {}
        self._cu_count = None
        if plan.training:
            # label counts: a sample spread over K workgroups (msau_label_counts_split), the K integers added up by the CE launch
            self.counts_k = max(1, min(16, 256 // plan.B)) if plan.B <= 1024 and _env_on("MSAU_LABEL_SPLIT") else 1
            self.counts = self.buf("counts", None, plan.B * self.counts_k, torch.int32)
            self.ce_ws = self._ws("msau_ce_ws_floats", torch.float32, plan.B * plan.H * plan.W)
            self.ce_multi_ws = self._ws("msau_ce_multi_ws_floats", torch.float32, plan.B * plan.H * plan.W)
            self.loss_buf = self.buf("loss_buf", None, 1, torch.float32)

    # ---- buffers ------------------------------------------------------------------------------
    def buf(self, name: str, key, n, dtype) -> torch.Tensor:
        """the zero-initialised buffer `name`, made at its first use and again only when `key` -- what its size function takes
        beyond the plan's shape -- changes: a captured sweep freezes these pointers, and `TrainEngine.set_cost` drops the graphs
        when the cost changes.  `n`: the shape, or a function that gives it (asked only when the buffer is made)."""
        kept = self._bufs.get(name)
        if kept is None or kept[0] != key:
            kept = self._bufs[name] = (key, torch.zeros(n() if callable(n) else n, dtype=dtype, device=self.p.device))
        return kept[1]

    def _ws(self, size_fn: str, dtype, *args) -> torch.Tensor:
        """the workspace that the library's `size_fn` (<entry point>_ws_floats / _ws_bytes) sizes, keyed by what that function takes"""
        return self.buf(size_fn, args, lambda: int(getattr(L.load(), size_fn)(*args)), dtype)

    def _hist(self, name: str, lead: tuple, K: int) -> int:
        """pointer of the histogram buffer [*lead, B, K', C] with K' >= K (it grows once, when a plan's cost changes to Dice)"""
        kept = self._bufs.get(name)
        K = max(K, kept[0]) if kept is not None else K
        return self.buf(name, K, lead + (self.p.B, K, self.p.logits.C), torch.int32).data_ptr()

    @property
    def masked_loss3(self) -> torch.Tensor:
        """(total, final, auxiliary) of `loss_grads` under a cost or class weights"""
        return self.buf("masked_loss3", None, 3, torch.float32)

    # ---- checks -------------------------------------------------------------------------------
    def check(self, maps, class_w: Optional[torch.Tensor], heads: bool = True):
        """one call's label maps (one per head that has its own), the heads' shapes and the class weights"""
        p = self.p
        lg, ax = p.logits, p.aux
        for t in maps:
            assert t is not None and t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == (p.B, p.H, p.W)
        if heads:
            assert ax is None or (ax.C, ax.Cs, ax.H, ax.W) == (lg.C, lg.Cs, lg.H, lg.W), "the auxiliary head must have the final head's shape"
            assert (lg.H, lg.W) == (p.H, p.W)
        if class_w is not None:
            assert class_w.dtype == torch.float32 and class_w.is_contiguous() and class_w.numel() == lg.C and class_w.device == lg.data.device

    def doc_rows(self, out):
        """the (doc_loss fp32 [B, 2], doc_counts int32 [B, 2, 2]) pair of an eval call: fresh when `out` is None, else checked"""
        p = self.p
        if out is None:
            out = (torch.empty((p.B, 2), dtype=torch.float32, device=p.device),
                   torch.empty((p.B, 2, 2), dtype=torch.int32, device=p.device))
        doc_loss, doc_counts = out
        assert doc_loss.dtype == torch.float32 and doc_loss.is_contiguous() and tuple(doc_loss.shape) == (p.B, 2) \
            and doc_counts.dtype == torch.int32 and doc_counts.is_contiguous() and tuple(doc_counts.shape) == (p.B, 2, 2) \
            and doc_loss.device == doc_counts.device == p.logits.data.device, "stats: (fp32 [B, 2], int32 [B, 2, 2]) on the model's device"
        return doc_loss, doc_counts

    # ---- launches -----------------------------------------------------------------------------
    def hist_k(self, dice: bool) -> int:
        return cost_hist_k(self.p.B, dice)

    def eval_k(self) -> int:
        """workgroups per document of `eval_unet`: enough to give every compute unit two workgroups, never more than the smallest
        document has rows (more would only be empty slabs), at most the kernel's 256.  Reasoned, not measured."""
        p = self.p
        if self._cu_count is None:
            self._cu_count = int(torch.cuda.get_device_properties(p.device).multi_processor_count)
        rows = int(p._ext_host[0, :, 0].min()) if p.ragged else p.H      # the pinned host copy of set_extents: no sync
        return max(1, min(256, rows, -(-2 * self._cu_count // p.B)))

    def _call(self, entry: str, cost: Optional[UnetCost], maps, class_w, *rest):
        """one launch of a loss family (include/msau_hip.h): [kind, param,] both heads' logits, the label map of each head (UNetLoss)
        or of both (masked), the extents (level 0: the documents' own (h, w)), the class weights, `rest`, the shape.  An entry
        point with a cost differs from the one without by the two leading arguments alone."""
        p = self.p
        lg, ax = p.logits, p.aux
        L.call(entry, p._stream(), p.dtype, *(() if cost is None else cost), lg.data.data_ptr(), _ptr(ax.data) if ax is not None else None,
               *(_ptr(t) for t in maps), p.extents.data_ptr() if p.ragged else None, _ptr(class_w), *rest, p.B, p.H, p.W, lg.C, lg.Cs)

    def _grads(self, entry: str, cost, maps, class_w, hist_name: str, lead: tuple, loss3: torch.Tensor) -> torch.Tensor:
        """a loss with its gradient, both heads in one launch of `entry`; class weights or Dice: the label histogram of every map first"""
        p = self.p
        lg, ax = p.logits, p.aux
        dice = cost is not None and cost.kind == L.COST_DICE
        K, hist = self.hist_k(dice), None
        if class_w is not None or dice:
            hist = self._hist(hist_name, lead, K)
            for t, lab in enumerate(m for m in maps if m is not None):
                L.call("msau_label_hist", p._stream(), lab.data_ptr(), p.extents.data_ptr() if p.ragged else None,
                       hist + 4 * t * p.B * K * lg.C, p.B, p.H, p.W, lg.C, K)
        ws = self._ws(entry + "_ws_floats", torch.float32, *((p.B * p.H * p.W,) if cost is None else (cost.kind, p.B, p.H, p.W, lg.C)))
        self._call(entry, cost, maps, class_w, hist, K, lg.grad.data_ptr(), _ptr(ax.grad) if ax is not None else None,
                   loss3.data_ptr(), ws.data_ptr())
        return loss3

    def _eval(self, entry: str, cost, maps, class_w, out):
        """the rows of an eval call; its workspace is sized for the largest K: the extents, and with them K, change per batch"""
        p = self.p
        doc_loss, doc_counts = self.doc_rows(out)
        ws = self._ws(entry + "_ws_bytes", torch.uint8, *((p.B, 256) if cost is None else (cost.kind, p.B, 256, p.logits.C)))
        self._call(entry, cost, maps, class_w, self.eval_k(), doc_loss.data_ptr(), doc_counts.data_ptr(), ws.data_ptr())
        return doc_loss, doc_counts

    def _unet_maps(self, labels, aux_labels, class_w) -> tuple:
        """UNetLoss, checked: each head has its own label map; without an auxiliary head `aux_labels` is not looked at"""
        two = self.p.aux is not None
        self.check((labels, aux_labels) if two else (labels,), class_w)
        return labels, aux_labels if two else None

    def loss_grads(self, labels: torch.Tensor, cost=None, class_w: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Masked CE (model/model.py:446-459, batch rule SURVEY 8e) fused with its gradient: writes d(logits), d(aux)
        in place and returns the loss as a 1-element device tensor.  One launch for final + aux.
        `cost` (`unet_cost`) and `class_w` (fp32 [n_class] on the device): the masked loss under the focal or the soft Dice cost and
        with class weights (msau_masked_cost, which reads the extents of a ragged plan itself: whatever the label canvas
        holds outside the documents is ignored).  The three values (total, final, auxiliary) stay readable as `masked_loss3`, the
        total is returned.  With neither -- also with "cross_entropy" by name -- the launches are those below, unchanged."""
        p = self.p
        self.check((labels,), None, heads=False)
        cost = unet_cost(cost)
        if cost is not None or class_w is not None:
            self.check((), class_w)
            cost = cost or UnetCost(L.COST_CE, 0.0)
            return self._grads("msau_masked_cost", cost, (labels,), class_w, "masked_hist", (), self.masked_loss3)[:1]
        s = p._stream()
        HW = p.H * p.W
        if p.ragged:                                     # the label canvas: 0 (= not counted) outside the documents
            canvas = self.buf("labels", None, labels.shape, labels.dtype)
            p._zero_outside(labels, canvas, 1, p.H, p.W, 8)
            labels = canvas
        lg, ax = p.logits, p.aux
        multi = lg.Cs <= 16 and p.B * HW < (1 << 31) and (ax is None or (ax.C, ax.Cs) == (lg.C, lg.Cs)) and _env_on("MSAU_CE_MULTI")
        K = self.counts_k if multi else 1
        if K > 1:
            L.call("msau_label_counts_split", s, labels.data_ptr(), self.counts.data_ptr(), p.B, HW, K, key="msau_label_counts")
        else:
            L.call("msau_label_counts", s, labels.data_ptr(), self.counts.data_ptr(), p.B, HW)
        if multi:
            L.call("msau_masked_ce_multi", s, p.dtype, lg.data.data_ptr(), _ptr(ax.data) if ax is not None else None,
                   labels.data_ptr(), self.counts.data_ptr(), lg.grad.data_ptr(), _ptr(ax.grad) if ax is not None else None,
                   self.loss_buf.data_ptr(), self.ce_multi_ws.data_ptr(), p.B, HW, lg.C, lg.Cs, 1.0 / p.B, K)
            return self.loss_buf
        self.loss_buf.zero_()
        for act in (lg, ax):
            if act is None:
                continue
            L.call("msau_masked_ce", s, p.dtype, act.data.data_ptr(), labels.data_ptr(), self.counts.data_ptr(),
                   act.grad.data_ptr(), self.loss_buf.data_ptr(), self.ce_ws.data_ptr(), p.B, HW, act.C, act.Cs, 1.0 / p.B)
        return self.loss_buf

    def loss_grads_unet(self, labels: torch.Tensor, aux_labels: Optional[torch.Tensor], class_w: Optional[torch.Tensor] = None,
                        cost=None) -> torch.Tensor:
        """UNetLoss (model/training/cost.py:35-65: CE over every pixel, class 0 counted, 0.5 final + 0.5 auxiliary, optional class
        weights) fused with its gradient, under the ragged rule: every document computes what it computes alone, the batch is the
        mean of the documents.  `labels` / `aux_labels` int64 [B,H,W]: each head has its own map; the kernel reads the extents
        itself, so the canvases are not copied and whatever they hold outside the documents is ignored.  `class_w`: fp32 [n_class]
        on the device; only then the per-document class histograms are taken (one launch per head).  Writes d(logits), d(aux) in
        place and returns the plan's 3-float buffer (total, final, auxiliary).
        `cost` (`unet_cost`: None, a dict such as {"cost_name": "focal", "gamma": 2.0} or {"cost_name": "dice", "smooth": 1.0}): the
        focal or the soft Dice loss under the same rules (msau_unet_cost; Dice always takes the histograms).  None or
        "cross_entropy": msau_unet_ce, launch for launch."""
        cost = unet_cost(cost)
        return self._grads("msau_unet_ce" if cost is None else "msau_unet_cost", cost, self._unet_maps(labels, aux_labels, class_w),
                           class_w, "unet_hist", (2,), self.buf("unet_loss", None, 3, torch.float32))

    def eval_masked(self, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None, out=None, cost=None):
        """The masked loss and the accuracy counts per document, forward only (msau_masked_cost_eval): the counterpart of
        `eval_unet` for the loss of `loss_grads` -- after `forward(export=False)` on a forward-only plan, on the logits both heads
        left in the plan, both against `labels` (int64 [B,H,W]; the kernel reads the extents itself).  `class_w` and `cost` as
        `loss_grads` takes them; None: the masked CE's per-document loss.  -> (doc_loss fp32 [B, 2], doc_counts int32 [B, 2, 2]) on
        the device, as `eval_unet` returns them; `out`: a pair of such tensors to write.  No gradient buffer is touched and nothing
        waits for the device."""
        cost = unet_cost(cost) or UnetCost(L.COST_CE, 0.0)
        self.check((labels,), class_w)
        return self._eval("msau_masked_cost_eval", cost, (labels,), class_w, out)

    def eval_unet(self, labels: torch.Tensor, aux_labels: Optional[torch.Tensor], class_w: Optional[torch.Tensor] = None, out=None,
                  cost=None):
        """UNetLoss and the reference's accuracy per document, forward only (msau_unet_eval): after `forward(export=False)` on a
        forward-only plan, on the logits both heads left in the plan (`TrainEngine.step_unet(stats=...)` calls it on the training
        plan's, between the forward and the loss kernel).  `labels` / `aux_labels` / `class_w` as `loss_grads_unet` takes
        them; the kernel reads the extents itself.  -> (doc_loss fp32 [B, 2], doc_counts int32 [B, 2, 2]) on the device, head 0 =
        final, head 1 = auxiliary, counts = (labelled, correct); `out`: a pair of such tensors to write instead of fresh ones.  No
        gradient buffer is touched and nothing waits for the device.  `cost` as `loss_grads_unet` takes it: doc_loss is then the
        document's loss under that cost (msau_unet_cost_eval), the counts are unchanged."""
        cost = unet_cost(cost)
        return self._eval("msau_unet_eval" if cost is None else "msau_unet_cost_eval", cost, self._unet_maps(labels, aux_labels, class_w),
                          class_w, out)

    # ---- accounting ---------------------------------------------------------------------------
    def _bytes(self, label_reads: int, passes: int) -> int:
        """algorithmic bytes of one sweep over the canvas: per pixel `label_reads` int64 labels and, per head, `passes` times its
        stored logits (a read of the logits and a write of the gradient are one pass each)"""
        p = self.p
        nl, esz = 2 if p.aux is not None else 1, 4 if p.dtype == L.F32 else 2
        return p.B * p.H * p.W * (8 * label_reads + nl * passes * p.logits.Cs * esz)

    def _row(self, key: str, label_reads: int, passes: int, more: int = 0) -> Launch:
        return Launch(0, None, key, self._bytes(label_reads, passes) + more)

    def masked_launches(self, weighted: bool, cost=None) -> List[Launch]:
        """the launches of `loss_grads(labels, cost, class_w)`, stated as `unet_launches` states those of `loss_grads_unet`: key and
        algorithmic bytes.  The default (no cost or "cross_entropy", no weights) is what `Plan._boundary_launches` takes from here:
        the label counts and the masked CE.  Anything else is msau_masked_cost: the label and both heads' logits read and both
        gradients written; class weights or Dice put msau_label_hist in front (one launch: one label map), otherwise the call
        counts the labelled pixels itself (the labels once more); Dice reads label and logits once more (the reduction behind its
        gradient pass)."""
        cost = unet_cost(cost)
        if cost is None and not weighted:
            multi = self.p.logits.Cs <= 16
            return [self._row("msau_label_counts", 1, 0), self._row("msau_masked_ce_multi" if multi else "msau_masked_ce", 1, 2)]
        dice = cost is not None and cost.kind == L.COST_DICE
        extra = self._bytes(1, 1) if dice else 0 if weighted else self._bytes(1, 0)
        return [self._row("msau_label_hist", 1, 0)] * (1 if weighted or dice else 0) + [self._row("msau_masked_cost", 1, 2, extra)]

    def unet_launches(self, weighted: bool, cost=None) -> List[Launch]:
        """the launches of `loss_grads_unet`, stated as `masked_launches` states those of `loss_grads` (which they replace in a
        key-value training step): key and algorithmic bytes, for the step's accounting and a profiler's attribution.  `cost` as
        `loss_grads_unet` takes it: the focal loss moves the cross entropy's bytes under its own key; the Dice loss always takes
        the histograms and reads label and logits once more (the reduction behind its gradient pass)."""
        cost = unet_cost(cost)
        nl, dice = 2 if self.p.aux is not None else 1, cost is not None and cost.kind == L.COST_DICE
        return [self._row("msau_label_hist", 1, 0)] * (nl if weighted or dice else 0) + \
            [self._row("msau_unet_ce" if cost is None else "msau_unet_cost", nl, 2, self._bytes(nl, 1) if dice else 0)]

    def unet_eval_launches(self, cost=None) -> List[Launch]:
        """the launch of `eval_unet`, stated as `unet_launches` states those of `loss_grads_unet`: key and algorithmic bytes (per head
        the int64 label and the pixel's stored logits, read once; the K partial rows and the finish launch are noise beside them).
        `cost` as `eval_unet` takes it: Dice reads both once more and the labels a third time (its own histograms)."""
        cost = unet_cost(cost)
        nl = 2 if self.p.aux is not None else 1
        more = self._bytes(2 * nl, 1) if cost is not None and cost.kind == L.COST_DICE else 0
        return [self._row("msau_unet_eval" if cost is None else "msau_unet_cost_eval", nl, 1, more)]


def nchw_loss(heads, label: torch.Tensor, kernel, hist: bool = False) -> List[torch.Tensor]:
    """The NCHW adapter of the autograd functions: `heads` (one or two NCHW logits of one shape) become fp32 NHWC copies with the
    channels rounded up to 8, `kernel(nhwc, dn, label, hist, B, H, W, C, Cs, stream)` -- the one call that differs per function --
    reads them and writes the gradient buffers `dn` (both lists of device pointers, one per head), which come back as NCHW fp32.
    `label`: anything with B*H*W class indices; the kernel gets the pointer of its int64 [B, H, W] form.  `hist`: take the label
    histogram (msau_label_hist, NCHW_HIST_K rows per sample, before the conversions) and hand its pointer to the kernel, else None."""
    B, C, H, W = heads[0].shape
    dev, Cs, s = heads[0].device, _ru(C, 8), torch.cuda.current_stream().cuda_stream
    label = label.reshape(B, H, W).contiguous().long()
    h = None
    if hist:
        h = torch.empty((B, NCHW_HIST_K, C), dtype=torch.int32, device=dev)
        L.call("msau_label_hist", s, label.data_ptr(), None, h.data_ptr(), B, H, W, C, NCHW_HIST_K)
    nhwc = [torch.empty((B, H, W, Cs), dtype=torch.float32, device=dev) for _ in heads]
    dn = [torch.empty_like(x) for x in nhwc]
    for t, x in zip(heads, nhwc):
        src = t.contiguous().float()
        L.call("msau_nchw_to_nhwc", s, L.F32, src.data_ptr(), x.data_ptr(), B, C, Cs, H, W)
    kernel([x.data_ptr() for x in nhwc], [d.data_ptr() for d in dn], label.data_ptr(), _ptr(h), B, H, W, C, Cs, s)
    grads = []
    for d in dn:
        g = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        L.call("msau_nhwc_to_nchw", s, L.F32, d.data_ptr(), g.data_ptr(), B, C, Cs, H, W)
        grads.append(g)
    return grads
