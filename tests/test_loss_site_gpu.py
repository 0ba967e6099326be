"""GPU: the host side of the losses (msau_amd/plan_loss.py).  The plumbing: every loss entry point of a Plan against the launch
sequence of include/msau_hip.h, written once here on the test's own buffers and on the plan's logits -- equal arguments give equal
bits (block partials, slab rows and the ordered sums: no floating-point atomics), so everything is compared bit for bit.  The NCHW
adapter of the five autograd functions: a non-contiguous NCHW view against its contiguous copy, bit for bit, and both against the
float64 statements of test_ops_gpu.py / test_unet_cost_gpu.py / test_masked_cost_gpu.py within those tests' tolerances."""
import functools

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper
from msau_amd.model import _MaskedCEFunction, _MaskedCostFunction
from msau_amd.plan import unet_cost
from msau_amd.training.cost import _SoftmaxCE, _UnetCost, _WeightedSoftmaxCE
from oracle import msau_oracle as O
from tests import masked_cost_util as M
from tests import unet_cost_util as U
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", seed=0)
CH, NCLS = 13, 5
B, H, W = 2, 33, 26
SIZES = [(33, 26), (17, 9)]               # the second document has fewer rows than the Dice K and than the evaluation's cap
HIST_K = {False: 16, True: 32}            # rows per document of msau_label_hist at B = 2: min(16, 256 // B), Dice min(32, 512 // B)
COUNTS_K = 16                             # msau_label_counts_split's K at B = 2: min(16, 256 // B)
COSTS = {"none": None, "focal": {"cost_name": "focal", "gamma": 0.5}, "dice": {"cost_name": "dice"}}
CW = [0.5, 1.0, 0.0, 2.0, 1.5]


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("MSAU_CE_MULTI", "MSAU_LABEL_SPLIT"):
        monkeypatch.delenv(name, raising=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _same_bits(a, b):
    raw = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


@functools.lru_cache(maxsize=None)
def _forwarded(num_blocks):
    """-> (model, its ragged training plan after one forward, the two label maps, the class weights, the extents), on the device"""
    g = torch.Generator().manual_seed(11 + num_blocks)
    model = MSAUWrapper(CH, NCLS, dict(KW, num_blocks=num_blocks)).to(DEV)
    x = torch.randn(B, CH, H, W, generator=g).to(DEV)
    plan = model._plan_for(x, training=True, ragged=True)
    plan.set_extents(torch.tensor(SIZES))
    plan.forward(model._flat, x, export=False)
    labels = [torch.randint(0, NCLS, (B, H, W), generator=g).to(DEV) for _ in range(2)]       # (also outside the documents)
    ext = torch.tensor(SIZES, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert (plan.aux is not None) == (num_blocks >= 2) and plan.logits.Cs == 8
    return model, plan, labels, torch.tensor(CW, device=DEV), ext


def _direct(plan, entry, cost, cw, labels, ext, eval_k):
    """the launches of `entry` under `cost` / `cw` as include/msau_hip.h spells them, on this call's own buffers and the plan's logits
    -> (loss values, gradient of the final head, of the auxiliary head) or (doc_loss, doc_counts)"""
    lg, ax = plan.logits, plan.aux
    s, dt, lib = _stream(), plan.dtype, L.load()
    C, Cs = lg.C, lg.Cs
    heads = (lg.data.data_ptr(), ax.data.data_ptr() if ax is not None else None)
    d = [torch.zeros_like(lg.data), torch.zeros_like(ax.data) if ax is not None else None]
    kind, param = (cost.kind, cost.param) if cost is not None else (L.COST_CE, 0.0)
    dice = kind == L.COST_DICE
    masked = entry in ("loss_grads", "eval_masked")
    maps = [labels[0]] if masked else [labels[0], labels[1] if ax is not None else None]
    shape = (B, H, W, C, Cs)
    if entry.startswith("eval"):
        out = (torch.zeros((B, 2), device=DEV), torch.zeros((B, 2, 2), dtype=torch.int32, device=DEV))
        rest = (ext.data_ptr(), _ptr(cw), eval_k, out[0].data_ptr(), out[1].data_ptr())
        if masked:
            ws = torch.zeros(int(lib.msau_masked_cost_eval_ws_bytes(kind, B, eval_k, C)), dtype=torch.uint8, device=DEV)
            L.call("msau_masked_cost_eval", s, dt, kind, param, *heads, maps[0].data_ptr(), *rest, ws.data_ptr(), *shape)
        elif cost is None:
            ws = torch.zeros(int(lib.msau_unet_eval_ws_bytes(B, eval_k)), dtype=torch.uint8, device=DEV)
            L.call("msau_unet_eval", s, dt, *heads, _ptr(maps[0]), _ptr(maps[1]), *rest, ws.data_ptr(), *shape)
        else:
            ws = torch.zeros(int(lib.msau_unet_cost_eval_ws_bytes(kind, B, eval_k, C)), dtype=torch.uint8, device=DEV)
            L.call("msau_unet_cost_eval", s, dt, kind, param, *heads, _ptr(maps[0]), _ptr(maps[1]), *rest, ws.data_ptr(), *shape)
        return out
    if masked and cost is None and cw is None:         # the default: the label canvas, the split counts, both heads' CE in one launch
        canvas, counts, loss = torch.zeros_like(labels[0]), torch.zeros(B * COUNTS_K, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
        ws = torch.zeros(int(lib.msau_ce_multi_ws_floats(B * H * W)), device=DEV)
        L.call("msau_extent_copy", s, labels[0].data_ptr(), canvas.data_ptr(), B, 1, H, W, 8, ext.data_ptr())
        L.call("msau_label_counts_split", s, canvas.data_ptr(), counts.data_ptr(), B, H * W, COUNTS_K)
        L.call("msau_masked_ce_multi", s, dt, *heads, canvas.data_ptr(), counts.data_ptr(), d[0].data_ptr(), _ptr(d[1]), loss.data_ptr(),
               ws.data_ptr(), B, H * W, C, Cs, 1.0 / B, COUNTS_K)
        return loss, d[0], d[1]
    K, hist = HIST_K[dice], None
    if cw is not None or dice:
        hist = torch.zeros((len(maps), B, K, C), dtype=torch.int32, device=DEV)
        for t, lab in enumerate(m for m in maps if m is not None):                          # the rows of head t behind those of head t - 1
            L.call("msau_label_hist", s, lab.data_ptr(), ext.data_ptr(), hist.data_ptr() + 4 * t * B * K * C, B, H, W, C, K)
    loss3 = torch.zeros(3, device=DEV)
    rest = (ext.data_ptr(), _ptr(cw), _ptr(hist), K, d[0].data_ptr(), _ptr(d[1]), loss3.data_ptr())
    if masked:
        ws = torch.zeros(int(lib.msau_masked_cost_ws_floats(kind, B, H, W, C)), device=DEV)
        L.call("msau_masked_cost", s, dt, kind, param, *heads, maps[0].data_ptr(), *rest, ws.data_ptr(), *shape)
    elif cost is None:
        ws = torch.zeros(int(lib.msau_unet_ce_ws_floats(B * H * W)), device=DEV)
        L.call("msau_unet_ce", s, dt, *heads, _ptr(maps[0]), _ptr(maps[1]), *rest, ws.data_ptr(), *shape)
    else:
        ws = torch.zeros(int(lib.msau_unet_cost_ws_floats(kind, B, H, W, C)), device=DEV)
        L.call("msau_unet_cost", s, dt, kind, param, *heads, _ptr(maps[0]), _ptr(maps[1]), *rest, ws.data_ptr(), *shape)
    return loss3, d[0], d[1]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cost_name", list(COSTS))
@pytest.mark.parametrize("entry", ["loss_grads", "loss_grads_unet", "eval_masked", "eval_unet"])
@pytest.mark.parametrize("num_blocks", [2, 1])
def test_plan_entry_point_issues_the_header_sequence(num_blocks, entry, cost_name, weighted):
    _model, plan, labels, cw, ext = _forwarded(num_blocks)
    cost, cw = COSTS[cost_name], cw if weighted else None
    cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    eval_k = max(1, min(256, min(h for h, _ in SIZES), -(-2 * cu // B)))       # two workgroups per compute unit, no empty slab
    assert plan.unet_eval_k() == eval_k and (plan.cost_hist_k(False), plan.cost_hist_k(True)) == (HIST_K[False], HIST_K[True])
    aux_labels = labels[1] if plan.aux is not None else None

    def through_the_plan(out=None):
        if entry == "loss_grads":
            loss = plan.loss_grads(labels[0], cost, cw)
        elif entry == "loss_grads_unet":
            loss = plan.loss_grads_unet(labels[0], aux_labels, cw, cost=cost)
        elif entry == "eval_masked":
            return plan.eval_masked(labels[0], cw, out=out, cost=cost)
        else:
            return plan.eval_unet(labels[0], aux_labels, cw, out=out, cost=cost)
        return loss, plan.logits.grad, plan.aux.grad if plan.aux is not None else None

    first = through_the_plan()
    kept = [t.clone() if t is not None else None for t in first]
    again = through_the_plan(out=first if entry.startswith("eval") else None)      # (an eval call: into the pair the first one made)
    want = _direct(plan, entry, unet_cost(cost), cw, labels, ext, eval_k)
    torch.cuda.synchronize()
    what = (num_blocks, entry, cost_name, weighted)
    for got, old, new, ref in zip(first, kept, again, want):
        if ref is None:
            assert got is None and new is None, what
            continue
        assert got.data_ptr() == new.data_ptr(), what        # the plan's buffers, or the pair handed in: the same storage both times
        assert _same_bits(old, new), what
        assert _same_bits(new, ref[:new.numel()] if ref.dim() == 1 else ref), what
    if entry.startswith("eval"):
        assert int(want[1][:, 0, 0].min()) > 0 and float(want[0][:, 0].min()) > 0, what
    else:
        assert float(want[0][0]) > 0 and float(want[1].abs().max()) > 0, what
        if entry == "loss_grads" and (cost is not None or cw is not None):
            assert _same_bits(plan.masked_loss3, want[0]) and first[0].data_ptr() == plan.masked_loss3.data_ptr(), what
        elif entry == "loss_grads_unet":
            assert first[0].numel() == 3, what


# ---- the NCHW adapter -------------------------------------------------------------------------------------------------------------
AB, AC, AH, AW = 2, 5, 9, 7


@functools.lru_cache(maxsize=None)
def _adapter_inputs():
    """-> (two heads' logits as NHWC fp32 [B,H,W,C], labels int64 [B,H,W]) on the CPU, left unchanged"""
    g = torch.Generator().manual_seed(3)
    x = [torch.randn(AB, AH, AW, AC, generator=g) * 2 for _ in range(2)]
    return x, torch.randint(0, AC, (AB, AH, AW), generator=g)


def _nchw64(t):
    return t.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)


def _reference(name, with_aux):
    """the float64 statement of `name` -> (loss, [gradient per head as NHWC float64 numpy])"""
    x, lab = _adapter_inputs()
    heads = x if with_aux else x[:1]
    if name in ("softmax_ce", "weighted_ce", "masked_ce"):
        leaves = [_nchw64(t) for t in heads]
        if name == "masked_ce":
            loss = O.msau_loss(leaves[0], leaves[1] if with_aux else None, lab)
        else:
            loss = torch.nn.functional.cross_entropy(leaves[0], lab, weight=torch.tensor(CW).double() if name == "weighted_ce" else None)
        loss.backward()
        return float(loss), [t.grad.permute(0, 2, 3, 1).numpy() for t in leaves]
    family, kind, weighted = name.split("_")
    param = {"ce": 0.0, "focal": 2.0, "dice": 1.0}[kind]
    nhwc = [t.double().numpy() for t in heads]
    cw = CW if weighted == "w" else None
    if family == "unet":
        ref3, _doc, grads = U.unet_cost_host(kind, param, nhwc[0], None, lab.numpy(), None, None, cw)
    else:
        ref3, _doc, grads = M.masked_cost_host(M.CE if kind == "ce" else kind, param, nhwc[0], nhwc[1] if with_aux else None, lab.numpy(), None, cw)
    return float(ref3[0]), grads


def _apply(name, heads, lab):
    cw = torch.tensor(CW, device=DEV)
    if name == "softmax_ce":
        return _SoftmaxCE.apply(heads[0], lab)
    if name == "weighted_ce":
        return _WeightedSoftmaxCE.apply(heads[0], lab, cw)
    if name == "masked_ce":
        return _MaskedCEFunction.apply(heads[0], heads[1] if len(heads) > 1 else None, lab)
    family, kind, weighted = name.split("_")
    cost = {"ce": (L.COST_CE, 0.0), "focal": (L.COST_FOCAL, 2.0), "dice": (L.COST_DICE, 1.0)}[kind]
    if family == "unet":
        return _UnetCost.apply(heads[0], lab, unet_cost({"cost_name": kind, "gamma": 2.0, "smooth": 1.0}), cw if weighted == "w" else None)
    return _MaskedCostFunction.apply(heads[0], heads[1] if len(heads) > 1 else None, lab, *cost, cw if weighted == "w" else None)


@pytest.mark.parametrize("name,with_aux", [("softmax_ce", False), ("weighted_ce", False), ("unet_focal_n", False), ("unet_focal_w", False),
                                           ("unet_dice_n", False), ("unet_dice_w", False), ("masked_ce", False), ("masked_ce", True),
                                           ("masked_ce_w", False), ("masked_ce_w", True), ("masked_focal_n", False),
                                           ("masked_focal_n", True), ("masked_dice_w", False), ("masked_dice_w", True)])
def test_autograd_function_on_a_view_and_on_its_copy(name, with_aux):
    """the logits as a permuted NHWC tensor (a non-contiguous NCHW view) and as that view's contiguous copy: value and input
    gradients bit-equal, and within the function's tolerance of its float64 statement.  (2.0 * loss).backward(): the scaling rule."""
    x, lab = _adapter_inputs()
    runs = []
    for contiguous in (False, True):
        views = [t.to(DEV).permute(0, 3, 1, 2) for t in (x if with_aux else x[:1])]
        assert not views[0].is_contiguous()
        heads = [(v.contiguous() if contiguous else v).requires_grad_(True) for v in views]
        assert heads[0].is_contiguous() == contiguous
        loss = _apply(name, heads, lab.to(DEV))
        (2.0 * loss).backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), [h.grad.clone() for h in heads]))
    assert _same_bits(runs[0][0], runs[1][0]), name
    for a, b in zip(runs[0][1], runs[1][1]):
        assert _same_bits(a.contiguous(), b.contiguous()), name
    ref_loss, ref_g = _reference(name, with_aux)
    got = float(runs[0][0])
    print(name, with_aux, "loss", got, "float64", ref_loss)
    if name in ("softmax_ce", "weighted_ce", "masked_ce"):            # test_ops_gpu.py's bounds
        assert abs(got - ref_loss) < 1e-5, (name, got, ref_loss)
        for g_, r in zip(runs[0][1], ref_g):
            assert rel_err(g_.permute(0, 2, 3, 1).cpu(), 2.0 * r) < 1e-5, name
    else:                                                             # test_unet_cost_gpu.py's / test_masked_cost_gpu.py's
        assert abs(got - ref_loss) <= 1e-5 * ref_loss, (name, got, ref_loss)
        for g_, r in zip(runs[0][1], ref_g):
            e, mx = float(np.abs(g_.permute(0, 2, 3, 1).double().cpu().numpy() - 2.0 * r).max()), 2.0 * float(np.abs(r).max())
            assert mx > 0 and e <= 1e-5 * mx + 1e-7, (name, e, mx)
