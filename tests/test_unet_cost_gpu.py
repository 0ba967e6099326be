"""GPU: UNetLoss under the focal and the soft Dice cost -- msau_unet_cost / msau_unet_cost_eval against the float64 host statement
(tests/unet_cost_util.py) on the shapes of test_kv_train_gpu.py's cross-entropy test, the cross entropy's bits at MSAU_COST_CE and at
gamma = 0, the register form against the cache form, and the cost through `TrainEngine.step_unet` / `step_kv`, `MSAUWrapper.eval_unet`
and the `UNetLoss` module.  Tolerances are the kernel family's: relative 1e-5 (fp32) / 1e-2 (bf16, the inputs rounded first so that
both sides see the same numbers; the stored gradient is bf16), plus an absolute 1e-7 on gradients."""
import functools

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import UNetLoss
from tests import kv_train_util as T
from tests import unet_cost_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = 60, T.N_CLASS
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
B, H, W = 3, 37, 29
EXTENTS = [(37, 29), (8, 6), (1, 1)]
MARGIN = (0, 3, 4, 1)                                                         # (b, y, x, label): the label's logit 50, every other 0; class 1 has weight
KIND = {U.FOCAL: L.COST_FOCAL, U.DICE: L.COST_DICE}
PARAMS = {U.FOCAL: (0.5, 2.0), U.DICE: (1.0, 1e-3)}
COSTS = {U.FOCAL: {"cost_name": "focal", "gamma": 2.0}, U.DICE: {"cost_name": "dice", "smooth": 1.0}}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


@functools.lru_cache(maxsize=None)
def _inputs(C, dtype, ragged, Cs=None):
    """-> (logits [2] of [B,H,W,Cs] in the storage dtype, labels [2] int64, extents, class weights), CPU tensors, left unchanged.
    Every label inside the extents is in [0, C); one weight is 0 and (ragged) the 1 x 1 document's final head has only that class;
    head 0 has the MARGIN pixel; the padded channels hold random values (from a generator of their own: the real channels do not
    depend on Cs); ragged: outside the extents labels -1, logits 1e4 garbage and one +inf"""
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    Cs = Cs or -(-C // 8) * 8
    g = torch.Generator().manual_seed(C)
    gp = torch.Generator().manual_seed(1000 + Cs)
    logits = [(torch.randn(B, H, W, Cs, generator=gp) * 2).to(td) for _ in range(2)]
    for x in logits:
        x[..., :C] = (torch.randn(B, H, W, C, generator=g) * 2).to(td)
    labs = [torch.randint(0, C, (B, H, W), generator=g) for _ in range(2)]
    b, y, x, lab = MARGIN
    logits[0][b, y, x, :C] = 0.0
    logits[0][b, y, x, lab] = 50.0
    labs[0][b, y, x] = lab
    cw = torch.rand(C, generator=g) + 0.5
    cw[2] = 0.0
    ext = [(H, W)] * B
    if ragged:
        ext = EXTENTS
        labs[0][2, 0, 0], labs[1][2, 0, 0] = 2, 3
        for b, (h, w) in enumerate(ext):
            for t in range(2):
                keep_l, keep_x = labs[t][b, :h, :w].clone(), logits[t][b, :h, :w].clone()
                labs[t][b] = -1
                logits[t][b] = (torch.randn(H, W, Cs, generator=g) * 1e4).to(td)
                if h < H:
                    logits[t][b, h, 0] = float("inf")
                labs[t][b, :h, :w], logits[t][b, :h, :w] = keep_l, keep_x
    return logits, labs, ext, cw


class _Dev:
    """a case on the device, with the label histograms of both heads at K rows"""

    def __init__(self, C, dtype, ragged, K, Cs=None):
        logits, labs, ext, cw = _inputs(C, dtype, ragged, Cs)
        self.C, self.Cs, self.K, self.ragged = C, logits[0].shape[3], K, ragged
        self.dt = L.F32 if dtype == "fp32" else L.BF16
        self.lg, self.lab = [x.to(DEV) for x in logits], [x.to(DEV) for x in labs]
        self.ext = torch.tensor(ext, dtype=torch.int32, device=DEV) if ragged else None
        self.cw = cw.to(DEV)
        self.hist = torch.zeros((2, B, K, C), dtype=torch.int32, device=DEV)
        for t in range(2):
            L.call("msau_label_hist", _stream(), self.lab[t].data_ptr(), _ptr(self.ext), self.hist[t].data_ptr(), B, H, W, C, K)

    def train(self, kind, param, with_aux, weighted, ce=False):
        """msau_unet_cost (ce: msau_unet_ce) into sentinel-filled buffers -> (loss3, [gradients]) on the CPU"""
        loss3 = torch.full((3,), 123.0, device=DEV)
        d = [torch.full_like(x, 9.0) for x in self.lg]
        rest = (self.lg[0].data_ptr(), self.lg[1].data_ptr() if with_aux else None, self.lab[0].data_ptr(),
                self.lab[1].data_ptr() if with_aux else None, _ptr(self.ext), self.cw.data_ptr() if weighted else None,
                self.hist.data_ptr() if weighted or kind == L.COST_DICE else None, self.K, d[0].data_ptr(), d[1].data_ptr() if with_aux else None,
                loss3.data_ptr())
        dims = (B, H, W, self.C, self.Cs)
        if ce:
            ws = torch.zeros(int(L.load().msau_unet_ce_ws_floats(B * H * W)), device=DEV)
            L.call("msau_unet_ce", _stream(), self.dt, *rest, ws.data_ptr(), *dims)
        else:
            ws = torch.full((int(L.load().msau_unet_cost_ws_floats(kind, B, H, W, self.C)),), float("nan"), device=DEV)
            L.call("msau_unet_cost", _stream(), self.dt, kind, param, *rest, ws.data_ptr(), *dims)
        torch.cuda.synchronize()
        return loss3.cpu(), [x.cpu() for x in d]

    def evaluate(self, kind, param, with_aux, weighted, K, plain=False):
        """msau_unet_cost_eval (plain: msau_unet_eval) -> (doc_loss [B, 2], doc_counts [B, 2, 2]) on the CPU"""
        loss = torch.full((B, 2), 123.0, device=DEV)
        counts = torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
        rest = (self.lg[0].data_ptr(), self.lg[1].data_ptr() if with_aux else None, self.lab[0].data_ptr(),
                self.lab[1].data_ptr() if with_aux else None, _ptr(self.ext), self.cw.data_ptr() if weighted else None, K, loss.data_ptr(),
                counts.data_ptr())
        dims = (B, H, W, self.C, self.Cs)
        if plain:
            ws = torch.zeros(int(L.load().msau_unet_eval_ws_bytes(B, K)), dtype=torch.uint8, device=DEV)
            L.call("msau_unet_eval", _stream(), self.dt, *rest, ws.data_ptr(), *dims)
        else:
            ws = torch.full((int(L.load().msau_unet_cost_eval_ws_bytes(kind, B, K, self.C)),), 255, dtype=torch.uint8, device=DEV)
            L.call("msau_unet_cost_eval", _stream(), self.dt, kind, param, *rest, ws.data_ptr(), *dims)
        torch.cuda.synchronize()
        return loss.cpu(), counts.cpu()


def _host(kind, param, C, dtype, ragged, with_aux, weighted, Cs=None):
    logits, labs, ext, cw = _inputs(C, dtype, ragged, Cs)
    x = [t.double().numpy() for t in logits]
    return U.unet_cost_host(kind, param, x[0][..., :C], x[1][..., :C] if with_aux else None, labs[0].numpy(), labs[1].numpy() if with_aux else None,
                            ext if ragged else None, cw.double().numpy() if weighted else None)


def _assert_against_host(what, tol, C, ext, got, ref, with_aux):
    """loss3 and every gradient element, the exact zeros, the absent head -> (worst loss error, worst gradient error), relative"""
    (loss3, d), (ref3, _doc, ref_g) = got, ref
    worst_l = worst_g = 0.0
    assert bool(torch.isfinite(loss3).all()), (what, loss3)
    for g_, r in zip(loss3.tolist(), ref3.tolist()):
        assert abs(g_ - r) <= tol * abs(r), (what, g_, r)
        worst_l = max(worst_l, abs(g_ - r) / abs(r) if r else 0.0)
    for t, rg in enumerate(ref_g):
        x = d[t].float()
        assert bool(torch.isfinite(x).all()), (what, t)
        err, mx = float((x[..., :C].double() - torch.from_numpy(rg)).abs().max()), float(np.abs(rg).max())
        assert mx > 0 and err <= tol * mx + 1e-7, (what, t, err, mx)
        worst_g = max(worst_g, err / mx)
        assert x.shape[3] == C or float(x[..., C:].abs().max()) == 0.0, what          # padded channels: exactly 0
        for b, (h, w) in enumerate(ext):                                              # outside the extents: exactly 0
            assert float(x[b, h:].abs().sum()) == 0.0 and float(x[b, :, w:].abs().sum()) == 0.0, (what, b)
    if not with_aux:
        assert bool((d[1] == 9.0).all()), what                                        # the absent head is not written
    return worst_l, worst_g


# ---- 1: the training call against the host statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 8, 12, 17, 40])                                # 8: C == Cs in a register instance
@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_unet_cost_equals_float64_host(kind, C, dtype):
    tol = 1e-5 if dtype == "fp32" else 1e-2
    worst = [0.0, 0.0]
    for ragged in (False, True):
        ext = _inputs(C, dtype, ragged)[2]
        cases = {K: _Dev(C, dtype, ragged, K) for K in ((1, 4, 8) if kind == U.DICE else (1, 4))}    # 8 > the rows of two documents
        for param in PARAMS[kind]:
            for with_aux in (True, False):
                for weighted in (False, True):
                    ref = _host(kind, param, C, dtype, ragged, with_aux, weighted)
                    for K, case in cases.items():
                        what = (kind, param, C, dtype, ragged, with_aux, weighted, K)
                        got = case.train(KIND[kind], param, with_aux, weighted)
                        again = case.train(KIND[kind], param, with_aux, weighted)
                        assert torch.equal(got[0], again[0]) and all(torch.equal(a, b_) for a, b_ in zip(got[1], again[1])), what
                        wl, wg = _assert_against_host(what, tol, C, ext, got, ref, with_aux)
                        worst = [max(worst[0], wl), max(worst[1], wg)]
                        if kind == U.FOCAL:                                           # 1 - p_t rounds to 0: no gradient at all
                            b, y, x, _lab = MARGIN
                            assert float(got[1][0][b, y, x].float().abs().max()) == 0.0, what
                    if ragged and weighted and kind == U.FOCAL:
                        assert float(np.abs(ref[2][0][2]).max()) == 0.0               # the D_b = 0 document
    print(kind, C, dtype, "worst relative error: loss", worst[0], "gradient (of its maximum)", worst[1])


# ---- 2: the cross entropy's bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 17, 40])
def test_cost_ce_and_gamma_zero_are_msau_unet_ce_bit_for_bit(C, dtype):
    for ragged in (False, True):
        case = _Dev(C, dtype, ragged, 4)
        for with_aux in (True, False):
            for weighted in (False, True):
                want = case.train(None, None, with_aux, weighted, ce=True)
                assert float(want[0][0]) > 0 and float(want[1][0].float().abs().max()) > 0
                for kind, param in ((L.COST_CE, 0.0), (L.COST_CE, 7.0), (L.COST_FOCAL, 0.0)):
                    got = case.train(kind, param, with_aux, weighted)
                    what = (C, dtype, ragged, with_aux, weighted, kind)
                    assert torch.equal(got[0], want[0]), (what, got[0], want[0])
                    assert all(torch.equal(a, b_) for a, b_ in zip(got[1], want[1])), what
                # and the evaluation rows
                rows = case.evaluate(None, None, with_aux, weighted, 4, plain=True)
                for kind in (L.COST_CE, L.COST_FOCAL):
                    got = case.evaluate(kind, 0.0, with_aux, weighted, 4)
                    assert torch.equal(got[0], rows[0]) and torch.equal(got[1], rows[1]), (C, dtype, ragged, with_aux, weighted, kind)


# ---- 3: register form against cache form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_register_form_equals_cache_form(kind, dtype):
    """the same 17 real logits stored at Cs = 24 (a pixel in registers) and at Cs = 40 (a pixel read from the cache), the padded
    channels holding different random values: the same three loss bits, the same gradient bits in the real channels, zeros in the
    padded ones"""
    C, K = 17, 4
    param = PARAMS[kind][1]
    for ragged in (False, True):
        reg, wide = _Dev(C, dtype, ragged, K, 24), _Dev(C, dtype, ragged, K, 40)
        assert ragged or torch.equal(reg.lg[0][..., :C], wide.lg[0][..., :C])      # (ragged: the garbage outside the extents differs)
        for with_aux in (True, False):
            for weighted in (False, True):
                what = (kind, dtype, ragged, with_aux, weighted)
                (l_r, d_r), (l_w, d_w) = reg.train(KIND[kind], param, with_aux, weighted), wide.train(KIND[kind], param, with_aux, weighted)
                assert torch.equal(l_r, l_w) and bool(torch.isfinite(l_r).all()) and float(l_r[0]) > 0, (what, l_r, l_w)
                for a, b_ in list(zip(d_r, d_w))[:2 if with_aux else 1]:
                    assert torch.equal(a[..., :C], b_[..., :C]) and float(a[..., :C].float().abs().max()) > 0, what
                    assert float(a[..., C:].float().abs().max()) == 0.0 and float(b_[..., C:].float().abs().max()) == 0.0, what
                e_r, e_w = reg.evaluate(KIND[kind], param, with_aux, weighted, K), wide.evaluate(KIND[kind], param, with_aux, weighted, K)
                assert torch.equal(e_r[0], e_w[0]) and torch.equal(e_r[1], e_w[1]), what


RUNGS = (8, 16, 24, 32, 40)                                                   # every register instance (Cs = 8 * CS8 <= 32) and the cache form


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 8])
def test_every_rung_gives_the_same_bits(C, dtype):
    """the same C real logits stored at every rung of the instance ladder, the padded channels holding different random values (C = 8:
    the first rung has none): the cross entropy, the focal and the Dice loss give the same three loss bits, the same gradient bits in the
    real channels, zeros in the padded ones, and the same evaluation rows and counts"""
    K = 4
    for ragged in (False, True):
        rungs = {Cs: _Dev(C, dtype, ragged, K, Cs) for Cs in RUNGS}
        for kind, param in ((L.COST_CE, 0.0), (L.COST_FOCAL, PARAMS[U.FOCAL][1]), (L.COST_DICE, PARAMS[U.DICE][1])):
            for with_aux in (True, False):
                for weighted in (False, True):
                    first = None
                    for Cs, case in rungs.items():
                        what = (kind, C, dtype, ragged, with_aux, weighted, Cs)
                        (l3, d), (rows, cnt) = case.train(kind, param, with_aux, weighted), case.evaluate(kind, param, with_aux, weighted, K)
                        assert bool(torch.isfinite(l3).all()) and float(l3[0]) > 0, (what, l3)
                        for x in d[:2 if with_aux else 1]:
                            assert float(x[..., :C].float().abs().max()) > 0, what
                            assert Cs == C or float(x[..., C:].float().abs().max()) == 0.0, what
                        if first is None:
                            first = (l3, d, rows, cnt)
                            continue
                        assert torch.equal(l3, first[0]), (what, l3, first[0])
                        for x, y in list(zip(d, first[1]))[:2 if with_aux else 1]:
                            assert torch.equal(x[..., :C], y[..., :C]), what
                        assert torch.equal(rows, first[2]) and torch.equal(cnt, first[3]), (what, rows, first[2])


# ---- 4: evaluation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 12, 17, 40])
@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_unet_cost_eval_rows(kind, C, dtype):
    """rows against the host's doc_loss, their document mean against the training call's loss3 (both are fp32 sums of the same
    numbers in different orders: 1e-5 in either dtype), the counts msau_unet_eval's"""
    tol = 1e-5 if dtype == "fp32" else 1e-2
    worst = 0.0
    for ragged in (False, True):
        case = _Dev(C, dtype, ragged, 4)
        for param in PARAMS[kind]:
            for with_aux in (True, False):
                for weighted in (False, True):
                    ref3, ref_doc, _g = _host(kind, param, C, dtype, ragged, with_aux, weighted)
                    loss3, _d = case.train(KIND[kind], param, with_aux, weighted)
                    counts = case.evaluate(None, None, with_aux, weighted, 4, plain=True)[1]
                    for K in (1, 4, 8):
                        what = (kind, param, C, dtype, ragged, with_aux, weighted, K)
                        rows, cnt = case.evaluate(KIND[kind], param, with_aux, weighted, K)
                        again = case.evaluate(KIND[kind], param, with_aux, weighted, K)
                        assert torch.equal(rows, again[0]) and torch.equal(cnt, again[1]) and torch.equal(cnt, counts), what
                        assert bool(torch.isfinite(rows).all()), what
                        for g_, r in zip(rows.reshape(-1).tolist(), ref_doc.reshape(-1).tolist()):
                            assert abs(g_ - r) <= tol * abs(r), (what, g_, r)
                            worst = max(worst, abs(g_ - r) / abs(r) if r else 0.0)
                        mean = rows.double().mean(dim=0).tolist()
                        for t in range(2 if with_aux else 1):
                            assert abs(mean[t] - float(loss3[1 + t])) <= 1e-5 * abs(mean[t]), (what, t, mean, loss3)
                        assert with_aux or float(rows[:, 1].abs().max()) == 0.0, what
    print(kind, C, dtype, "worst relative error of a row", worst)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dice_of_a_perfect_prediction(dtype):
    """logit 30 on the label everywhere in document 0: its loss is below 1e-3 at either smooth, and nothing is not finite"""
    C, Cs, K = 17, 24, 4
    td, dt = (torch.float32, L.F32) if dtype == "fp32" else (torch.bfloat16, L.BF16)
    logits, labs, _ext, _cw = _inputs(C, dtype, True)
    lg = [x.clone() for x in logits]
    for t in range(2):
        lg[t][0] = 0.0
        lg[t][0].scatter_(2, labs[t][0].unsqueeze(-1), torch.full((H, W, 1), 30.0, dtype=td))
    lg_d, lab_d = [x.to(DEV) for x in lg], [x.to(DEV) for x in labs]
    ext = torch.tensor(EXTENTS, dtype=torch.int32, device=DEV)
    hist = torch.zeros((2, B, K, C), dtype=torch.int32, device=DEV)
    for t in range(2):
        L.call("msau_label_hist", _stream(), lab_d[t].data_ptr(), ext.data_ptr(), hist[t].data_ptr(), B, H, W, C, K)
    for eps in PARAMS[U.DICE]:
        rows = torch.full((B, 2), 123.0, device=DEV)
        counts = torch.zeros((B, 2, 2), dtype=torch.int32, device=DEV)
        ws = torch.zeros(int(L.load().msau_unet_cost_eval_ws_bytes(L.COST_DICE, B, K, C)), dtype=torch.uint8, device=DEV)
        L.call("msau_unet_cost_eval", _stream(), dt, L.COST_DICE, eps, lg_d[0].data_ptr(), lg_d[1].data_ptr(), lab_d[0].data_ptr(),
               lab_d[1].data_ptr(), ext.data_ptr(), None, K, rows.data_ptr(), counts.data_ptr(), ws.data_ptr(), B, H, W, C, Cs)
        loss3 = torch.full((3,), 123.0, device=DEV)
        d = [torch.empty_like(x) for x in lg_d]
        ws2 = torch.zeros(int(L.load().msau_unet_cost_ws_floats(L.COST_DICE, B, H, W, C)), device=DEV)
        L.call("msau_unet_cost", _stream(), dt, L.COST_DICE, eps, lg_d[0].data_ptr(), lg_d[1].data_ptr(), lab_d[0].data_ptr(), lab_d[1].data_ptr(),
               ext.data_ptr(), None, hist.data_ptr(), K, d[0].data_ptr(), d[1].data_ptr(), loss3.data_ptr(), ws2.data_ptr(), B, H, W, C, Cs)
        torch.cuda.synchronize()
        print(dtype, eps, "rows", rows.tolist(), "loss3", loss3.tolist())
        assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(loss3).all()) and all(bool(torch.isfinite(x.float()).all()) for x in d)
        assert float(rows[0].abs().max()) < 1e-3 and float(rows[1].min()) > 0.1
        assert int(counts[0, 0, 0]) == int(counts[0, 0, 1]) > 0                        # every labelled pixel of it predicted


# ---- 5: the engine ----------------------------------------------------------------------------------------------------------------
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


CW = [0.0, 2.0] + [0.5 + 0.1 * c for c in range(NCLS - 2)]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _step(eng, ids, lab, aux, sizes=None, cw=None, cost=None, stats=None):
    loss = eng.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw, cost=cost, stats=stats)
    torch.cuda.synchronize()
    return loss.cpu().clone(), eng.flat_grad.clone().cpu()


@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_fp32_step_is_the_mean_of_the_documents(canvases, kind):
    """the bounds of test_kv_train_gpu.py's cross-entropy form of this test"""
    ids, lab, aux, sizes = canvases
    eng = TrainEngine(_model(), lr=0.0)
    for cw in (None, CW):
        loss, grad = _step(eng, ids, lab, aux, sizes, cw, COSTS[kind])
        losses, grads = [], []
        for b, (h, w) in enumerate(sizes.tolist()):
            l1, g1 = _step(eng, ids[b:b + 1, :h, :w], lab[b:b + 1, :h, :w], aux[b:b + 1, :h, :w], None, cw, COSTS[kind])
            losses.append(l1.double())
            grads.append(g1.double())
        ref_loss, ref_grad = sum(losses) / 3, sum(grads) / 3
        print(kind, cw is not None, "loss", loss.tolist(), "ref", ref_loss.tolist(), "grad rel", _rel(grad, ref_grad))
        for got, ref in zip(loss.tolist(), ref_loss.tolist()):
            assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        assert _rel(grad, ref_grad) <= 1e-4 and float(ref_grad.norm()) > 0
        l3 = loss.double().tolist()
        assert abs(l3[0] - (0.5 * l3[1] + 0.5 * l3[2])) <= 1e-6 * abs(l3[0]), l3


@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_tables_and_canvases_give_the_same_bits(gold, canvases, kind):
    ids, lab, aux, sizes = canvases
    a, b = TrainEngine(_model(deterministic=True)), TrainEngine(_model(deterministic=True))
    for _step_no in range(2):
        la = a.step_kv(gold, cost=COSTS[kind])
        lb = b.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, cost=COSTS[kind])
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.flat_grad, b.flat_grad) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and bool(torch.isfinite(a.model._flat).all())


@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_step_with_stats_is_the_step_and_the_rows_are_eval_unet(canvases, kind):
    ids, lab, aux, sizes = canvases
    a, b = TrainEngine(_model(deterministic=True)), TrainEngine(_model(deterministic=True))
    fresh = _model()
    stats = (torch.full((3, 2), 123.0, device=DEV), torch.full((3, 2, 2), 77, dtype=torch.int32, device=DEV))
    la, ga = _step(a, ids, lab, aux, sizes, CW, COSTS[kind])
    lb, gb = _step(b, ids, lab, aux, sizes, CW, COSTS[kind], stats=stats)
    assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(a.model._flat, b.model._flat)
    ref = fresh.eval_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=CW, cost=COSTS[kind])       # the weights before the step
    ce = fresh.eval_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=CW)
    # the counts the step wrote: those of a cross-entropy step with stats on the same weights (the same forward, so the same bits)
    c = TrainEngine(_model(deterministic=True))
    ce_stats = (torch.full((3, 2), 123.0, device=DEV), torch.full((3, 2, 2), 77, dtype=torch.int32, device=DEV))
    _step(c, ids, lab, aux, sizes, CW, None, stats=ce_stats)
    torch.cuda.synchronize()
    assert torch.equal(stats[1], ce_stats[1]) and int(stats[1][:, :, 0].min()) > 0 and torch.equal(stats[1][:, :, 0], ref[1][:, :, 0])
    assert not torch.equal(stats[0], ce_stats[0])
    print(kind, "rows", stats[0].tolist(), "eval_unet", ref[0].tolist(), "cross entropy", ce[0].tolist())
    assert torch.equal(ref[1], ce[1]) and not torch.equal(ref[0], ce[0])
    for g_, r in zip(stats[0].reshape(-1).tolist(), ref[0].reshape(-1).tolist()):
        assert abs(g_ - r) <= 1e-5 * abs(r), (g_, r)
    l3 = la.double().tolist()
    for t in range(2):
        assert abs(float(stats[0][:, t].double().mean()) - l3[1 + t]) <= 1e-5 * l3[1 + t]


def test_a_default_cost_step_is_todays_step(canvases):
    """no cost, the cross entropy by name, and the focal loss at gamma = 0 (the cross entropy's bits through msau_unet_cost): the
    same loss, gradient and parameters, bit for bit, with and without class weights"""
    ids, lab, aux, sizes = canvases
    for cw in (None, CW):
        out = []
        for cost in (None, {"cost_name": "cross_entropy"}, {"cost_name": "focal", "gamma": 0.0}):
            eng = TrainEngine(_model(deterministic=True))
            for _ in range(2):
                loss, grad = _step(eng, ids, lab, aux, sizes, cw, cost)
            out.append((loss, grad, eng.model._flat.clone().cpu()))
            keys = [l.key for l in eng.model._plan(3, ids.shape[1], ids.shape[2], DEV, True, eng.model._check_sizes_for(sizes, 3, ids.shape[1], ids.shape[2]))
                    .unet_launches(cw is not None, cost)]
            assert keys[-1] == ("msau_unet_ce" if cost is None or cost["cost_name"] == "cross_entropy" else "msau_unet_cost"), keys
        for other in out[1:]:
            assert all(torch.equal(x, y) for x, y in zip(out[0], other))
        assert float(out[0][0][0]) > 0


@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_unet_loss_module_against_float64_torch(kind):
    """loss and input gradient of `UNetLoss({"cost_name": ...})` on NCHW logits, every sample a document: fp32 bounds"""
    Bn, C, Hn, Wn = 2, 7, 13, 11
    g = torch.Generator().manual_seed(3)
    x = [(torch.randn(Bn, C, Hn, Wn, generator=g) * 2) for _ in range(2)]
    tg = [torch.randint(0, C, (Bn, Hn, Wn), generator=g) for _ in range(2)]
    one_hot = lambda t: torch.nn.functional.one_hot(t, C).permute(0, 3, 1, 2).float().to(DEV)
    for cw in (None, [0.5, 1.0, 0.0, 2.0, 1.5, 0.7, 1.1]):
        crit = UNetLoss(dict(COSTS[kind], **({"class_weights": cw} if cw is not None else {}))).to(DEV)
        xs = [t.to(DEV).requires_grad_(True) for t in x]
        acc, total, final = crit(xs[0], one_hot(tg[0]), {"aux_logits": xs[1], "aux_tgt": one_hot(tg[1])})
        total.backward()
        torch.cuda.synchronize()
        nhwc = [t.double().permute(0, 2, 3, 1).numpy() for t in x]
        ref3, _doc, ref_g = U.unet_cost_host(kind, COSTS[kind].get("gamma", COSTS[kind].get("smooth")), nhwc[0], nhwc[1], tg[0].numpy(), tg[1].numpy(), None, cw)
        total, final = float(total.detach()), float(final.detach())
        print(kind, cw is not None, "loss", total, final, "ref", ref3.tolist())
        assert abs(total - ref3[0]) <= 1e-5 * ref3[0] and abs(final - ref3[1]) <= 1e-5 * ref3[1] and 0 <= acc <= 1
        for t in range(2):
            want = torch.from_numpy(ref_g[t]).permute(0, 3, 1, 2)
            err = float((xs[t].grad.double().cpu() - want).abs().max())
            assert err <= 1e-5 * float(want.abs().max()) + 1e-7, (kind, t, err)
        acc1, alone, none = crit(xs[0].detach(), one_hot(tg[0]), {})
        assert none is None and abs(float(alone) - ref3[1]) <= 1e-5 * ref3[1]


@pytest.mark.parametrize("kind", [U.FOCAL, U.DICE])
def test_it_trains(gold, kind):
    eng = TrainEngine(_model())
    losses = []
    for _ in range(20):
        losses.append(eng.step_kv(gold, cost=COSTS[kind]).clone())
    torch.cuda.synchronize()
    losses = torch.stack(losses).cpu().double()
    print(kind, losses[:, 0].tolist())
    assert bool(torch.isfinite(losses).all())
    for l3 in losses.tolist():
        assert abs(l3[0] - (0.5 * l3[1] + 0.5 * l3[2])) <= 1e-6 * abs(l3[0]), l3
    assert float(losses[-1, 0]) < float(losses[0, 0])
