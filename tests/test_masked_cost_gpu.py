"""GPU: the masked cost -- msau_masked_cost / msau_masked_cost_eval against the float64 host statement
(tests/masked_cost_util.py), the bits the cross entropy, a junk parameter and gamma = 0 share, the register form against the cache form,
and the cost through `TrainEngine` (default path untouched, mean of the documents, `step_ids`, captured graph, training on the golden
FUNSD documents) and `MSAUWrapper.loss` / `eval_loss`.  Tolerances are the kernel family's (tests/test_unet_cost_gpu.py): relative
1e-5 (fp32) / 1e-2 (bf16, the inputs rounded first so that both sides see the same numbers; the stored gradient is bf16) on a loss,
the same times the reference gradient's largest element plus an absolute 1e-7 on gradients."""
import functools

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.model import _MaskedCEFunction
from tests import masked_cost_util as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
B, H, W = 3, 37, 29
EXTENTS = [(37, 29), (8, 6), (1, 1)]
MARGIN = (0, 3, 4, 1)                                                         # (b, y, x, label): the label's logit 50, every other 0; class 1 has weight
KIND = {M.CE: L.COST_CE, M.FOCAL: L.COST_FOCAL, M.DICE: L.COST_DICE}
PARAMS = {M.CE: (0.0,), M.FOCAL: (0.5, 2.0), M.DICE: (1.0, 1e-3)}
SETS = ("dense", "ragged", "ragged_empty")                                    # ragged_empty: the 8 x 6 document has no labelled pixel


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


@functools.lru_cache(maxsize=None)
def _inputs(C, dtype, which, Cs=None):
    """-> (logits [2] of [B,H,W,Cs] in the storage dtype, labels int64, extents, class weights), CPU tensors, left unchanged.
    Inside the extents about 40 % of the labels are 0 and a few are -1; one weight is 0 and (ragged) the 1 x 1 document's label is
    that class; head 0 has the MARGIN pixel; the padded channels hold random values (from a generator of their own: the real channels
    do not depend on Cs); ragged: outside the extents the labels are garbage, the logits 1e4 noise and one +inf"""
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    Cs = Cs or -(-C // 8) * 8
    g = torch.Generator().manual_seed(C)
    gp = torch.Generator().manual_seed(1000 + Cs)
    logits = [(torch.randn(B, H, W, Cs, generator=gp) * 2).to(td) for _ in range(2)]
    for x in logits:
        x[..., :C] = (torch.randn(B, H, W, C, generator=g) * 2).to(td)
    lab = torch.randint(1, C, (B, H, W), generator=g)
    u = torch.rand(B, H, W, generator=g)
    lab[u < 0.4] = 0
    lab[u > 0.99] = -1
    b, y, x, ml = MARGIN
    logits[0][b, y, x, :C] = 0.0
    logits[0][b, y, x, ml] = 50.0
    lab[b, y, x] = ml
    cw = torch.rand(C, generator=g) + 0.5
    cw[2] = 0.0
    ext = [(H, W)] * B
    if which != "dense":
        ext = EXTENTS
        lab[2, 0, 0] = 2
        lab[1, 1, 2], lab[1, 3, 3] = 1, 3                                     # (labelled whatever the draw)
        if which == "ragged_empty":
            lab[1, :8, :6] = torch.where(lab[1, :8, :6] > 0, torch.zeros((), dtype=torch.int64), lab[1, :8, :6])
        for b, (h, w) in enumerate(ext):
            keep_l = lab[b, :h, :w].clone()
            lab[b] = torch.randint(-5, 3 * C, (H, W), generator=g)
            lab[b, :h, :w] = keep_l
            for t in range(2):
                keep_x = logits[t][b, :h, :w].clone()
                logits[t][b] = (torch.randn(H, W, Cs, generator=g) * 1e4).to(td)
                if h < H:
                    logits[t][b, h, 0] = float("inf")
                logits[t][b, :h, :w] = keep_x
    return logits, lab, ext, cw


class _Dev:
    """a case on the device, with the label histogram at K rows"""

    def __init__(self, C, dtype, which, K, Cs=None):
        logits, lab, ext, cw = _inputs(C, dtype, which, Cs)
        self.C, self.Cs, self.K = C, logits[0].shape[3], K
        self.dt = L.F32 if dtype == "fp32" else L.BF16
        self.lg, self.lab = [x.to(DEV) for x in logits], lab.to(DEV)
        self.ext = torch.tensor(ext, dtype=torch.int32, device=DEV) if which != "dense" else None
        self.cw = cw.to(DEV)
        self.hist = torch.zeros((B, K, C), dtype=torch.int32, device=DEV)
        L.call("msau_label_hist", _stream(), self.lab.data_ptr(), _ptr(self.ext), self.hist.data_ptr(), B, H, W, C, K)

    def train(self, kind, param, with_aux, weighted, own_hist=False):
        """msau_masked_cost into sentinel-filled buffers -> (loss3, [gradients]) on the CPU.  The histogram is handed over when the
        call needs it (weights, Dice) or `own_hist` is off; otherwise the call counts the labelled pixels itself."""
        loss3 = torch.full((3,), 123.0, device=DEV)
        d = [torch.full_like(x, 9.0) for x in self.lg]
        give = weighted or kind == L.COST_DICE or not own_hist
        ws = torch.full((int(L.load().msau_masked_cost_ws_floats(kind, B, H, W, self.C)),), float("nan"), device=DEV)
        L.call("msau_masked_cost", _stream(), self.dt, kind, param, self.lg[0].data_ptr(), self.lg[1].data_ptr() if with_aux else None,
               self.lab.data_ptr(), _ptr(self.ext), self.cw.data_ptr() if weighted else None, self.hist.data_ptr() if give else None, self.K,
               d[0].data_ptr(), d[1].data_ptr() if with_aux else None, loss3.data_ptr(), ws.data_ptr(), B, H, W, self.C, self.Cs)
        torch.cuda.synchronize()
        return loss3.cpu(), [x.cpu() for x in d]

    def evaluate(self, kind, param, with_aux, weighted, K):
        """msau_masked_cost_eval -> (doc_loss [B, 2], doc_counts [B, 2, 2]) on the CPU"""
        loss = torch.full((B, 2), 123.0, device=DEV)
        counts = torch.full((B, 2, 2), 77, dtype=torch.int32, device=DEV)
        ws = torch.full((int(L.load().msau_masked_cost_eval_ws_bytes(kind, B, K, self.C)),), 255, dtype=torch.uint8, device=DEV)
        L.call("msau_masked_cost_eval", _stream(), self.dt, kind, param, self.lg[0].data_ptr(), self.lg[1].data_ptr() if with_aux else None,
               self.lab.data_ptr(), _ptr(self.ext), self.cw.data_ptr() if weighted else None, K, loss.data_ptr(), counts.data_ptr(),
               ws.data_ptr(), B, H, W, self.C, self.Cs)
        torch.cuda.synchronize()
        return loss.cpu(), counts.cpu()


@functools.lru_cache(maxsize=None)
def _host(kind, param, C, dtype, which, with_aux, weighted, Cs=None):
    logits, lab, ext, cw = _inputs(C, dtype, which, Cs)
    x = [t.double().numpy() for t in logits]
    return M.masked_cost_host(kind, param, x[0][..., :C], x[1][..., :C] if with_aux else None, lab.numpy(), ext if which != "dense" else None,
                              cw.double().numpy() if weighted else None)


def _assert_against_host(what, tol, C, lab, ext, got, ref, with_aux):
    """loss3 and every gradient element, the exact zeros, the absent head -> (worst loss error, worst gradient error), relative"""
    (loss3, d), (ref3, _doc, ref_g) = got, ref
    worst_l = worst_g = 0.0
    assert bool(torch.isfinite(loss3).all()), (what, loss3)
    for g_, r in zip(loss3.tolist(), ref3.tolist()):
        assert abs(g_ - r) <= tol * abs(r), (what, g_, r)
        worst_l = max(worst_l, abs(g_ - r) / abs(r) if r else 0.0)
    inactive = (lab < 1) | (lab >= C)
    for t, rg in enumerate(ref_g):
        x = d[t].float()
        assert bool(torch.isfinite(x).all()), (what, t)
        err, mx = float((x[..., :C].double() - torch.from_numpy(rg)).abs().max()), float(np.abs(rg).max())
        assert mx > 0 and err <= tol * mx + 1e-7, (what, t, err, mx)
        worst_g = max(worst_g, err / mx)
        assert x.shape[3] == C or float(x[..., C:].abs().max()) == 0.0, what          # padded channels: exactly 0
        assert float(x[inactive].abs().max()) == 0.0, what                            # inactive pixels: exactly 0
        for b, (h, w) in enumerate(ext):                                              # outside the extents: exactly 0
            assert float(x[b, h:].abs().sum()) == 0.0 and float(x[b, :, w:].abs().sum()) == 0.0, (what, b)
    if not with_aux:
        assert bool((d[1] == 9.0).all()), what                                        # the absent head is not written
    return worst_l, worst_g


# ---- 1: the training call against the host statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 8, 12, 17, 40])                                # 8: C == Cs in a register instance
@pytest.mark.parametrize("kind", [M.CE, M.FOCAL, M.DICE])
def test_masked_cost_equals_float64_host(kind, C, dtype):
    tol = 1e-5 if dtype == "fp32" else 1e-2
    worst = [0.0, 0.0]
    for which in SETS:
        _lg, lab, ext, _cw = _inputs(C, dtype, which)
        cases = {K: _Dev(C, dtype, which, K) for K in ((1, 4, 8) if kind == M.DICE else (1, 4))}    # 8 = the rows of the 8 x 6 document
        for param in PARAMS[kind]:
            for with_aux in (True, False):
                for weighted in (False, True):
                    ref = _host(kind, param, C, dtype, which, with_aux, weighted)
                    for K, case in cases.items():
                        what = (kind, param, C, dtype, which, with_aux, weighted, K)
                        own = K == 1                                                  # K = 1: the call counts the labelled pixels itself
                        got = case.train(KIND[kind], param, with_aux, weighted, own_hist=own)
                        again = case.train(KIND[kind], param, with_aux, weighted, own_hist=own)
                        assert torch.equal(got[0], again[0]) and all(torch.equal(a, b_) for a, b_ in zip(got[1], again[1])), what
                        wl, wg = _assert_against_host(what, tol, C, lab, ext, got, ref, with_aux)
                        worst = [max(worst[0], wl), max(worst[1], wg)]
                        assert abs(float(got[0][0]) - float(got[0][1]) - float(got[0][2])) <= 1e-6 * float(got[0][0]), what
                        if kind == M.FOCAL:                                           # 1 - p_t rounds to 0: no gradient at all
                            b, y, x, _lab = MARGIN
                            assert float(got[1][0][b, y, x].float().abs().max()) == 0.0, what
                        if which == "ragged_empty":                                   # the document without a labelled pixel
                            assert float(got[1][0][1].float().abs().max()) == 0.0, what
                    if which != "dense" and weighted and kind != M.DICE:
                        assert float(np.abs(ref[2][0][2]).max()) == 0.0 and ref[1][2, 0] == 0.0      # the D_b = 0 document
    print(kind, C, dtype, "worst relative error: loss", worst[0], "gradient (of its maximum)", worst[1])


# ---- 2: bit equalities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 17, 40])
def test_ce_junk_param_and_gamma_zero_are_equal_bit_for_bit(C, dtype):
    for which in ("dense", "ragged"):
        case = _Dev(C, dtype, which, 4)
        for with_aux in (True, False):
            for weighted in (False, True):
                want = case.train(L.COST_CE, 0.0, with_aux, weighted)
                assert float(want[0][0]) > 0 and float(want[1][0].float().abs().max()) > 0
                for kind, param in ((L.COST_CE, 7.0), (L.COST_FOCAL, 0.0)):
                    got = case.train(kind, param, with_aux, weighted)
                    what = (C, dtype, which, with_aux, weighted, kind)
                    assert torch.equal(got[0], want[0]), (what, got[0], want[0])
                    assert all(torch.equal(a, b_) for a, b_ in zip(got[1], want[1])), what


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", [M.CE, M.FOCAL, M.DICE])
def test_register_form_equals_cache_form(kind, dtype):
    """the same 17 real logits stored at Cs = 24 (a pixel in registers) and at Cs = 40 (a pixel read from the cache), the padded
    channels holding different random values: the same three loss bits, the same gradient bits in the real channels, zeros in the
    padded ones; the evaluation rows likewise"""
    C, K = 17, 4
    param = PARAMS[kind][-1]
    for which in ("dense", "ragged"):
        reg, wide = _Dev(C, dtype, which, K, 24), _Dev(C, dtype, which, K, 40)
        assert which != "dense" or torch.equal(reg.lg[0][..., :C], wide.lg[0][..., :C])      # (ragged: the garbage outside the extents differs)
        for with_aux in (True, False):
            for weighted in (False, True):
                what = (kind, dtype, which, with_aux, weighted)
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
    the first rung has none): every cost gives the same three loss bits, the same gradient bits in the real channels, zeros in the
    padded ones, and the same evaluation rows and counts"""
    K = 4
    for which in ("dense", "ragged"):
        rungs = {Cs: _Dev(C, dtype, which, K, Cs) for Cs in RUNGS}
        for kind in (M.CE, M.FOCAL, M.DICE):
            param = PARAMS[kind][-1]
            for with_aux in (True, False):
                for weighted in (False, True):
                    first = None
                    for Cs, case in rungs.items():
                        what = (kind, C, dtype, which, with_aux, weighted, Cs)
                        (l3, d), (rows, cnt) = case.train(KIND[kind], param, with_aux, weighted), case.evaluate(KIND[kind], param, with_aux, weighted, K)
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


# ---- 3: evaluation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 12, 17, 40])
@pytest.mark.parametrize("kind", [M.CE, M.FOCAL, M.DICE])
def test_masked_cost_eval_rows(kind, C, dtype):
    """rows against the host's doc_loss, the counts against numpy's, the cross entropy's rows at gamma = 0"""
    tol = 1e-5 if dtype == "fp32" else 1e-2
    worst = 0.0
    for which in SETS:
        logits, lab, ext, _cw = _inputs(C, dtype, which)
        case = _Dev(C, dtype, which, 4)
        for param in PARAMS[kind]:
            for with_aux in (True, False):
                want_counts = M.counts_host(logits[0].double().numpy(), logits[1].double().numpy() if with_aux else None, lab.numpy(),
                                            ext if which != "dense" else None, C)
                for weighted in (False, True):
                    _ref3, ref_doc, _g = _host(kind, param, C, dtype, which, with_aux, weighted)
                    for K in (1, 4, 8):
                        what = (kind, param, C, dtype, which, with_aux, weighted, K)
                        rows, cnt = case.evaluate(KIND[kind], param, with_aux, weighted, K)
                        again = case.evaluate(KIND[kind], param, with_aux, weighted, K)
                        assert torch.equal(rows, again[0]) and torch.equal(cnt, again[1]), what
                        assert np.array_equal(cnt.numpy(), want_counts), (what, cnt, want_counts)
                        assert bool(torch.isfinite(rows).all()), what
                        for g_, r in zip(rows.reshape(-1).tolist(), ref_doc.reshape(-1).tolist()):
                            assert abs(g_ - r) <= tol * abs(r), (what, g_, r)
                            worst = max(worst, abs(g_ - r) / abs(r) if r else 0.0)
                        assert with_aux or float(rows[:, 1].abs().max()) == 0.0, what
                        if kind == M.CE:
                            zero = case.evaluate(L.COST_FOCAL, 0.0, with_aux, weighted, K)
                            assert torch.equal(zero[0], rows) and torch.equal(zero[1], cnt), what
    print(kind, C, dtype, "worst relative error of a row", worst)


# ---- 4-8: the engine and the module -----------------------------------------------------------------------------------------------
CH, NCLS = 13, 5
SIZES = [(40, 32), (24, 16), (9, 7)]
CW5 = [1.0, 0.6, 0.0, 2.0, 1.4]
COSTS = {"focal": dict(cost={"cost_name": "focal", "gamma": 2.0}), "dice": dict(cost={"cost_name": "dice", "smooth": 1.0}),
         "weighted": dict(class_weights=CW5)}


def _model(dtype="fp32", **extra):
    return MSAUWrapper(CH, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


@functools.lru_cache(maxsize=None)
def _batch():
    """-> (x [3,13,40,32] one-hot of ids where occupied, ids int32 (-1: empty), labels int64, sizes): the documents at the origin,
    label garbage outside them"""
    g = torch.Generator().manual_seed(4)
    Hc, Wc = SIZES[0]
    ids = torch.full((len(SIZES), Hc, Wc), -1, dtype=torch.int32)
    lab = torch.randint(1, NCLS, (len(SIZES), Hc, Wc), generator=g)
    for b, (h, w) in enumerate(SIZES):
        occ = torch.rand((h, w), generator=g) < 0.35
        ids[b, :h, :w] = torch.where(occ, torch.randint(0, CH, (h, w), generator=g).int(), torch.full((), -1, dtype=torch.int32))
        lab[b, :h, :w] = occ * torch.randint(1, NCLS, (h, w), generator=g)
    x = torch.zeros((len(SIZES), CH, Hc, Wc))
    x.scatter_(1, ids.clamp(min=0).long().unsqueeze(1), (ids >= 0).unsqueeze(1).float())
    return x, ids, lab, torch.tensor(SIZES)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _two_steps(eng, x, lab, sizes):
    losses = []
    for _ in range(2):
        losses.append(eng.step(x.to(DEV), lab.to(DEV), sizes).clone())
    torch.cuda.synchronize()
    return torch.cat(losses).cpu(), eng.flat_grad.clone().cpu(), eng.model._flat.detach().clone().cpu()


def test_default_path_is_untouched():
    x, _ids, lab, sizes = _batch()
    want = _two_steps(TrainEngine(_model(deterministic=True)), x, lab, sizes)
    assert float(want[0][0]) > 0 and float(want[1].abs().max()) > 0
    for kw in (dict(cost={"cost_name": "cross_entropy"}), dict(cost={})):
        got = _two_steps(TrainEngine(_model(deterministic=True), **kw), x, lab, sizes)
        assert all(torch.equal(a, b_) for a, b_ in zip(got, want)), kw
    eng = TrainEngine(_model(deterministic=True))
    eng.set_cost({"cost_name": "dice"}, CW5)
    eng.set_cost(None)
    assert eng._cost is None and eng._cost_cw is None
    assert all(torch.equal(a, b_) for a, b_ in zip(_two_steps(eng, x, lab, sizes), want))
    # the new kernels at CE (weights all ones): other partial sums, the same loss
    ones = TrainEngine(_model(deterministic=True), lr=0.0, class_weights=[1.0] * NCLS)
    plain = TrainEngine(_model(deterministic=True), lr=0.0)
    l1, l0 = ones.step(x.to(DEV), lab.to(DEV), sizes), plain.step(x.to(DEV), lab.to(DEV), sizes)
    torch.cuda.synchronize()
    print("new CE against default CE: loss", abs(float(l1) - float(l0)) / float(l0), "gradient", _rel(ones.flat_grad, plain.flat_grad))
    assert abs(float(l1) - float(l0)) <= 1e-5 * float(l0) and _rel(ones.flat_grad, plain.flat_grad) <= 1e-4
    assert sorted(ones.state_dict()) == sorted(plain.state_dict())


@pytest.mark.parametrize("name", ["focal", "dice", "weighted"])
def test_fp32_step_is_the_mean_of_the_documents(name):
    x, ids, lab, sizes = _batch()
    m = _model(deterministic=True)
    eng = TrainEngine(m, lr=0.0, **COSTS[name])                               # lr 0: the parameters stay put between steps
    loss = eng.step(x.to(DEV), lab.to(DEV), sizes)
    torch.cuda.synchronize()
    loss, grad = loss.clone().cpu(), eng.flat_grad.clone().cpu()
    l_ids = eng.step_ids(ids.to(DEV), lab.to(DEV), sizes)
    torch.cuda.synchronize()
    assert torch.equal(l_ids.cpu(), loss) and torch.equal(eng.flat_grad.cpu(), grad)
    losses, grads = [], []
    for b, (h, w) in enumerate(SIZES):
        l1 = eng.step(x[b:b + 1, :, :h, :w].contiguous().to(DEV), lab[b:b + 1, :h, :w].contiguous().to(DEV))
        torch.cuda.synchronize()
        losses.append(float(l1))
        grads.append(eng.flat_grad.clone().cpu())
    ref_loss, ref_grad = sum(losses) / len(losses), sum(grads) / len(grads)
    print(name, "loss", abs(float(loss) - ref_loss) / ref_loss, "gradient", _rel(grad, ref_grad))
    assert ref_loss > 0 and abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    assert _rel(grad, ref_grad) <= 1e-4, _rel(grad, ref_grad)


def test_captured_graph_equals_eager():
    x, _ids, lab, sizes = _batch()
    kw = dict(cost={"cost_name": "focal", "gamma": 2.0}, class_weights=CW5)
    eager = _two_steps(TrainEngine(_model(deterministic=True), **kw), x, lab, sizes)
    graph_engine = TrainEngine(_model(deterministic=True), use_graph=True, **kw)          # one capture, two replays
    graph = _two_steps(graph_engine, x, lab, sizes)
    assert float(eager[0][0]) > 0 and float(eager[0][0]) != float(eager[0][1])
    assert all(torch.equal(a, b_) for a, b_ in zip(graph, eager))


def test_module_loss_and_eval_loss():
    Bm, C, Hm, Wm = 2, 7, 13, 11
    g = torch.Generator().manual_seed(11)
    m = MSAUWrapper(CH, C, dict(KW)).to(DEV)
    lg, ax = [(torch.randn(Bm, C, Hm, Wm, generator=g) * 2) for _ in range(2)]
    lab = torch.randint(1, C, (Bm, Hm, Wm), generator=g)
    lab[torch.rand(Bm, Hm, Wm, generator=g) < 0.4] = 0
    cw = [0.5, 1.5, 0.0, 1.0, 2.0, 0.7, 1.2]
    nhwc = lambda t: t.permute(0, 2, 3, 1).double().numpy()
    for kind, param, cost in ((M.FOCAL, 2.0, {"cost_name": "focal", "gamma": 2.0}), (M.DICE, 1.0, {"cost_name": "dice"}), (M.CE, 0.0, None)):
        for weights in (cw, None):
            if cost is None and weights is None:
                continue
            for with_aux in (True, False):
                a, b_ = lg.to(DEV).requires_grad_(True), ax.to(DEV).requires_grad_(True) if with_aux else None
                loss = m.loss(a, b_, lab.to(DEV), cost=cost, class_weights=weights)
                (2.0 * loss).backward()
                torch.cuda.synchronize()
                ref3, _doc, ref_g = M.masked_cost_host(kind, param, nhwc(lg), nhwc(ax) if with_aux else None, lab.numpy(), None, weights)
                what = (kind, weights is not None, with_aux)
                assert abs(float(loss.detach()) - ref3[0]) <= 1e-5 * ref3[0], (what, float(loss.detach()), ref3[0])
                for t, rg in zip((a, b_) if with_aux else (a,), ref_g):
                    err, mx = float(np.abs(nhwc(t.grad.cpu()) - 2.0 * rg).max()), 2.0 * float(np.abs(rg).max())
                    assert mx > 0 and err <= 1e-5 * mx + 1e-7, (what, err, mx)
    # the defaults: _MaskedCEFunction's bits
    a, b_ = lg.to(DEV).requires_grad_(True), ax.to(DEV).requires_grad_(True)
    l0 = m.loss(a, b_, lab.to(DEV))
    l0.backward()
    a2, b2 = lg.to(DEV).requires_grad_(True), ax.to(DEV).requires_grad_(True)
    l1 = _MaskedCEFunction.apply(a2, b2, lab.to(DEV))
    l1.backward()
    l2 = m.loss(lg.to(DEV), ax.to(DEV), lab.to(DEV), cost={"cost_name": "cross_entropy"})
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(l0, l2) and torch.equal(a.grad, a2.grad) and torch.equal(b_.grad, b2.grad)
    # eval_loss: the rows of msau_masked_cost_eval on the exported logits
    x, _ids, labels, sizes = _batch()
    net = _model()
    with torch.no_grad():
        _, logits, aux = net(x.to(DEV), sizes)
    Bn, Hn, Wn = labels.shape
    exported = [torch.zeros((Bn, Hn, Wn, 8), device=DEV) for _ in range(2)]
    for dst, src in zip(exported, (logits, aux)):
        dst[..., :NCLS] = src.permute(0, 2, 3, 1)
    ext = sizes.to(device=DEV, dtype=torch.int32).contiguous()
    for cost, kind, param in ((None, L.COST_CE, 0.0), ({"cost_name": "focal", "gamma": 0.5}, L.COST_FOCAL, 0.5), ({"cost_name": "dice"}, L.COST_DICE, 1.0)):
        for weights in (None, CW5):
            rows, counts = net.eval_loss(x.to(DEV), labels.to(DEV), sizes, cost=cost, class_weights=weights)
            K = net._plan_for(x.to(DEV), training=False, ragged=True).unet_eval_k()
            want = (torch.full((Bn, 2), 5.0, device=DEV), torch.full((Bn, 2, 2), 5, dtype=torch.int32, device=DEV))
            ws = torch.zeros(int(L.load().msau_masked_cost_eval_ws_bytes(kind, Bn, K, NCLS)), dtype=torch.uint8, device=DEV)
            cwd = torch.tensor(weights, device=DEV) if weights is not None else None
            L.call("msau_masked_cost_eval", _stream(), L.F32, kind, param, exported[0].data_ptr(), exported[1].data_ptr(), labels.to(DEV).data_ptr(),
                   ext.data_ptr(), _ptr(cwd), K, want[0].data_ptr(), want[1].data_ptr(), ws.data_ptr(), Bn, Hn, Wn, NCLS, 8)
            torch.cuda.synchronize()
            assert torch.equal(rows, want[0]) and torch.equal(counts, want[1]), (cost, weights)
            assert float(rows.min()) > 0 and int(counts[:, :, 0].min()) > 0 and not rows.requires_grad


@pytest.mark.parametrize("name", ["focal", "dice", "weighted"])
def test_it_trains_on_the_golden_documents(name, tmp_path, monkeypatch):
    import os
    import pickle
    from msau_amd.data import FUNSDCharGridDataLoaderBoxMaskBoxLabel, ragged
    from msau_amd.data.funsd import get_preprocessed_list_word_msau
    monkeypatch.chdir(tmp_path)                                               # (the loader writes its label map beside the process)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "funsd")
    docs, inv = get_preprocessed_list_word_msau(os.path.join(golden, "train"), None)
    docs = docs + get_preprocessed_list_word_msau(os.path.join(golden, "test"), inv)[0]       # (the training split's charset)
    with open("train.pkl", "wb") as fh:
        pickle.dump(docs, fh)
    loader = FUNSDCharGridDataLoaderBoxMaskBoxLabel("train.pkl")
    items = [loader[i] for i in range(len(loader))]
    assert len(items) == 3
    x, lab, sizes = ragged.pack(items)
    n_class = len(loader.labels) + 1
    m = MSAUWrapper(x.shape[1], n_class, dict(KW)).to(DEV)
    kw = dict(COSTS[name])
    if "class_weights" in kw:
        kw["class_weights"] = [1.0] + [0.5 + 0.5 * c for c in range(1, n_class)]
    eng = TrainEngine(m, lr=1e-3, **kw)
    x, lab = x.to(DEV), lab.to(DEV)
    plan = m._plan_for(x, training=True, ragged=True)
    totals = []
    for _ in range(20):
        loss = eng.step(x, lab, sizes)
        l3 = plan.masked_loss3.clone()
        totals.append(float(loss))
        assert np.isfinite(totals[-1]) and float(l3[0]) == totals[-1]
        assert abs(float(l3[0]) - float(l3[1]) - float(l3[2])) <= 1e-6 * max(1.0, float(l3[0])), l3
    print(name, "first", totals[0], "last", totals[-1])
    assert totals[-1] < totals[0]
