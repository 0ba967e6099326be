"""CPU: UNetLoss under the focal and the soft Dice cost -- the host statement (tests/unet_cost_util.py) against float64 torch autograd
and, at gamma = 0, against `unet_eval_host`'s cross entropy; the per-pixel focal factor and the Dice coefficients of
csrc/loss_cost.h built as plain C++ (-DMSAU_COST_CPU) against the host statement and at their edges; the ABI's additions and their
argument checks (which return before anything is launched); the `cost` check in Python and `KVTrainer(cost_kwargs=...)`."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd.plan import UnetCost, unet_cost
from tests import unet_cost_util as U
from tests.kv_eval_util import unet_eval_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, CN = 3, 7, 6, 5
SIZES = [(7, 6), (4, 3), (1, 1)]
CW = [0.7, 1.3, 0.0, 2.0, 0.4]


def _case(seed, ragged):
    """two heads of logits and labels; ragged: label -1 and huge logits outside the extents, one label -1 and one label C inside"""
    g = torch.Generator().manual_seed(seed)
    x = [torch.randn(B, H, W, CN, generator=g, dtype=torch.float64) * 2 for _ in range(2)]
    lab = [torch.randint(0, CN, (B, H, W), generator=g) for _ in range(2)]
    if ragged:
        for t in range(2):
            for b, (h, w) in enumerate(SIZES):
                keep_l, keep_x = lab[t][b, :h, :w].clone(), x[t][b, :h, :w].clone()
                lab[t][b], x[t][b] = -1, 1e4
                lab[t][b, :h, :w], x[t][b, :h, :w] = keep_l, keep_x
            lab[t][0, 2, 3], lab[t][1, 1, 1] = -1, CN
        lab[0][2, 0, 0] = 2                                                  # the 1 x 1 document's only class has weight 0
    return x, lab


def _torch_total(kind, param, xs, labs, sizes, cw):
    """the definition, written with torch: every document's crop alone -> (total, [per head])"""
    v = torch.tensor(cw, dtype=torch.float64) if cw is not None else torch.ones(CN, dtype=torch.float64)
    per_head = []
    for x, lab in zip(xs, labs):
        tot = torch.zeros((), dtype=torch.float64)
        for b in range(B):
            h, w = sizes[b] if sizes is not None else (H, W)
            xb, tg = x[b, :h, :w].reshape(-1, CN), lab[b, :h, :w].reshape(-1)
            on = (tg >= 0) & (tg < CN)
            xb, tg = xb[on], tg[on]
            if len(tg) == 0:
                continue
            logp = torch.log_softmax(xb, dim=1)
            p = logp.exp()
            if kind == U.FOCAL:
                D = float(h * w) if cw is None else float(v[tg].sum())
                if D > 0:
                    pt, nll = p[torch.arange(len(tg)), tg], -logp[torch.arange(len(tg)), tg]
                    tot = tot + (v[tg] * (1 - pt) ** param * nll).sum() / D / B
            elif float(v.sum()) > 0:
                oh = torch.nn.functional.one_hot(tg, CN).double()
                dice = (2 * (p * oh).sum(0) + param) / (p.sum(0) + oh.sum(0) + param)
                tot = tot + (1 - (v * dice).sum() / v.sum()) / B
        per_head.append(tot)
    return (0.5 * per_head[0] + 0.5 * per_head[1] if len(per_head) == 2 else per_head[0]), per_head


@pytest.mark.parametrize("kind,param", [(U.FOCAL, 2.0), (U.FOCAL, 0.5), (U.FOCAL, 1.0), (U.DICE, 1.0), (U.DICE, 1e-3)])
def test_host_statement_equals_float64_autograd(kind, param):
    for ragged in (False, True):
        x, lab = _case(3, ragged)
        sizes = SIZES if ragged else None
        for heads in (2, 1):
            for cw in (None, CW):
                xs = [t.clone().requires_grad_(True) for t in x[:heads]]
                total, per_head = _torch_total(kind, param, xs, lab[:heads], sizes, cw)
                total.backward()
                loss3, doc_loss, grads = U.unet_cost_host(kind, param, x[0].numpy(), x[1].numpy() if heads == 2 else None, lab[0].numpy(),
                                                          lab[1].numpy() if heads == 2 else None, sizes, cw)
                what = (kind, param, ragged, heads, cw is not None)
                want3 = [float(total.detach()), float(per_head[0].detach()), float(per_head[1].detach()) if heads == 2 else 0.0]
                assert np.allclose(loss3, want3, rtol=1e-12, atol=1e-15), (what, loss3, want3)
                assert np.allclose(doc_loss.mean(axis=0)[:heads], want3[1:1 + heads], rtol=1e-12), what
                assert want3[0] > 0
                for t in range(heads):
                    err = float(np.abs(grads[t] - xs[t].grad.numpy()).max())
                    assert err <= 1e-14, (what, t, err)
                    assert float(np.abs(grads[t]).max()) > 0
                if ragged:
                    assert float(np.abs(grads[0][1, 4:]).max()) == 0.0 and float(np.abs(grads[0][0, 2, 3]).max()) == 0.0


def test_focal_at_gamma_zero_is_the_cross_entropy():
    x, lab = _case(5, True)
    for t in range(2):
        lab[t][0, 2, 3], lab[t][1, 1, 1] = 1, 2                              # every pixel inside the extents labelled: D_b is the area
    for cw in (None, CW):
        _loss3, doc_loss, _g = U.unet_cost_host(U.FOCAL, 0.0, x[0].numpy(), x[1].numpy(), lab[0].numpy(), lab[1].numpy(), SIZES, cw)
        want, _counts, _near = unet_eval_host(x[0].numpy(), x[1].numpy(), lab[0].numpy(), lab[1].numpy(), SIZES, cw)
        assert np.allclose(doc_loss, want, rtol=1e-13, atol=0), (doc_loss, want)
        assert cw is None or doc_loss[2, 0] == 0.0                           # the document without weight


# ---- the shared statements as plain C++ -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_cost(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("cost_cpu") / "libcost_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_COST_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "loss_cost.h"), "-o", out], check=True)
    lib = C.CDLL(out)
    fp = C.POINTER(C.c_float)
    lib.msau_focal_factor_cpu.restype = None
    lib.msau_focal_factor_cpu.argtypes = [C.c_float] * 3 + [fp] * 2
    lib.msau_dice_coef_cpu.restype = None
    lib.msau_dice_coef_cpu.argtypes = [C.c_float] * 5 + [fp] * 3
    lib.msau_dice_loss_cpu.restype = C.c_float
    lib.msau_dice_loss_cpu.argtypes = [C.c_float] * 2

    def focal(pt, nll, gamma):
        f, m = C.c_float(), C.c_float()
        lib.msau_focal_factor_cpu(pt, nll, gamma, C.byref(f), C.byref(m))
        return f.value, m.value

    def dice(I, P, Y, eps, vn):
        out3 = [C.c_float() for _ in range(3)]
        lib.msau_dice_coef_cpu(I, P, Y, eps, vn, *[C.byref(o) for o in out3])
        return tuple(o.value for o in out3)

    return focal, dice, lib.msau_dice_loss_cpu


def _pt_nll32(x, y):
    """a pixel's p_t and nll as the kernels have them: fp32 max, exp sum, log"""
    x = np.asarray(x, dtype=np.float32)
    mx = x.max()
    lse = np.float32(mx + np.log(np.exp(x - mx, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32))
    return float(np.exp(x[y] - lse, dtype=np.float32)), float(lse - x[y])


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0])
def test_cpp_focal_factor(cpu_cost, gamma):
    focal, _dice, _loss = cpu_cost
    g = np.random.default_rng(1)
    worst = 0.0
    for _ in range(200):
        x = g.normal(size=5) * 3
        pt, nll = _pt_nll32(x, int(g.integers(0, 5)))
        f, m = focal(pt, nll, gamma)
        wf, wm = U.focal_factor_host(np.float64(pt), np.float64(nll), gamma)
        worst = max(worst, abs(f - wf) / wf, abs(m - wm) / wm)
    assert worst <= 1e-6, worst
    if gamma == 0.0:
        assert focal(0.3, 1.2, 0.0) == (1.0, 1.0) and focal(1.0, 0.0, 0.0) == (1.0, 1.0)
    # p_t rounds to 1 (logit 50 against zeros): nothing left, and nothing that is not finite
    pt, nll = _pt_nll32([50.0, 0, 0, 0, 0], 0)
    assert pt == 1.0
    assert focal(pt, nll, gamma) == ((1.0, 1.0) if gamma == 0.0 else (0.0, 0.0))
    # p_t tiny (the label's logit 50 below): large, finite
    pt, nll = _pt_nll32([50.0, 0, 0, 0, 0], 1)
    f, m = focal(pt, nll, gamma)
    assert 0 < pt < 1e-20 and math.isfinite(f) and math.isfinite(m) and f == 1.0 and m == pytest.approx(1.0 + gamma * pt * nll, rel=1e-6)
    f, m = focal(0.0, 104.0, gamma)                                         # p_t underflowed to 0
    assert (f, m) == (1.0, 1.0)
    # the smallest 1 - p_t above 0
    f, m = focal(float(np.float32(1) - np.float32(2.0 ** -24)), 2.0 ** -24, gamma)
    assert math.isfinite(f) and math.isfinite(m) and f >= 0 and m >= 0


def test_cpp_dice_coefficients(cpu_cost):
    _focal, dice, loss = cpu_cost
    g = np.random.default_rng(2)
    v = np.array(CW)
    for eps in (1.0, 1e-3):
        for _ in range(50):
            n = int(g.integers(1, 400))
            P = g.random(CN) * n / CN
            I = P * g.random(CN)
            Y = g.integers(0, n, CN).astype(np.float64)
            want_loss, hit, miss = U.dice_coef_host(I, P, Y, eps, v)
            got = [dice(I[c], P[c], Y[c], eps, v[c] / v.sum()) for c in range(CN)]
            assert loss(v.sum(), sum(t for t, _h, _m in got)) == pytest.approx(want_loss, rel=1e-5)
            for c in range(CN):
                assert got[c][1] == pytest.approx(hit[c], rel=1e-5, abs=1e-12) and got[c][2] == pytest.approx(miss[c], rel=1e-5, abs=1e-12)
        # an absent class that nothing predicts: dice 1, and its logits are still pushed down (miss > 0)
        term, hit, miss = dice(0.0, 0.25, 0.0, eps, 0.2)
        assert term == pytest.approx(0.2 * eps / (0.25 + eps)) and miss > 0 and math.isfinite(hit)
        term, hit, miss = dice(0.0, 0.0, 0.0, eps, 0.2)                       # a document without an active pixel
        assert term == pytest.approx(0.2) and math.isfinite(hit) and math.isfinite(miss)
        # no weight at all: V = 0 -> vn = 0: loss 0, coefficients 0
        assert dice(3.0, 5.0, 4.0, eps, 0.0) == (0.0, 0.0, 0.0) and loss(0.0, 0.0) == 0.0
    assert loss(5.0, 1.0) == 0.0 and loss(5.0, 0.25) == 0.75
    want_loss, hit, miss = U.dice_coef_host(np.ones(CN), np.ones(CN), np.ones(CN), 1.0, np.zeros(CN))
    assert want_loss == 0.0 and not hit.any() and not miss.any()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_additions():
    lib = L.load()
    assert lib.msau_version() == 11
    hdr = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name, value in (("CE", L.COST_CE), ("FOCAL", L.COST_FOCAL), ("DICE", L.COST_DICE)):
        assert re.search(rf"#define MSAU_COST_{name} {value}\b", hdr), name
    assert (L.COST_CE, L.COST_FOCAL, L.COST_DICE) == (0, 1, 2)
    vp, i = C.c_void_p, C.c_int
    assert L._SIGNATURES["msau_unet_cost_ws_floats"] == (C.c_int64, [i] * 5)
    assert L._SIGNATURES["msau_unet_cost_eval_ws_bytes"] == (C.c_int64, [i] * 4)
    # `kind, param` in front of the rest of msau_unet_ce's / msau_unet_eval's list
    for new, old in (("msau_unet_cost", "msau_unet_ce"), ("msau_unet_cost_eval", "msau_unet_eval")):
        assert hasattr(lib, new) and hasattr(lib, old)
        res, args = L._SIGNATURES[old]
        assert L._SIGNATURES[new] == (res, args[:2] + [i, C.c_float] + args[2:])
        decl = lambda fn: [" ".join(a.split()[:-1]) for a in re.search(rf"int {fn}\((.*?)\);", hdr, re.S).group(1).replace("\n", " ").split(",")]
        assert decl(new) == decl(old)[:2] + ["int", "float"] + decl(old)[2:]
    assert hasattr(lib, "msau_unet_cost_ws_floats") and hasattr(lib, "msau_unet_cost_eval_ws_bytes")
    assert re.search(r"int64_t msau_unet_cost_ws_floats\(int kind, int B, int H, int W, int C\);", hdr)
    assert re.search(r"int64_t msau_unet_cost_eval_ws_bytes\(int kind, int B, int K, int C\);", hdr)
    # workspaces: CE and focal are msau_unet_ce's / msau_unet_eval's; Dice adds its table and rows
    n = int(lib.msau_unet_ce_ws_floats(3 * 37 * 29))
    assert [int(lib.msau_unet_cost_ws_floats(k, 3, 37, 29, 17)) for k in (L.COST_CE, L.COST_FOCAL)] == [n, n]
    assert int(lib.msau_unet_cost_ws_floats(L.COST_DICE, 3, 37, 29, 17)) == 2 * 3 + 4 * 3 * 17 + 2 * 3 * 64 * 2 * 17
    rows = int(lib.msau_unet_eval_ws_bytes(3, 4))
    assert [int(lib.msau_unet_cost_eval_ws_bytes(k, 3, 4, 17)) for k in (L.COST_CE, L.COST_FOCAL)] == [rows, rows]
    assert int(lib.msau_unet_cost_eval_ws_bytes(L.COST_DICE, 3, 4, 17)) == rows + 4 * (2 * 3 * 4 * 2 * 17 + 2 * 3 * 4 * 17)
    assert int(lib.msau_unet_cost_eval_ws_bytes(L.COST_DICE, 3, 256, 17)) == int(lib.msau_unet_eval_ws_bytes(3, 256)) + 4 * (2 * 3 * 256 * 2 * 17 + 2 * 3 * 64 * 17)


def test_argument_errors_return_a_status():
    """every one of them is found before the first launch: no device is needed, the buffers are never touched"""
    buf = (C.c_float * 4096)()
    ptr = C.addressof(buf)
    lib = L.load()

    def train(kind, param, hist=ptr, K=1):
        return lib.msau_unet_cost(None, L.F32, kind, param, ptr, None, ptr, None, None, None, hist, K, ptr, None, ptr, ptr, 1, 2, 2, 5, 8)

    def evaluate(kind, param):
        return lib.msau_unet_cost_eval(None, L.F32, kind, param, ptr, None, ptr, None, None, None, 1, ptr, ptr, ptr, 1, 2, 2, 5, 8)

    def refused(match, rc):
        assert rc == -1
        assert re.search(match, lib.msau_last_error().decode()), (match, lib.msau_last_error())

    for fn in (train, evaluate):
        refused("unknown cost", fn(3, 1.0))
        refused("unknown cost", fn(-1, 1.0))
        for gamma in (-0.5, float("nan"), float("inf"), -float("inf")):
            refused("gamma", fn(L.COST_FOCAL, gamma))
        for eps in (0.0, -1.0, float("nan"), float("inf")):
            refused("smooth", fn(L.COST_DICE, eps))
    refused("histograms", train(L.COST_DICE, 1.0, hist=None))
    refused("histograms", train(L.COST_DICE, 1.0, K=65))
    assert not any(buf)
    with pytest.raises(L.MsauHipError, match="unknown cost"):
        L.call("msau_unet_cost", None, L.F32, 9, 0.0, ptr, None, ptr, None, None, None, None, 1, ptr, None, ptr, ptr, 1, 2, 2, 5, 8)


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_cost_is_checked_in_one_place():
    assert unet_cost(None) is None and unet_cost({}) is None and unet_cost({"cost_name": "cross_entropy", "class_weights": [1.0]}) is None
    assert unet_cost({"cost_name": "focal"}) == UnetCost(L.COST_FOCAL, 2.0) and unet_cost({"cost_name": "focal", "gamma": 0}) == UnetCost(L.COST_FOCAL, 0.0)
    assert unet_cost({"cost_name": "dice"}) == UnetCost(L.COST_DICE, 1.0)
    assert unet_cost({"cost_name": "dice", "smooth": 1e-3, "act_name": "softmax"}) == UnetCost(L.COST_DICE, 1e-3)
    c = unet_cost({"cost_name": "focal", "gamma": 0.5})
    assert unet_cost(c) is c
    for bad in ({"cost_name": "dice_coefficient"}, {"cost_name": "focal", "gamma": -1}, {"cost_name": "focal", "gamma": float("nan")},
                {"cost_name": "focal", "gamma": "two"}, {"cost_name": "focal", "gamma": float("inf")}, {"cost_name": "dice", "smooth": 0},
                {"cost_name": "dice", "smooth": -1.0}, {"cost_name": "dice", "smooth": None}, "focal", ("focal", 2.0)):
        with pytest.raises(ValueError):
            unet_cost(bad)


def test_entry_points_refuse_a_bad_cost_before_anything_else():
    """on the CPU: the cost is checked first, so its ValueError comes before the need for a GPU"""
    from msau_amd import MSAUWrapper, TrainEngine
    from msau_amd.training import UNetLoss
    kw = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
    m = MSAUWrapper(13, 5, kw)
    ids, lab = torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 8, 8), dtype=torch.int64)
    bad = {"cost_name": "focal", "gamma": -2.0}
    with pytest.raises(ValueError, match="gamma"):
        m.eval_unet(ids, lab, lab, cost=bad)
    with pytest.raises(ValueError, match="gamma"):
        m.eval_kv([], cost=bad)
    eng = TrainEngine.__new__(TrainEngine)                                    # no GPU here: the methods only reach their first lines
    eng.use_graph = False
    eng._eager = lambda name: None
    for call in (lambda: eng.step_unet(ids, lab, lab, cost=bad), lambda: eng.step_kv([], cost=bad),
                 lambda: eng.step_unet_nhwc(torch.zeros((1, 8, 8, 16)), lab, lab, cost={"cost_name": "tversky"})):
        with pytest.raises(ValueError, match="gamma|cost_name"):
            call()
    with pytest.raises(ValueError, match="smooth"):
        UNetLoss({"cost_name": "dice", "smooth": 0.0})
    # every other cost_name keeps the reference's behaviour: the prediction comes back
    x = torch.randn(1, 5, 4, 4)
    assert torch.equal(UNetLoss({"cost_name": "dice_coefficient"})(x, None, {}), torch.softmax(x, dim=1))
    assert UNetLoss({"cost_name": "focal", "gamma": 1.5}).cost == UnetCost(L.COST_FOCAL, 1.5) and UNetLoss({}).cost is None


class _Batches:
    batch_size = 2

    def __next__(self):
        return ["t0", "t1"]

    def validation(self):
        return [["v0", "v1"], ["v2"]]


class _Model:
    def __init__(self):
        self.flat_parameters, self.calls = torch.zeros(1), []

    def eval_kv(self, tables, **kw):
        self.calls.append(kw)
        return torch.full((len(tables), 2), 0.25), torch.ones((len(tables), 2, 2), dtype=torch.int32)


class _Engine:
    def __init__(self):
        self.lr, self.calls = None, []

    def step_kv(self, tables, stats=None, **kw):
        self.calls.append(kw)
        stats[0].fill_(0.5)
        stats[1].fill_(1)


def test_kv_trainer_passes_the_cost_to_every_step_and_every_validation():
    from msau_amd.training.kv_trainer import KVTrainer

    class Stubbed(KVTrainer):
        def _engine(self, kwargs):
            return _Engine()

    for cost_kwargs, want in (({"cost_name": "dice", "smooth": 0.5}, {"cost": UnetCost(L.COST_DICE, 0.5)}),
                              ({"cost_name": "focal"}, {"cost": UnetCost(L.COST_FOCAL, 2.0)}), (None, {}), ({"cost_name": "cross_entropy"}, {})):
        model = _Model()
        tr = Stubbed(model, _Batches(), class_weights=[1.0, 2.0], cost_kwargs=cost_kwargs)
        hist = tr.fit(None, 2, 3)
        assert len(tr.engine.calls) == 6 and len(model.calls) == 4
        for kw in tr.engine.calls + model.calls:
            assert kw == dict(class_weights=[1.0, 2.0], **want), kw
        assert hist[0]["train"]["loss"] == 0.5 and hist[0]["val"]["loss"] == 0.25
    with pytest.raises(ValueError, match="cost_name"):
        Stubbed(_Model(), _Batches(), cost_kwargs={"cost_name": "lovasz"})


def test_launch_accounting_and_the_default_path():
    """`unet_launches` / `unet_eval_launches` on plans built on the CPU (as tools/plan_dump.py builds them): without a cost, with an
    empty one and with "cross_entropy" by name they state the launches they stated before there were costs -- the keys and the bytes
    written out here -- and the plan's own launch lists, which is all a plan dump holds, do not depend on any of it"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    PD = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PD)
    cases = {c[0]: c for c in PD.cases()}
    keys = lambda launches: [(l.key, l.nbytes) for l in launches]
    for name, esz in (("small.f32.train", 4), ("cfg2.bf16.ragged", 2)):
        plan = PD.build_plan(cases[name], "cpu")
        before = PD.launch_lists(plan)
        nl = 2 if plan.aux is not None else 1
        px, Cs = plan.B * plan.H * plan.W, plan.logits.Cs
        ce, once = px * nl * (8 + 2 * Cs * esz), px * nl * (8 + Cs * esz)
        hist = [("msau_label_hist", px * 8)] * nl
        for weighted in (False, True):
            want = (hist if weighted else []) + [("msau_unet_ce", ce)]
            assert keys(plan.unet_launches(weighted)) == want
            for cost in (None, {}, {"cost_name": "cross_entropy"}, {"cost_name": "cross_entropy", "class_weights": [1.0]}):
                assert keys(plan.unet_launches(weighted, cost)) == want, (name, weighted, cost)
            assert keys(plan.unet_launches(weighted, {"cost_name": "focal"})) == (hist if weighted else []) + [("msau_unet_cost", ce)]
            assert keys(plan.unet_launches(weighted, {"cost_name": "dice"})) == hist + [("msau_unet_cost", ce + once)]
        assert keys(plan.unet_eval_launches()) == keys(plan.unet_eval_launches({"cost_name": "cross_entropy"})) == [("msau_unet_eval", once)]
        assert keys(plan.unet_eval_launches({"cost_name": "focal", "gamma": 0.5})) == [("msau_unet_cost_eval", once)]
        assert keys(plan.unet_eval_launches({"cost_name": "dice"})) == [("msau_unet_cost_eval", 2 * once + px * nl * 8)]
        with pytest.raises(ValueError):
            plan.unet_launches(False, {"cost_name": "tversky"})
        assert PD.launch_lists(plan) == before
