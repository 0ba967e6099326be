"""CPU: the masked cost -- the host statement (tests/masked_cost_util.py) against float64 torch autograd of the plain
torch expression of every cost, against the masked-CE golden and the oracle, and its simple identities; the ABI's four additions
and their argument checks (which return before anything is launched); the `cost` check of the engine and the module; the launch
accounting of `Plan.masked_cost_launches`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from oracle import msau_oracle as O
from tests import masked_cost_util as M
from tests.golden_util import load_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, CN = 3, 13, 11, 7
SIZES = [(13, 11), (6, 9), (2, 3)]
CW = [0.7, 1.3, 0.0, 2.0, 0.4, 1.1, 0.9]


def _case(seed, ragged):
    """two heads of logits and one label map with about 40 % zeros; ragged: label garbage and huge logits outside the extents, one
    label -1 and one label C inside"""
    g = torch.Generator().manual_seed(seed)
    x = [torch.randn(B, H, W, CN, generator=g, dtype=torch.float64) * 2 for _ in range(2)]
    lab = torch.randint(1, CN, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.4] = 0
    if ragged:
        for b, (h, w) in enumerate(SIZES):
            keep = lab[b, :h, :w].clone()
            lab[b] = torch.randint(-3, 2 * CN, (H, W), generator=g)
            lab[b, :h, :w] = keep
            for t in range(2):
                keep_x = x[t][b, :h, :w].clone()
                x[t][b] = 1e4
                x[t][b, :h, :w] = keep_x
        lab[0, 2, 3], lab[1, 1, 1] = -1, CN
        lab[2, 0, 0], lab[2, 1, 2] = 3, 5                                    # the small document has labelled pixels
    return x, lab


def _torch_total(kind, param, xs, lab, sizes, cw):
    """the definition, written with torch: every document's labelled pixels gathered -> (total, [per head])"""
    v = torch.tensor(cw, dtype=torch.float64) if cw is not None else torch.ones(CN, dtype=torch.float64)
    per_head = []
    for x in xs:
        tot = torch.zeros((), dtype=torch.float64)
        for b in range(B):
            h, w = sizes[b] if sizes is not None else (H, W)
            xb, tg = x[b, :h, :w].reshape(-1, CN), lab[b, :h, :w].reshape(-1)
            on = (tg >= 1) & (tg < CN)
            xb, tg = xb[on], tg[on]
            if len(tg) == 0:
                continue
            if kind == M.CE:
                if float(v[tg].sum()) > 0:
                    tot = tot + torch.nn.CrossEntropyLoss(weight=v)(xb, tg) / B
                continue
            logp = torch.log_softmax(xb, dim=1)
            p = logp.exp()
            if kind == M.FOCAL:
                D = float(v[tg].sum())
                if D > 0:
                    pt, nll = p[torch.arange(len(tg)), tg], -logp[torch.arange(len(tg)), tg]
                    tot = tot + (v[tg] * (1 - pt) ** param * nll).sum() / D / B
            elif float(v.sum()) > 0:
                oh = torch.nn.functional.one_hot(tg, CN).double()
                dice = (2 * (p * oh).sum(0) + param) / (p.sum(0) + oh.sum(0) + param)
                tot = tot + (1 - (v * dice).sum() / v.sum()) / B
        per_head.append(tot)
    return sum(per_head), per_head


@pytest.mark.parametrize("kind,param", [(M.CE, 0.0), (M.FOCAL, 0.5), (M.FOCAL, 1.0), (M.FOCAL, 2.0), (M.DICE, 1.0), (M.DICE, 1e-3)])
def test_host_statement_equals_float64_autograd(kind, param):
    for ragged in (True, False):
        x, lab = _case(3, ragged)
        sizes = SIZES if ragged else None
        for heads in (2, 1):
            for cw in (None, CW):
                xs = [t.clone().requires_grad_(True) for t in x[:heads]]
                total, per_head = _torch_total(kind, param, xs, lab, sizes, cw)
                total.backward()
                loss3, doc_loss, grads = M.masked_cost_host(kind, param, x[0].numpy(), x[1].numpy() if heads == 2 else None, lab.numpy(), sizes, cw)
                what = (kind, param, ragged, heads, cw is not None)
                want3 = [float(total.detach()), float(per_head[0].detach()), float(per_head[1].detach()) if heads == 2 else 0.0]
                assert np.allclose(loss3, want3, rtol=1e-12, atol=1e-15), (what, loss3, want3)
                assert np.allclose(doc_loss.mean(axis=0)[:heads], want3[1:1 + heads], rtol=1e-12), what
                assert want3[0] > 0 and loss3[0] == loss3[1] + loss3[2]
                for t in range(heads):
                    err = float(np.abs(grads[t] - xs[t].grad.numpy()).max())
                    assert err <= 1e-14, (what, t, err)
                    assert float(np.abs(grads[t]).max()) > 0
                    assert float(np.abs(grads[t][lab.numpy() == 0]).max()) == 0.0          # label 0 is inactive
                if ragged:
                    assert float(np.abs(grads[0][1, 6:]).max()) == 0.0 and float(np.abs(grads[0][0, 2, 3]).max()) == 0.0


def test_statement_reproduces_the_golden_and_the_oracle():
    """CE without weights, B = 1: the masked CE of the reference (the golden vectors it wrote) and of the oracle's restatement"""
    g = load_ops()
    lg, ax, lab = g["ce.logits"], g["ce.aux"], g["ce.label"]
    nhwc = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
    loss3, _doc, grads = M.masked_cost_host(M.CE, 0.0, nhwc(lg), nhwc(ax), lab)
    assert abs(loss3[0] - float(g["ce.loss"])) < 1e-6
    for got, want in zip(grads, (g["ce.glogits"], g["ce.gaux"])):
        assert float(np.abs(got - nhwc(want)).max()) <= 2e-5 * float(np.abs(want).max())
    tl, ta = torch.tensor(lg, dtype=torch.float64, requires_grad=True), torch.tensor(ax, dtype=torch.float64, requires_grad=True)
    loss = O.msau_loss(tl, ta, torch.tensor(lab))
    loss.backward()
    assert abs(loss3[0] - float(loss.detach())) < 1e-12
    assert float(np.abs(grads[0] - nhwc(tl.grad.numpy())).max()) < 1e-14 and float(np.abs(grads[1] - nhwc(ta.grad.numpy())).max()) < 1e-14
    # a batch, ragged: the oracle on every document's crop
    x, lab = _case(7, True)
    loss3, _doc, _g = M.masked_cost_host(M.CE, 0.0, x[0].numpy(), x[1].numpy(), lab.numpy(), SIZES)
    want = 0.0
    for b, (h, w) in enumerate(SIZES):
        crop = lab[b:b + 1, :h, :w].clone()
        crop[(crop < 0) | (crop >= CN)] = 0
        want += float(O.msau_loss(x[0][b:b + 1, :h, :w].permute(0, 3, 1, 2), x[1][b:b + 1, :h, :w].permute(0, 3, 1, 2), crop)) / B
    assert abs(loss3[0] - want) < 1e-12


def test_simple_identities():
    x, lab = _case(5, True)
    for cw in (None, CW):
        ce = M.masked_cost_host(M.CE, 0.0, x[0].numpy(), x[1].numpy(), lab.numpy(), SIZES, cw)
        f0 = M.masked_cost_host(M.FOCAL, 0.0, x[0].numpy(), x[1].numpy(), lab.numpy(), SIZES, cw)
        assert np.array_equal(ce[0], f0[0]) and np.array_equal(ce[1], f0[1]) and all(np.array_equal(a, b_) for a, b_ in zip(ce[2], f0[2]))
    for kind, param in ((M.CE, 0.0), (M.FOCAL, 2.0), (M.DICE, 1.0)):
        full = M.masked_cost_host(kind, param, x[0].numpy(), x[1].numpy(), lab.numpy(), SIZES, CW)
        assert full[0][0] == full[0][1] + full[0][2] and full[0][0] > 0
        # document 1 without a labelled pixel; document 2's only labelled class has weight 0 (CE, focal: D_b = 0)
        lab2 = lab.clone()
        lab2[1, :6, :9] = 0
        lab2[2, :2, :3] = 0
        lab2[2, 1, 1] = 2
        loss3, doc, grads = M.masked_cost_host(kind, param, x[0].numpy(), x[1].numpy(), lab2.numpy(), SIZES, CW)
        assert doc[1].tolist() == [0.0, 0.0] and all(float(np.abs(g_[1]).max()) == 0.0 for g_ in grads)
        if kind != M.DICE:
            assert doc[2].tolist() == [0.0, 0.0] and all(float(np.abs(g_[2]).max()) == 0.0 for g_ in grads)
        assert doc[0, 0] > 0 and abs(loss3[1] - doc[0, 0] / B - doc[2, 0] / B) < 1e-15          # B still divides
        zero = M.masked_cost_host(kind, param, x[0].numpy(), x[1].numpy(), lab2.numpy(), SIZES, [0.0] * CN)
        assert not zero[0].any() and not any(g_.any() for g_ in zero[2])                        # sum v = 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_additions():
    lib = L.load()
    assert lib.msau_version() == 11
    hdr = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    i = C.c_int
    decl = lambda fn: [" ".join(a.split()[:-1]) for a in re.search(rf"int {fn}\((.*?)\);", hdr, re.S).group(1).replace("\n", " ").split(",")]
    names = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(rf"int {fn}\((.*?)\);", hdr, re.S).group(1).replace("\n", " ").split(",")]
    # msau_unet_cost's / msau_unet_cost_eval's lists without the second label map
    for new, old in (("msau_masked_cost", "msau_unet_cost"), ("msau_masked_cost_eval", "msau_unet_cost_eval")):
        assert hasattr(lib, new)
        res, args = L._SIGNATURES[old]
        assert L._SIGNATURES[new] == (res, args[:7] + args[8:])
        assert decl(new) == decl(old)[:7] + decl(old)[8:]
    assert names("msau_masked_cost") == "stream dtype kind param logits aux labels extent class_w hist_partial K dlogits daux loss3 ws B H W C Cs".split()
    assert names("msau_masked_cost_eval") == "stream dtype kind param logits aux labels extent class_w K doc_loss doc_counts ws B H W C Cs".split()
    assert L._SIGNATURES["msau_masked_cost_ws_floats"] == (C.c_int64, [i] * 5) and L._SIGNATURES["msau_masked_cost_eval_ws_bytes"] == (C.c_int64, [i] * 4)
    assert hasattr(lib, "msau_masked_cost_ws_floats") and hasattr(lib, "msau_masked_cost_eval_ws_bytes")
    assert re.search(r"int64_t msau_masked_cost_ws_floats\(int kind, int B, int H, int W, int C\);", hdr)
    assert re.search(r"int64_t msau_masked_cost_eval_ws_bytes\(int kind, int B, int K, int C\);", hdr)
    # workspaces: CE and focal are msau_unet_ce's block partials and 16 histogram rows per document; Dice is msau_unet_cost's
    n = int(lib.msau_unet_ce_ws_floats(3 * 37 * 29))
    assert [int(lib.msau_masked_cost_ws_floats(k, 3, 37, 29, 17)) for k in (L.COST_CE, L.COST_FOCAL)] == [n + 3 * 16 * 17] * 2
    assert int(lib.msau_masked_cost_ws_floats(L.COST_DICE, 3, 37, 29, 17)) == 2 * 3 + 4 * 3 * 17 + 2 * 3 * 64 * 2 * 17
    rows = int(lib.msau_unet_eval_ws_bytes(3, 4))
    assert [int(lib.msau_masked_cost_eval_ws_bytes(k, 3, 4, 17)) for k in (L.COST_CE, L.COST_FOCAL)] == [rows, rows]
    assert int(lib.msau_masked_cost_eval_ws_bytes(L.COST_DICE, 3, 4, 17)) == rows + 4 * (2 * 3 * 4 * 2 * 17 + 3 * 4 * 17)
    assert int(lib.msau_masked_cost_eval_ws_bytes(L.COST_DICE, 3, 256, 17)) == int(lib.msau_unet_eval_ws_bytes(3, 256)) + 4 * (2 * 3 * 256 * 2 * 17 + 3 * 64 * 17)
    assert int(lib.msau_masked_cost_ws_floats(L.COST_CE, 0, 37, 29, 17)) == 0


def test_argument_errors_return_a_status():
    """every one of them is found before the first launch: no device is needed, the buffers are never touched"""
    buf = (C.c_float * 4096)()
    ptr = C.addressof(buf)
    lib = L.load()

    def train(kind, param, hist=ptr, K=1, cw=None, logits=ptr, B_=1):
        return lib.msau_masked_cost(None, L.F32, kind, param, logits, None, ptr, None, cw, hist, K, ptr, None, ptr, ptr, B_, 2, 2, 5, 8)

    def evaluate(kind, param, K=1):
        return lib.msau_masked_cost_eval(None, L.F32, kind, param, ptr, None, ptr, None, None, K, ptr, ptr, ptr, 1, 2, 2, 5, 8)

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
    refused("histograms", train(L.COST_DICE, 1.0, K=0))
    for kind in (L.COST_CE, L.COST_FOCAL):
        refused("histograms", train(kind, 1.0, hist=None, cw=ptr))
        refused("histograms", train(kind, 1.0, K=65))
        refused("histograms", train(kind, 1.0, K=0, cw=ptr))
        refused("null pointer", train(kind, 1.0, hist=None, logits=None))       # (before the call's own histogram launch)
        refused("bad dims", train(kind, 1.0, hist=None, B_=0))
    refused("K = 0", evaluate(L.COST_CE, 0.0, K=0))
    refused("K = 257", evaluate(L.COST_DICE, 1.0, K=257))
    assert not any(buf)
    with pytest.raises(L.MsauHipError, match="unknown cost"):
        L.call("msau_masked_cost", None, L.F32, 9, 0.0, ptr, None, ptr, None, None, None, 1, ptr, None, ptr, ptr, 1, 2, 2, 5, 8)


# ---- Python ------------------------------------------------------------------------------------------------------------------------
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)


def test_entry_points_refuse_a_bad_cost_before_anything_else():
    """on the CPU: the cost is checked first, so its ValueError comes before the need for a GPU"""
    from msau_amd import MSAUWrapper, TrainEngine
    m = MSAUWrapper(13, 5, KW)
    bad = {"cost_name": "focal", "gamma": -2.0}
    with pytest.raises(ValueError, match="gamma"):
        TrainEngine(m, cost=bad)
    with pytest.raises(ValueError, match="cost_name"):
        TrainEngine(m, cost={"cost_name": "tversky"})
    with pytest.raises(RuntimeError, match="GPU"):                           # a good cost: the constructor gets as far as before
        TrainEngine(m, cost={"cost_name": "focal"})
    x, lab = torch.zeros((1, 5, 8, 8)), torch.zeros((1, 8, 8), dtype=torch.int64)
    with pytest.raises(ValueError, match="gamma"):
        m.loss(x, x, lab, cost=bad)
    with pytest.raises(ValueError, match="smooth"):
        m.loss(x, None, lab, cost={"cost_name": "dice", "smooth": 0})
    with pytest.raises(ValueError, match="gamma"):
        m.eval_loss(torch.zeros((1, 13, 8, 8)), lab, cost=bad)
    with pytest.raises(ValueError, match="n_class"):
        m.eval_loss(torch.zeros((1, 13, 8, 8)), lab, class_weights=[1.0, 2.0])
    eng = TrainEngine.__new__(TrainEngine)                                    # no GPU here: the methods only reach their first lines
    eng.model, eng._token = m, 0
    with pytest.raises(ValueError, match="gamma"):
        eng.set_cost(bad)
    with pytest.raises(ValueError, match="cost_name"):
        eng.set_cost("focal")
    assert eng._token == 0


def test_set_cost_changes_the_graph_token():
    from msau_amd import MSAUWrapper, TrainEngine
    from msau_amd.plan import UnetCost
    eng = TrainEngine.__new__(TrainEngine)
    eng.model, eng._token = MSAUWrapper(13, 5, KW), TrainEngine._tokens
    seen = {eng._token}
    for cost in ({"cost_name": "focal", "gamma": 1.5}, {"cost_name": "dice"}, {"cost_name": "cross_entropy"}, None):
        eng.set_cost(cost)
        assert eng._token not in seen
        seen.add(eng._token)
        assert eng._cost == (UnetCost(L.COST_FOCAL, 1.5) if cost and cost["cost_name"] == "focal" else
                             UnetCost(L.COST_DICE, 1.0) if cost and cost["cost_name"] == "dice" else None) and eng._cost_cw is None
    import inspect
    assert "cost" not in inspect.getsource(TrainEngine.state_dict)           # configuration, not state


def test_launch_accounting_and_the_default_path():
    """`masked_cost_launches` on plans built on the CPU (as tools/plan_dump.py builds them): without a cost, with an empty one and
    with "cross_entropy" by name it states the two launches the plan's boundary record states -- keys and bytes written out here --
    and the plan's own launch lists, which is all a plan dump holds, do not depend on any of it"""
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
        assert Cs <= 16
        ce = px * (8 + nl * 2 * Cs * esz)
        today = [("msau_label_counts", px * 8), ("msau_masked_ce_multi", ce)]
        assert [kb for kb in keys(plan._boundary_launches()) if kb[0] in ("msau_label_counts", "msau_masked_ce_multi")] == today
        for cost in (None, {}, {"cost_name": "cross_entropy"}, {"cost_name": "cross_entropy", "class_weights": [1.0]}):
            assert keys(plan.masked_cost_launches(False, cost)) == today, (name, cost)
        hist = [("msau_label_hist", px * 8)]
        assert keys(plan.masked_cost_launches(True)) == keys(plan.masked_cost_launches(True, {})) == hist + [("msau_masked_cost", ce)]
        assert keys(plan.masked_cost_launches(False, {"cost_name": "focal"})) == [("msau_masked_cost", ce + px * 8)]
        assert keys(plan.masked_cost_launches(True, {"cost_name": "focal", "gamma": 0.5})) == hist + [("msau_masked_cost", ce)]
        for weighted in (False, True):
            assert keys(plan.masked_cost_launches(weighted, {"cost_name": "dice"})) == hist + [("msau_masked_cost", ce + px * (8 + nl * Cs * esz))]
        with pytest.raises(ValueError):
            plan.masked_cost_launches(False, {"cost_name": "tversky"})
        assert (plan.cost_hist_k(False), plan.cost_hist_k(True)) == (max(1, min(16, 256 // plan.B)), max(1, min(32, 512 // plan.B)))
        assert PD.launch_lists(plan) == before


@pytest.mark.parametrize("name", ["small.f32.train", "small.bf16.train", "cfg1.f32.train", "cfg1.bf16.train"])
def test_the_boundary_record_takes_its_loss_rows_from_the_loss_site(name):
    """the loss rows of `_boundary_launches` ARE the default rows of `masked_cost_launches(False)` -- same records, same order, side
    by side -- on a plan with an auxiliary head (small.*) and on one without (cfg1.*: num_blocks = 1), in both dtypes; the bytes are
    written out here once more so that the two cannot drift together"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    PD = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PD)
    plan = PD.build_plan({c[0]: c for c in PD.cases()}[name], "cpu")
    assert (plan.aux is not None) == name.startswith("small")
    rows = plan.masked_cost_launches(False)
    nl, esz = (2 if plan.aux is not None else 1), (4 if ".f32." in name else 2)
    px = plan.B * plan.H * plan.W
    assert [(r.kind, r.args, r.key, r.nbytes, r.flops) for r in rows] == \
        [(0, None, "msau_label_counts", px * 8, 0.0), (0, None, "msau_masked_ce_multi", px * (8 + nl * 2 * plan.logits.Cs * esz), 0.0)]
    boundary = plan._boundary_launches()
    at = [i for i, r in enumerate(boundary) if r.key in {x.key for x in rows}]
    assert at == list(range(at[0], at[0] + len(rows))) and [boundary[i] for i in at] == rows
    assert all(plan.launch_meta[r.key] == (1, r.nbytes, 0.0) for r in rows)
