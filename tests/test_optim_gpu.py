"""GPU: msau_optim_step (csrc/optim.hip) -- RMSprop, SGD with momentum and Adam with weight decay, optional global-norm clip, skip
ranges -- against torch.optim, and its way through TrainEngine / KVTrainer.

The yardstick is torch.optim in float64 on the CPU.  The same torch optimiser in float32 gives e32 = max |p32 - p64|, the error of
one valid fp32 evaluation; the device must stay within 2 * e32 (the factor is the room for another equally valid rounding order:
FMA contraction, 1/x against a division).  The state buffers follow the same rule on the element-wise relative error."""
import ctypes as C

import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from tests import kv_train_util as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = 60, T.N_CLASS
KW = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
KINDS = {"adam": L.OPTIM_ADAM, "rmsprop": L.OPTIM_RMSPROP, "momentum": L.OPTIM_MOMENTUM}
BUFFERS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "momentum": ("momentum_buffer",)}
C1C2 = {"adam": (0.9, 0.999), "rmsprop": (0.99, 0.0), "momentum": (0.9, 0.0)}
LR, EPS = 1e-3, 1e-8
EXTENTS = [(37, 29), (8, 6), (1, 1)]
GRID = 512 * 256            # the update's grid: 512 workgroups of 256 threads, grid-stride beyond


def _inputs(n):
    torch.manual_seed(9)
    p0 = torch.randn(n)
    g0 = 3 * torch.randn(n)
    g0[:50] = 0
    return p0, g0


def _torch_opt(kind, params, lr, wd):
    if kind == "rmsprop":
        return torch.optim.RMSprop(params, lr=lr, weight_decay=wd)
    if kind == "momentum":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=wd)
    return torch.optim.Adam(params, lr=lr, weight_decay=wd)


def _torch_run(kind, p0, grads, wd, max_norm, gs, dtype):
    """torch.optim on the CPU in `dtype`; `grads`: the fp32 gradients the device sees, pre-multiplied by grad_scale here"""
    p = p0.to(dtype).clone().requires_grad_()
    opt = _torch_opt(kind, [p], LR, wd)
    norm = None
    for g in grads:
        p.grad = g.to(dtype) * gs
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        opt.step()
    return p.detach(), [opt.state[p][name].detach() for name in BUFFERS[kind]], norm


class _Dev:
    """parameters, state buffers and the 8-float state vector of one msau_optim_step run"""

    def __init__(self, kind, p0, bufs=None):
        self.kind, self.n = kind, p0.numel()
        self.p = p0.to(DEV).clone()
        nbuf = len(BUFFERS[kind])
        self.bufs = [torch.zeros_like(self.p) for _ in range(nbuf)] if bufs is None else [b.to(DEV).clone() for b in bufs]
        self.state = torch.zeros(8, dtype=torch.float32, device=DEV)
        self.ws = torch.zeros(max(int(L.load().msau_optim_ws_floats(self.n)), 1), dtype=torch.float32, device=DEV)

    def step(self, g, wd, max_norm, gs, ranges=()):
        g = g.to(DEV)
        arr = (C.c_int64 * max(2 * len(ranges), 1))(*[v for r in ranges for v in r])
        c1, c2 = C1C2[self.kind]
        L.call("msau_optim_step", torch.cuda.current_stream().cuda_stream, KINDS[self.kind], self.p.data_ptr(), g.data_ptr(),
               self.bufs[0].data_ptr(), self.bufs[1].data_ptr() if len(self.bufs) > 1 else None, self.state.data_ptr(),
               self.ws.data_ptr(), self.n, LR, c1, c2, EPS, wd, max_norm, gs, arr, len(ranges))
        torch.cuda.synchronize()


def _rel_err(x, ref):
    """element-wise relative error; an exact zero of the reference wants an exact zero"""
    x, ref = x.double(), ref.double()
    return float(((x - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def _check(kind, dev, p0, grads, wd, max_norm, gs, what):
    p64, s64, norm = _torch_run(kind, p0, grads, wd, max_norm, gs, torch.float64)
    p32, s32, _ = _torch_run(kind, p0, grads, wd, max_norm, gs, torch.float32)
    e32 = float((p32.double() - p64).abs().max())
    edev = float((dev.p.cpu().double() - p64).abs().max())
    print(f"{what}: params e32 {e32:.3e} device {edev:.3e} ({edev / max(e32, 1e-300):.2f} x)")
    assert edev <= 2 * e32, (what, edev, e32)
    for name, b_dev, b32, b64 in zip(BUFFERS[kind], dev.bufs, s32, s64):
        r32, rdev = _rel_err(b32, b64), _rel_err(b_dev.cpu(), b64)
        print(f"{what}: {name} relative e32 {r32:.3e} device {rdev:.3e} ({rdev / max(r32, 1e-300):.2f} x)")
        assert rdev <= 2 * r32, (what, name, rdev, r32)
    st = dev.state.cpu().tolist()
    assert st[0] == len(grads), st
    if max_norm > 0:
        assert abs(st[1] - norm) <= 1e-4 * norm, (st, norm)
        assert abs(st[2] - min(1.0, max_norm / (norm + 1e-6))) <= 1e-4, (st, norm)
    return e32, edev


# ---- 1: the launch against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind", ["rmsprop", "momentum", "adam"])
def test_three_steps_against_torch(kind, wd, max_norm, gs):
    n = 10007
    p0, g0 = _inputs(n)
    grads = [g0 * k for k in (1, 2, 3)]
    dev = _Dev(kind, p0)
    for g in grads:
        dev.step(g, wd, max_norm, gs)
    _check(kind, dev, p0, grads, wd, max_norm, gs, f"{kind} wd {wd} max_norm {max_norm} grad_scale {gs}")
    if max_norm <= 0 and kind != "adam":
        assert dev.state.cpu().tolist()[1:3] == [0.0, 0.0]          # the single launch leaves norm and coefficient alone


# ---- 2: sizes where the indexing can go wrong -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1025, 10007, GRID + 1])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("kind", ["rmsprop", "momentum", "adam"])
def test_sizes(kind, max_norm, n):
    p0, g0 = _inputs(n)
    if n <= 50:
        g0 = 3 * torch.randn(n)              # (the zeroed head of _inputs would be the whole gradient)
    guard = 64
    dev = _Dev(kind, torch.cat([p0, torch.full((guard,), 7.0)]))
    dev.n = n                                # the launch sees n elements; the tail behind them must stay as it is
    for b in dev.bufs:
        b[n:] = 5.0
    dev.step(torch.cat([g0, torch.full((guard,), 3.0)]), 0.01, max_norm, 1.0)
    assert bool((dev.p[n:] == 7.0).all()) and all(bool((b[n:] == 5.0).all()) for b in dev.bufs)
    dev.p, dev.bufs = dev.p[:n], [b[:n] for b in dev.bufs]
    _check(kind, dev, p0, [g0], 0.01, max_norm, 1.0, f"{kind} n {n} max_norm {max_norm}")


# ---- 3: skip ranges -------------------------------------------------------------------------------------------------------------------
RANGES = {"start": [(0, 5)], "across_workgroups": [(250, 262)], "end": [(1022, 1025)], "adjacent": [(500, 510), (510, 530)],
          "several": [(0, 5), (250, 262), (500, 530), (1022, 1025)]}


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("kind", ["rmsprop", "momentum", "adam"])
def test_skip_ranges(kind, max_norm):
    n = 1025
    p0, g0 = _inputs(n)
    p0 = p0 + 0.5 * torch.sign(p0)                               # no parameter near zero
    bufs0 = [torch.rand(n) + 0.25 for _ in BUFFERS[kind]]        # non-zero pre-filled state
    for name, ranges in RANGES.items():
        g = g0.clone()
        inside = torch.zeros(n, dtype=torch.bool)
        for b, e in ranges:
            g[b:e] = 0
            inside[b:e] = True
        with_r, without = _Dev(kind, p0, bufs0), _Dev(kind, p0, bufs0)
        with_r.step(g, 0.01, max_norm, 1.0, ranges)
        without.step(g, 0.01, max_norm, 1.0)
        assert torch.equal(with_r.p.cpu()[inside], p0[inside]), name
        assert not bool((without.p.cpu()[inside] == p0[inside]).any()), name          # (the weight decay alone moves them)
        assert torch.equal(with_r.p.cpu()[~inside], without.p.cpu()[~inside]), name
        for b_r, b_n, b0 in zip(with_r.bufs, without.bufs, bufs0):
            assert torch.equal(b_r.cpu()[inside], b0[inside]), name
            assert torch.equal(b_r.cpu()[~inside], b_n.cpu()[~inside]), name
        assert torch.equal(with_r.state, without.state), name


# ---- 4: determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rmsprop", "momentum", "adam"])
def test_two_runs_give_equal_bits(kind):
    n = GRID + 1
    p0, g0 = _inputs(n)
    runs = []
    for _ in range(2):
        dev = _Dev(kind, p0)
        for k in (1, 2):
            dev.step(g0 * k, 0.01, 1.0, 1.0)
        runs.append(dev)
    a, b = runs
    assert torch.equal(a.p, b.p) and torch.equal(a.state, b.state) and all(torch.equal(x, y) for x, y in zip(a.bufs, b.bufs))


# ---- 5: the engine's plumbing, fed its own gradient --------------------------------------------------------------------------------
def _model(dtype="fp32", **extra):
    return MSAUWrapper(CH, NCLS, dict(KW, dtype=dtype, **extra)).to(DEV)


@pytest.fixture(scope="module")
def gold():
    return T.gold_tables(0)


@pytest.fixture(scope="module")
def canvases(gold):
    """the three golden documents on one ragged canvas, cut to the extents 37x29 / 8x6 / 1x1 at their origins (what lies outside
    an extent is ignored: a small document, a tiny one and a single pixel in one step), as CPU tensors; shared and left unchanged"""
    ids, lab, aux, sizes = T.canvases_want(gold)
    assert all(h <= hh and w <= ww for (h, w), (hh, ww) in zip(EXTENTS, sizes.tolist())), sizes
    return torch.from_numpy(ids), torch.from_numpy(lab), torch.from_numpy(aux), torch.tensor(EXTENTS, dtype=torch.from_numpy(sizes).dtype)


def _flat_of(m, tensors):
    out = torch.zeros(m._flat.numel(), dtype=torch.float64)
    for (key, p), t in zip(m._named, tensors):
        out[m._poff[key]:m._poff[key] + p.numel()] = t.detach().reshape(-1).double()
    return out


@pytest.mark.parametrize("kind,wd", [("rmsprop", 0.0), ("momentum", 0.0), ("adam", 0.01), ("rmsprop", 0.01)])
def test_engine_steps_follow_torch_on_the_engines_own_gradient(canvases, kind, wd):
    ids, lab, aux, sizes = canvases
    m = _model()
    eng = TrainEngine(m, lr=LR, optimizer=kind, weight_decay=wd, max_norm=None)
    p_start = m._flat.cpu().clone()
    lrs = [LR, 0.5 * LR]
    # three CPU copies of the parameter list: float64 and float32 following the engine's learning rates, float64 staying at the first
    copies = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32), ("f64_same_lr", torch.float64)):
        ps = [p.detach().cpu().to(dtype).clone().requires_grad_() for _, p in m._named]
        copies[name] = (ps, _torch_opt(kind, ps, LR, wd))
    dead = torch.zeros(m._flat.numel(), dtype=torch.bool)
    for key, p in m._named:
        if key in m._dead:
            dead[m._poff[key]:m._poff[key] + p.numel()] = True
    assert int(dead.sum()) > 0
    for step, lr in enumerate(lrs):
        eng.lr = lr
        eng.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
        torch.cuda.synchronize()
        g = eng.flat_grad.cpu()
        assert float(g[dead].abs().max()) == 0.0 and float(g.abs().max()) > 0
        for name, (ps, opt) in copies.items():
            opt.param_groups[0]["lr"] = LR if name == "f64_same_lr" else lr
            for (key, p), q in zip(m._named, ps):
                q.grad = None if key in m._dead else g[m._poff[key]:m._poff[key] + p.numel()].view(p.shape).to(q.dtype).clone()
            opt.step()
        p64, p32 = _flat_of(m, copies["f64"][0]), _flat_of(m, copies["f32"][0])
        pdev = m._flat.cpu().double()
        e32, edev = float((p32 - p64).abs().max()), float((pdev - p64).abs().max())
        print(f"{kind} wd {wd} step {step + 1}: e32 {e32:.3e} device {edev:.3e} ({edev / e32:.2f} x)")
        assert edev <= 2 * e32, (step, edev, e32)
        assert torch.equal(m._flat.cpu()[dead], p_start[dead])
    # the second step ran at the halved rate: the copy that kept the first rate is far away
    far = float((m._flat.cpu().double() - _flat_of(m, copies["f64_same_lr"][0])).abs().max())
    assert far > 10 * e32, (far, e32)
    assert float(eng.state[0]) == 2.0


# ---- 6: use_graph ---------------------------------------------------------------------------------------------------------------------
def test_graph_engine_gives_the_eager_bits_under_rmsprop():
    torch.manual_seed(3)
    x = torch.zeros(2, CH, 16, 16)
    x.scatter_(1, torch.randint(0, CH, (2, 1, 16, 16)), 1.0)
    labels = torch.randint(0, NCLS, (2, 16, 16))
    x, labels = x.to(DEV), labels.to(DEV)
    res = {}
    for use_graph in (False, True):
        m = _model(deterministic=True)
        eng = TrainEngine(m, lr=LR, optimizer="rmsprop", max_norm=None, use_graph=use_graph)
        losses = [float(eng.step(x, labels)) for _ in range(3)]
        torch.cuda.synchronize()
        res[use_graph] = (losses, m._flat.clone(), eng.square_avg.clone(), float(eng.state[0]))
    assert res[False][0] == res[True][0], res
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    assert res[False][3] == res[True][3] == 3.0
    assert float(res[False][2].abs().max()) > 0


# ---- 7: guards ------------------------------------------------------------------------------------------------------------------------
def test_guards_and_the_default_engines_entry_point(canvases, monkeypatch):
    ids, lab, aux, sizes = canvases
    with pytest.raises(ValueError, match="optimizer"):
        TrainEngine(_model(), optimizer="adagrad")
    calls = []
    real = L.call

    def recording(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)

    monkeypatch.setattr(L, "call", recording)
    default = TrainEngine(_model())
    default.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
    assert calls.count("msau_clip_adam_step") == 1 and "msau_optim_step" not in calls
    assert default.optim_launches()[0][0] == "msau_clip_adam_step" and len(default.optim_launches()) == 1
    assert float(default.grad_norm) > 0
    assert (default.square_avg, default.momentum_buffer) == (None, None)
    del calls[:]
    rms = TrainEngine(_model(), optimizer="rmsprop", max_norm=None)
    rms.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
    assert calls.count("msau_optim_step") == 1 and "msau_clip_adam_step" not in calls
    assert [k for k, _ in rms.optim_launches()] == ["msau_optim_step<rmsprop>"]
    assert (rms.m, rms.v, rms.momentum_buffer) == (None, None, None)
    with pytest.raises(RuntimeError, match="norm"):
        rms.grad_norm
    clipped = TrainEngine(_model(), optimizer="momentum", max_norm=1.0)
    clipped.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
    assert float(clipped.grad_norm) > 0 and len(clipped.optim_launches()) == 2
    # the norm is the default engine's: same model, same batch
    assert abs(float(clipped.grad_norm) - float(default.grad_norm)) <= 1e-5 * float(default.grad_norm)
    for eng, other in ((rms, default), (default, rms), (clipped, rms)):
        with pytest.raises(ValueError, match="engine runs"):
            eng.load_state_dict(other.state_dict())
    with pytest.raises(ValueError, match="engine runs"):
        rms.load_state_dict(torch.optim.SGD(list(rms.model.parameters()), lr=0.1, momentum=0.9).state_dict())


# ---- 8: KVTrainer with the reference's optimiser options -----------------------------------------------------------------------------
class _Batches:
    """the golden group, over and over"""
    batch_size = 3

    def __init__(self, group):
        self.group = group

    def __iter__(self):
        return self

    def __next__(self):
        return self.group

    def validation(self):
        return [self.group]


def test_kv_trainer_with_opt_kwargs_trains_with_rmsprop(gold, capsys):
    from msau_amd.training.kv_trainer import KVTrainer
    tr = KVTrainer(_model(), _Batches(gold), opt_kwargs={})
    eng = tr.engine
    assert "Optimizer: rmsprop" in capsys.readouterr().out
    assert (eng.optimizer, eng.lr, eng.weight_decay, eng.max_norm) == ("rmsprop", 1e-3, 0.0, None)
    losses, step_kv = [], eng.step_kv

    def recording(*args, **kw):
        loss = step_kv(*args, **kw)
        losses.append(loss.clone())
        return loss

    eng.step_kv = recording
    hist = tr.fit(None, 1, 2)
    third = eng.step_kv(gold)
    torch.cuda.synchronize()
    losses = torch.stack(losses).cpu().double()
    print(losses[:, 0].tolist(), hist[0]["train"]["loss"], hist[0]["val"]["loss"])
    assert len(hist) == 1 and losses.shape[0] == 3 and bool(torch.isfinite(losses).all())
    assert eng.lr == 1e-3 and float(eng.state[0]) == 3.0
    assert float(third[0]) < float(losses[0, 0])


# ---- 9: the checkpoint round trip carries the new state ------------------------------------------------------------------------------
def test_checkpoint_round_trip_of_an_rmsprop_engine(canvases, tmp_path):
    import types
    from msau_amd.training import load_checkpoint, save_checkpoint
    ids, lab, aux, sizes = canvases
    m = _model(deterministic=True)
    eng = TrainEngine(m, lr=LR, optimizer="rmsprop", weight_decay=0.01, max_norm=None)
    step = lambda e: e.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes)
    step(eng)
    args = types.SimpleNamespace(ckptdir=str(tmp_path), bmname=None, dataset="kv", method="msau", hidden_dim=20, output_dim=20)
    path = save_checkpoint(m, eng, args, num_epochs=1)
    m2 = _model(deterministic=True, seed=5)
    eng2 = TrainEngine(m2, lr=1.0, optimizer="rmsprop")
    ck = load_checkpoint(path, model=m2, optimizer=eng2)
    assert ck["optimizer_state"]["optimizer"] == "rmsprop" and ck["optimizer"] is None
    assert torch.equal(eng2.square_avg, eng.square_avg) and float(eng2.state[0]) == 1.0
    assert (eng2.lr, eng2.weight_decay, eng2._clip()) == (LR, 0.01, 0.0)
    l1, l2 = step(eng), step(eng2)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(m._flat, m2._flat) and torch.equal(eng.square_avg, eng2.square_avg)
