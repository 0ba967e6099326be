"""CPU: the host side of the device optimisers (msau_optim_step): the mapping of the reference's get_optimizer options onto
TrainEngine, the conversion of torch.optim state dicts to the flat buffers, the KVTrainer switch, the ABI's additions and its
argument checks (which return before anything is launched)."""
import ctypes as C
import os
import re

import pytest
import torch

from msau_amd import _lib as L
from msau_amd import model as M
from msau_amd.model import MSAUWrapper
from msau_amd.training.optimizer import engine_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(scale_space_num=3, res_depth=2, featRoot=8, final_act="softmax", seed=1)


# ---- from_opt_kwargs' mapping: every branch of get_optimizer -------------------------------------------------------------------
def test_engine_options_follow_get_optimizer():
    assert engine_options({}) == {"optimizer": "rmsprop", "lr": 1e-3, "weight_decay": 0.0, "max_norm": None, "shown": ("rmsprop", "0.001")}
    assert engine_options({"optimizer": "rmsprop", "learning_rate": 5e-4, "lr_decay_rate": 0.01}) == \
        {"optimizer": "rmsprop", "lr": 5e-4, "weight_decay": 0.01, "max_norm": None, "shown": ("rmsprop", "0.0005")}
    # "momentum": SGD with the momentum option (0.9 by default); the other kinds do not take it
    assert engine_options({"optimizer": "momentum"}) == \
        {"optimizer": "momentum", "lr": 1e-3, "weight_decay": 0.0, "momentum": 0.9, "max_norm": None, "shown": ("momentum", "0.001")}
    assert engine_options({"optimizer": "momentum", "momentum": 0.5, "lr_decay_rate": 0.1})["momentum"] == 0.5
    assert "momentum" not in engine_options({"momentum": 0.5})
    # any other name is Adam, with the name printed as given
    for name in ("adam", "Adam", "adagrad", None):
        assert engine_options({"optimizer": name, "learning_rate": 2e-3, "lr_decay_rate": 0.3}) == \
            {"optimizer": "adam", "lr": 2e-3, "weight_decay": 0.3, "max_norm": None, "shown": (name, "0.002")}
    # no learning rate: torch.optim.Adam(parameters), i.e. torch's own defaults, the weight decay dropped with the rate
    assert engine_options({"optimizer": "adam", "learning_rate": None, "lr_decay_rate": 0.3}) == \
        {"optimizer": "adam", "lr": 1e-3, "weight_decay": 0.0, "max_norm": None, "shown": ("adam", "")}
    for name in ("rmsprop", "momentum"):                       # (torch refuses lr=None for them)
        with pytest.raises(ValueError, match="learning_rate"):
            engine_options({"optimizer": name, "learning_rate": None})
    # the mapped options are constructor keywords of the engine
    import inspect
    params = inspect.signature(M.TrainEngine.__init__).parameters
    for kw in ("optimizer", "weight_decay", "alpha", "momentum"):
        assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert set(engine_options({"optimizer": "momentum"})) - {"shown"} <= set(params)
    assert params["optimizer"].default == "adam" and params["weight_decay"].default == 0.0 and params["max_norm"].default == 1.0


# ---- torch.optim state dicts -> flat buffers ------------------------------------------------------------------------------------
def _stepped(kind):
    """a model, a CPU copy of its parameter list and a torch optimiser that stepped twice on it, the dead parameters without a
    gradient"""
    m = MSAUWrapper(13, 5, dict(KW))
    ps = [p.detach().clone().requires_grad_() for _, p in m._named]
    opt = {"rmsprop": lambda: torch.optim.RMSprop(ps, lr=2e-3, alpha=0.9, eps=1e-6, weight_decay=0.01),
           "momentum": lambda: torch.optim.SGD(ps, lr=3e-3, momentum=0.8, weight_decay=0.02),
           "adam": lambda: torch.optim.Adam(ps, lr=4e-3)}[kind]()
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        for (key, _p), q in zip(m._named, ps):
            q.grad = None if key in m._dead else torch.randn(q.shape, generator=gen)
        opt.step()
    return m, ps, opt


@pytest.mark.parametrize("kind", ["rmsprop", "momentum", "adam"])
def test_torch_state_to_flat(kind):
    m, ps, opt = _stepped(kind)
    sd = opt.state_dict()
    named = [(k, p.numel()) for k, p in m._named]
    assert M.torch_optim_kind(sd) == kind
    step, flats, g0 = M.torch_optim_state_to_flat(sd, named, m._poff, m._flat.numel(), kind)
    names = M.OPTIM_BUFFERS[kind]
    assert len(flats) == len(names) and all(f.dtype == torch.float32 and f.numel() == m._flat.numel() and not f.is_cuda for f in flats)
    assert step == (0 if kind == "momentum" else 2)            # (SGD keeps no step count)
    assert g0["lr"] == {"rmsprop": 2e-3, "momentum": 3e-3, "adam": 4e-3}[kind]
    covered = torch.zeros(m._flat.numel(), dtype=torch.bool)
    n_dead = 0
    for (key, p), q in zip(m._named, ps):
        off, n = m._poff[key], p.numel()
        covered[off:off + n] = True
        for name, flat in zip(names, flats):
            if key in m._dead:
                assert q not in opt.state and float(flat[off:off + n].abs().max()) == 0.0, key
            else:
                assert torch.equal(flat[off:off + n], opt.state[q][name].reshape(-1)), (key, name)
                assert float(flat[off:off + n].abs().max()) > 0, (key, name)
        n_dead += key in m._dead
    assert n_dead == len(m._dead) > 0
    assert all(float(f[~covered].abs().max()) == 0.0 for f in flats if bool((~covered).any()))


def test_torch_state_errors():
    m, ps, opt = _stepped("rmsprop")
    named = [(k, p.numel()) for k, p in m._named]
    sd = opt.state_dict()
    for other in ("adam", "momentum"):
        with pytest.raises(ValueError, match="engine runs"):
            M.torch_optim_state_to_flat(sd, named, m._poff, m._flat.numel(), other)
    with pytest.raises(ValueError, match="covers"):
        M.torch_optim_state_to_flat(sd, named[:-1], m._poff, m._flat.numel(), "rmsprop")
    wrong = [(k, n + 1) if i == 0 else (k, n) for i, (k, n) in enumerate(named)]
    with pytest.raises(ValueError, match="elements"):
        M.torch_optim_state_to_flat(sd, wrong, m._poff, m._flat.numel(), "rmsprop")
    # the variants the kernel does not implement
    q = [torch.zeros(3, requires_grad=True)]
    for bad in (torch.optim.RMSprop(q, momentum=0.5), torch.optim.RMSprop(q, centered=True), torch.optim.SGD(q, lr=0.1, momentum=0.9, nesterov=True),
                torch.optim.SGD(q, lr=0.1, momentum=0.9, dampening=0.5)):
        with pytest.raises(ValueError, match="implements"):
            M.torch_optim_kind(bad.state_dict())
    with pytest.raises(ValueError, match="unknown kind"):
        M.torch_optim_kind(torch.optim.Adagrad(q).state_dict())


def test_skip_ranges_of_the_dead_parameters():
    m = MSAUWrapper(64, 5, dict(scale_space_num=4, res_depth=2, featRoot=8, final_act="softmax"))
    numel = {k: p.numel() for k, p in m._named}
    ranges = M.skip_ranges(m._dead, m._poff, numel)
    assert 1 <= len(ranges) <= L.OPTIM_MAX_SKIP
    inside = torch.zeros(m._flat.numel(), dtype=torch.bool)
    last = 0
    for b, e in ranges:
        assert last <= b < e <= m._flat.numel() and (b != last or last == 0)       # ascending, apart, merged where adjacent
        inside[b:e] = True
        last = e
    for key, p in m._named:
        assert bool(inside[m._poff[key]:m._poff[key] + p.numel()].all()) == (key in m._dead), key
    assert M.skip_ranges([], m._poff, numel) == []
    assert M.skip_ranges(["a", "c", "b"], {"a": 0, "b": 4, "c": 12}, {"a": 3, "b": 4, "c": 1}) == [(0, 8), (12, 16)]


# ---- KVTrainer's switch ---------------------------------------------------------------------------------------------------------------
def test_kv_trainer_opt_kwargs_switch():
    from msau_amd.training.kv_trainer import KVTrainer
    made = []

    class Stubbed(KVTrainer):
        def _engine(self, kwargs):
            made.append(("engine", kwargs))
            return "default engine"

        def _engine_from_opt(self, opt_kwargs, kwargs):
            made.append(("opt", opt_kwargs, kwargs))
            return "reference optimiser"

    assert Stubbed("model", "batches", engine_kwargs={"max_norm": 2.0}).engine == "default engine"
    assert Stubbed("model", "batches", opt_kwargs=None).engine == "default engine"
    assert Stubbed("model", "batches", opt_kwargs={}).engine == "reference optimiser"
    assert Stubbed("model", "batches", engine_kwargs={"use_graph": False}, opt_kwargs={"optimizer": "momentum"}).engine == "reference optimiser"
    assert made == [("engine", {"max_norm": 2.0}), ("engine", {}), ("opt", {}, {}), ("opt", {"optimizer": "momentum"}, {"use_graph": False})]

    # the un-stubbed route ends in TrainEngine.from_opt_kwargs, which prints the reference's two lines before it builds the engine
    # (and refuses a model that is not on a GPU)
    class Model:
        _flat = torch.zeros(4)

    with pytest.raises(RuntimeError, match="GPU"):
        KVTrainer(Model(), "batches", opt_kwargs={"optimizer": "momentum"})


def test_from_opt_kwargs_prints_the_references_lines(capsys):
    with pytest.raises(RuntimeError, match="GPU"):
        M.TrainEngine.from_opt_kwargs(MSAUWrapper(13, 5, dict(KW)), {"learning_rate": 0.002})
    assert capsys.readouterr().out == "Optimizer: rmsprop\nLearning Rate: 0.002\n"
    with pytest.raises(ValueError, match="optimizer"):
        M.TrainEngine(MSAUWrapper(13, 5, dict(KW)), optimizer="adagrad")


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_additions():
    lib = L.load()
    assert lib.msau_version() == 11
    hdr = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    assert L._SIGNATURES["msau_optim_ws_floats"] == (C.c_int64, [C.c_int64])
    assert L._SIGNATURES["msau_optim_step"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int64, C.c_float, C.c_double, C.c_double]
                                                + [C.c_float] * 4 + [C.c_void_p, C.c_int])
    decl = re.search(r"int msau_optim_step\((.*?)\);", hdr, re.S).group(1)
    kinds = [" ".join(a.split()[:-1]) for a in decl.replace("\n", " ").split(",")]
    assert kinds == ["void*", "int", "float*", "const float*", "float*", "float*", "float*", "float*", "int64_t", "float", "double", "double"] + ["float"] * 4 + \
        ["const int64_t*", "int"]
    assert re.search(r"int64_t msau_optim_ws_floats\(int64_t n\);", hdr)
    for name, value in (("ADAM", L.OPTIM_ADAM), ("RMSPROP", L.OPTIM_RMSPROP), ("MOMENTUM", L.OPTIM_MOMENTUM), ("MAX_SKIP", L.OPTIM_MAX_SKIP)):
        assert re.search(rf"#define MSAU_OPTIM_{name} {value}\b", hdr), name
    assert hasattr(lib, "msau_optim_step") and hasattr(lib, "msau_clip_adam_step")
    # the workspace: one partial sum of squares per workgroup of the first launch, at most 128
    assert [int(lib.msau_optim_ws_floats(n)) for n in (0, 1, 256, 257, 128 * 256, 128 * 256 + 1, 1 << 24)] == [0, 1, 1, 2, 128, 128, 128]


def test_argument_errors_return_a_status():
    """every one of them is found before the first launch: no device is needed, the buffers are never touched"""
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)

    def call(kind=L.OPTIM_RMSPROP, p=ptr, g=ptr, a=ptr, b=None, state=ptr, ws=ptr, n=64, max_norm=0.0, ranges=(), n_skip=None, null_skip=False):
        arr = (C.c_int64 * max(2 * len(ranges), 1))(*[v for r in ranges for v in r])
        return L.load().msau_optim_step(None, kind, p, g, a, b, state, ws, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, max_norm, 1.0,
                                        None if null_skip else arr, len(ranges) if n_skip is None else n_skip)

    def refused(match, **kw):
        assert call(**kw) != 0
        msg = L.load().msau_last_error().decode()
        assert match in msg, msg

    refused("unknown kind", kind=3)
    refused("unknown kind", kind=-1)
    for name in ("p", "g", "a", "state"):
        refused("null", **{name: None})
    refused("null", n=0)
    refused("state_b", kind=L.OPTIM_ADAM, b=None)
    refused("workspace", ws=None, max_norm=1.0)
    refused("workspace", kind=L.OPTIM_ADAM, b=ptr, ws=None)
    refused("skip ranges", n_skip=L.OPTIM_MAX_SKIP + 1, ranges=[(i, i + 1) for i in range(L.OPTIM_MAX_SKIP + 1)])
    refused("skip ranges", n_skip=-1)
    refused("skip ranges", n_skip=1, null_skip=True)
    refused("reversed", ranges=[(10, 5)])
    refused("reversed", ranges=[(5, 5)])
    refused("reversed", ranges=[(-1, 5)])
    refused("beyond n", ranges=[(60, 65)])
    refused("overlaps", ranges=[(0, 10), (9, 20)])
    refused("overlaps", ranges=[(20, 30), (0, 10)])
    with pytest.raises(L.MsauHipError, match="unknown kind"):
        L.call("msau_optim_step", None, 7, ptr, ptr, ptr, None, ptr, ptr, 64, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, None, 0)
