"""GPU: the warp kernel (msau_kv_warp_train) against the float64 statement `kv_warp.warp_host`, `TrainEngine.step_unet_nhwc`
against `step_unet`, and `step_kv` on tables that carry a warp: the identity against no warp, warped tables against the statement's
arrays -- all bit for bit."""
import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import warp_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = U.N_TOKEN, U.N_CLASS
CS = -(-CH // 8) * 8
KWARGS = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
CW = [0.0, 2.0] + [0.5 + 0.1 * c for c in range(NCLS - 2)]
GUARD = 64
DOCS = [0, 1, 2, 3]
MIXED = ["rot13.7", "affine100", "rot-20", "rot-45"]                        # the warp of every document of the stepped group


def _model(dtype="fp32"):
    return MSAUWrapper(CH, NCLS, dict(KWARGS, dtype=dtype, deterministic=True)).to(DEV)


# ---- (e) the kernel against the statement ---------------------------------------------------------------------------------------------
def _launch(names, dtype, tables=None, warps=None):
    """the group DOCS, document b warped by names[b] (or `tables` under `warps`), through msau_kv_warp_train into sentinel-filled
    buffers with a guard band"""
    if tables is None:
        tables = [U.table(di) for di in DOCS]
        warps = [U.statement(di, n)[0] for di, n in zip(DOCS, names)]
    ids, lab, aux, sizes = (torch.from_numpy(a) for a in U.group_canvases(tables))
    B, H, W = ids.shape
    dsz, (Ho, Wo) = KW.warped_canvas(warps)
    td = torch.float32 if dtype == L.F32 else torch.bfloat16
    grid = torch.full((B * Ho * Wo * CS + 2 * GUARD,), 7.0, dtype=td, device=DEV)
    lab_o, aux_o = (torch.full((B * Ho * Wo + 2 * GUARD,), -77, dtype=torch.int64, device=DEV) for _ in range(2))
    n_ws = int(L.load().msau_kv_warp_train_ws_ints(B, Ho, Wo))
    flags = torch.full((B + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    ws = torch.full((n_ws + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    rec = torch.from_numpy(np.stack([w.record() for w in warps])).to(DEV)
    ssz, dsz_d = sizes.to(torch.int32).to(DEV), torch.from_numpy(dsz.astype(np.int32)).to(DEV)
    ids_d, lab_d, aux_d = ids.to(DEV), lab.to(DEV), aux.to(DEV)
    at = lambda t: t.data_ptr() + GUARD * t.element_size()
    L.call("msau_kv_warp_train", torch.cuda.current_stream().cuda_stream, dtype, ids_d.data_ptr(), lab_d.data_ptr(), aux_d.data_ptr(),
           ssz.data_ptr(), rec.data_ptr(), dsz_d.data_ptr(), B, H, W, Ho, Wo, CH, CS, NCLS, at(grid), at(lab_o), at(aux_o), at(flags), at(ws))
    torch.cuda.synchronize()
    for buf, fill in ((grid, 7.0), (lab_o, -77), (aux_o, -77), (flags, -77), (ws, -77)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())          # the guard bands
    inner = lambda t: t[GUARD:-GUARD].cpu()
    return (inner(grid).float().reshape(B, Ho, Wo, CS).numpy(), inner(lab_o).reshape(B, Ho, Wo).numpy(),
            inner(aux_o).reshape(B, Ho, Wo).numpy(), inner(flags).numpy(), inner(ws).numpy())


def _assert_document(got, b, di, name):
    grid, lab, aux = got[:3]
    warp, want, _ = U.statement(di, name)
    ho, wo = warp.out_shape
    skip = U.left_out(di, name, U.KERNEL_MARGIN)
    assert int(skip.sum()) <= U.KERNEL_CAP * ho * wo, (di, name)            # from the statement alone
    keep = ~skip
    assert bool(np.isin(grid[b], (0.0, 1.0)).all())                         # every sentinel is gone
    assert np.array_equal(grid[b, :ho, :wo, :CH][keep], want[0][keep].astype(np.float32)), (di, name)
    assert np.array_equal(lab[b, :ho, :wo][keep], want[1][keep]) and np.array_equal(aux[b, :ho, :wo][keep], want[2][keep]), (di, name)
    outside = np.ones(grid.shape[1:3], dtype=bool)
    outside[:ho, :wo] = False
    assert float(np.abs(grid[b][outside]).sum()) == 0.0 and float(np.abs(grid[b, :, :, CH:]).sum()) == 0.0
    assert bool((lab[b][outside] == -1).all()) and bool((aux[b][outside] == -1).all())
    assert bool((lab[b, :ho, :wo] >= 0).all()) and bool((aux[b, :ho, :wo] >= 0).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kernel_equals_statement(dtype):
    dt = L.F32 if dtype == "fp32" else L.BF16
    for names in [[n] * 4 for n in U.WARP_NAMES] + [MIXED]:
        got = _launch(names, dt)
        assert bool((got[3] == 0).all()) and bool((got[4] == 0).all()), names                  # all flags zero
        for b, (di, n) in enumerate(zip(DOCS, names)):
            _assert_document(got, b, di, n)


def test_kernel_reads_the_canvases_when_the_footprint_is_wide():
    """the path without the LDS tile (tests/warp_util.py: wide_case)"""
    t, warp, want, keep = U.wide_case()
    grid, gl, ga, flags, _ = _launch(None, L.F32, [t], [warp])
    ho, wo = warp.out_shape
    assert int(flags[0]) == 0 and bool(np.isin(grid, (0.0, 1.0)).all())
    assert np.array_equal(grid[0, :ho, :wo, :CH][keep], want[0][keep].astype(np.float32))
    assert np.array_equal(gl[0, :ho, :wo][keep], want[1][keep]) and np.array_equal(ga[0, :ho, :wo][keep], want[2][keep])
    assert bool((gl[0, ho:] == -1).all()) and bool((gl[0, :, wo:] == -1).all()) and float(np.abs(grid[0, ho:]).sum()) == 0.0


# ---- (f) the NHWC step ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def canvases():
    """the hand-made group on one canvas as CPU tensors (ids, labels, aux, sizes); shared and left unchanged"""
    return tuple(torch.from_numpy(a) for a in U.group_canvases([U.table(di) for di in DOCS]))


def _one_hot_grid(ids, td, junk_outside_sizes=None):
    """[B, H, W, CS] in the storage dtype: the one-hot grid of an id canvas (-1: no channel)"""
    B, H, W = ids.shape
    grid = torch.zeros((B, H, W, CS), dtype=torch.float32)
    inside = ids >= 0
    grid[inside] = torch.nn.functional.one_hot(ids[inside].long(), CS).float()
    if junk_outside_sizes is not None:                                      # what lies outside the documents must not matter
        for b, (h, w) in enumerate(junk_outside_sizes.tolist()):
            grid[b, h:] = 3.0
            grid[b, :, w:] = -2.0
    return grid.to(td)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_unet_nhwc_equals_step_unet_on_ids(canvases, dtype, weighted):
    ids, lab, aux, sizes = canvases
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    cw = CW if weighted else None
    a, b = TrainEngine(_model(dtype)), TrainEngine(_model(dtype))
    grid = _one_hot_grid(ids, td, sizes).to(DEV)
    for _ in range(2):
        la = a.step_unet(ids.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw)
        lb = b.step_unet_nhwc(grid, lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and bool(torch.isfinite(a.model._flat).all())
    with pytest.raises(ValueError, match="step_unet_nhwc wants"):
        b.step_unet_nhwc(grid[..., :8], lab.to(DEV), aux.to(DEV), sizes=sizes)
    with pytest.raises(RuntimeError, match="eager"):
        TrainEngine(_model(dtype), use_graph=True).step_unet_nhwc(grid, lab.to(DEV), aux.to(DEV), sizes=sizes)


# ---- (g) the identity warp --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_identity_warp_changes_nothing(dtype):
    plain = [U.table(di) for di in DOCS]
    ident = [U.with_warp(t, KW.identity_warp(t.shape)) for t in plain[:3]] + [plain[3]]       # the last one takes the identity unasked
    a, b = TrainEngine(_model(dtype)), TrainEngine(_model(dtype))
    before = D.STATS["host_warped"]
    for _ in range(2):
        la, lb = a.step_kv(plain), b.step_kv(ident)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and D.STATS["host_warped"] == before


# ---- (h) warped steps -------------------------------------------------------------------------------------------------------------------
def _statement_arrays(names, td):
    """the group warped by `warp_host`, as `step_unet_nhwc` takes it: the grid, both label maps (-1 outside) and the sizes"""
    parts = [U.statement(di, n) for di, n in zip(DOCS, names)]
    sizes, (Ho, Wo) = KW.warped_canvas([p[0] for p in parts])
    grid = torch.zeros((len(parts), Ho, Wo, CS), dtype=torch.float32)
    lab, aux = (torch.full((len(parts), Ho, Wo), -1, dtype=torch.int64) for _ in range(2))
    for b, (warp, want, _) in enumerate(parts):
        ho, wo = warp.out_shape
        grid[b, :ho, :wo, :CH] = torch.from_numpy(want[0].astype(np.float32))
        lab[b, :ho, :wo], aux[b, :ho, :wo] = torch.from_numpy(want[1].copy()), torch.from_numpy(want[2].copy())
    return grid.to(td), lab, aux, torch.from_numpy(sizes)


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_warped_step_kv_equals_the_statement_fed_step(dtype, optimizer):
    for di, n in zip(DOCS, MIXED):
        assert int(U.left_out(di, n, U.KERNEL_MARGIN).sum()) == 0           # a group the kernel must reproduce pixel for pixel
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    tables = [U.with_warp(U.table(di), U.statement(di, n)[0]) for di, n in zip(DOCS, MIXED)]
    grid, lab, aux, sizes = _statement_arrays(MIXED, td)
    assert int((grid.float().sum(dim=-1) > 1).sum()) > 0                    # multi-hot pixels take part
    make = (lambda: TrainEngine(_model(dtype))) if optimizer == "adam" else (lambda: TrainEngine.from_opt_kwargs(_model(dtype), {}))
    a, b = make(), make()
    assert b.optimizer == optimizer
    before = D.STATS["host_warped"]
    for cw in (None, CW):
        la = a.step_kv(tables, class_weights=cw)
        lb = b.step_unet_nhwc(grid.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and bool(torch.isfinite(a.model._flat).all())
    assert D.STATS["host_warped"] == before == 0


def test_flagged_document_is_warped_on_the_host():
    """a matrix that is not finite flags its document: `upload_host_warp` is what step_kv then runs; here on the group's buffers"""
    names = ["identity"] * 4
    tables = [U.table(di) for di in DOCS]
    warps = [U.statement(di, n)[0] for di, n in zip(DOCS, names)]
    bad = KW.Warp(np.array([[1.0, float("inf")], [0.0, 1.0]]), np.zeros(2), tables[1].shape)
    ids, lab, aux, sizes = D.paint_train_device(tables, device=DEV)
    _, (Ho, Wo) = KW.warped_canvas(warps)
    grid = torch.full((4, Ho, Wo, CS), 5.0, device=DEV)
    wl, wa, flags = KW.warp_train_device(ids, lab, aux, sizes, [warps[0], bad, warps[2], warps[3]], grid, CH, NCLS, L.F32)
    assert flags.cpu().tolist() == [0, 2, 0, 0]
    KW.upload_host_warp(1, tables[1], warps[1], grid, wl, wa, CH, NCLS)
    got = (grid.cpu().numpy(), wl.cpu().numpy(), wa.cpu().numpy())
    for b, di in enumerate(DOCS):
        _assert_document(got, b, di, "identity")
