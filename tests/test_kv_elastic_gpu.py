"""GPU: the elastic warp kernel (msau_kv_elastic_train) against the float64 statement `kv_warp.elastic_host` -- exact on every
pixel --, the identity `Elastic` against msau_kv_warp_train under the identity `Warp`, `step_kv` on tables that carry an `Elastic`
against `step_unet_nhwc` on the statement's arrays, and the flag of an alpha that is not finite -- all bit for bit.  The fields come
from tests/golden/kv/elastic_fields.npz: no Pillow is needed here."""
import numpy as np
import pytest
import torch

from msau_amd import _lib as L
from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import elastic_util as U
from tests import warp_util as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, NCLS = U.N_TOKEN, U.N_CLASS
CS = -(-CH // 8) * 8
KWARGS = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3, seed=0)
CW = [0.0, 2.0] + [0.5 + 0.1 * c for c in range(NCLS - 2)]
GUARD = 64


def _model(dtype="fp32"):
    return MSAUWrapper(CH, NCLS, dict(KWARGS, dtype=dtype, deterministic=True)).to(DEV)


def _launch(group, dtype, alphas=None):
    """the group through msau_kv_elastic_train into sentinel-filled buffers with a guard band"""
    (ids, lab, aux, sizes), (fields, alph) = U.group_canvases(group)
    alph = alph if alphas is None else np.ascontiguousarray(alphas, dtype=np.float64)
    B, H, Wd = ids.shape
    Ho, Wo = (-(-int(sizes[:, d].max()) // 16) * 16 for d in (0, 1))
    td = torch.float32 if dtype == L.F32 else torch.bfloat16
    grid = torch.full((B * Ho * Wo * CS + 2 * GUARD,), 7.0, dtype=td, device=DEV)
    lab_o, aux_o = (torch.full((B * Ho * Wo + 2 * GUARD,), -77, dtype=torch.int64, device=DEV) for _ in range(2))
    n_ws = int(L.load().msau_kv_elastic_train_ws_ints(B, Ho, Wo))
    flags = torch.full((B + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    ws = torch.full((n_ws + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ids_d, lab_d, aux_d, ssz, fld, alp = dev(ids), dev(lab), dev(aux), dev(sizes.astype(np.int32)), dev(fields), dev(alph)
    at = lambda t: t.data_ptr() + GUARD * t.element_size()
    L.call("msau_kv_elastic_train", torch.cuda.current_stream().cuda_stream, dtype, ids_d.data_ptr(), lab_d.data_ptr(), aux_d.data_ptr(),
           ssz.data_ptr(), fld.data_ptr(), alp.data_ptr(), B, H, Wd, Ho, Wo, CH, CS, NCLS, at(grid), at(lab_o), at(aux_o), at(flags), at(ws))
    torch.cuda.synchronize()
    for buf, fill in ((grid, 7.0), (lab_o, -77), (aux_o, -77), (flags, -77), (ws, -77)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())          # the guard bands
    inner = lambda t: t[GUARD:-GUARD].cpu()
    return (inner(grid).float().reshape(B, Ho, Wo, CS).numpy(), inner(lab_o).reshape(B, Ho, Wo).numpy(),
            inner(aux_o).reshape(B, Ho, Wo).numpy(), inner(flags).numpy(), inner(ws).numpy())


# ---- (1) the kernel against the statement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kernel_equals_statement(dtype):
    dt = L.F32 if dtype == "fp32" else L.BF16
    for group in U.GROUPS:
        got = _launch(group, dt)
        assert bool((got[3] == 0).all()) and bool((got[4] == 0).all()), group                  # all flags zero
        for b, (di, name) in enumerate(group):
            U.assert_document(got, b, di, name)                             # exact, all pixels kept, every sentinel overwritten


# ---- (2) 112 pixels ---------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_statement_at_112_pixels():
    got = _launch(U.FAR, L.F32)
    assert int(got[3][0]) == 0
    U.assert_document(got, 0, *U.FAR[0])


# ---- (3) the identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_identity_elastic_is_the_identity_warp(dtype):
    dt, td = (L.F32, torch.float32) if dtype == "fp32" else (L.BF16, torch.bfloat16)
    tables = [U.table(di) for di in (0, 1, 2, 3, 4)]
    ids, lab, aux, sizes = D.paint_train_device(tables, device=DEV)
    _, (Ho, Wo) = KW.warped_canvas([KW.identity_warp(t.shape) for t in tables])
    ga, gb = (torch.full((len(tables), Ho, Wo, CS), 5.0, dtype=td, device=DEV) for _ in range(2))
    la, aa, fa = KW.warp_train_device(ids, lab, aux, sizes, [KW.identity_warp(t.shape) for t in tables], ga, CH, NCLS, dt)
    lb, ab, fb = KW.elastic_train_device(ids, lab, aux, sizes, [KW.identity_elastic(t.shape) for t in tables], gb, CH, NCLS, dt)
    torch.cuda.synchronize()
    assert torch.equal(ga.view(torch.int32 if dtype == "fp32" else torch.int16), gb.view(torch.int32 if dtype == "fp32" else torch.int16))
    assert torch.equal(la, lb) and torch.equal(aa, ab) and torch.equal(fa, fb) and fb.cpu().tolist() == [0] * len(tables)
    assert float(gb.float().sum()) == sum(t.shape[0] * t.shape[1] for t in tables)             # one-hot inside, zeros outside


# ---- (4) elastic steps --------------------------------------------------------------------------------------------------------------------
def _statement_arrays(group, td):
    """the group warped by `elastic_host`, as `step_unet_nhwc` takes it: the grid, both label maps (-1 outside) and the sizes"""
    parts = [U.statement(di, n) for di, n in group]
    sizes, (Ho, Wo) = KW.warped_canvas([p[0] for p in parts])
    grid = torch.zeros((len(parts), Ho, Wo, CS), dtype=torch.float32)
    lab, aux = (torch.full((len(parts), Ho, Wo), -1, dtype=torch.int64) for _ in range(2))
    for b, (el, want, _) in enumerate(parts):
        h, w = el.out_shape
        grid[b, :h, :w, :CH] = torch.from_numpy(want[0].astype(np.float32))
        lab[b, :h, :w], aux[b, :h, :w] = torch.from_numpy(want[1].copy()), torch.from_numpy(want[2].copy())
    return grid.to(td), lab, aux, torch.from_numpy(sizes)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_elastic_step_kv_equals_the_statement_fed_step(dtype):
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    group = U.STEPPED[:3] + [(3, "rand4")]                                  # the last document carries no warp: the identity, as rand4 is
    for di, n in group:
        assert int(U.left_out(di, n).sum()) == 0
    tables = [W.with_warp(U.table(di), U.elastic_of(di, n)) for di, n in group[:3]] + [U.table(3)]
    grid, lab, aux, sizes = _statement_arrays(group, td)
    assert int((grid.float().sum(dim=-1) > 1).sum()) > 0                    # multi-hot pixels take part
    a, b = TrainEngine(_model(dtype)), TrainEngine(_model(dtype))
    before = D.STATS["host_warped"]
    for cw in (None, CW):
        la = a.step_kv(tables, class_weights=cw)
        lb = b.step_unet_nhwc(grid.to(DEV), lab.to(DEV), aux.to(DEV), sizes=sizes, class_weights=cw)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.model._flat, b.model._flat)
    assert float(la[0]) > 0 and bool(torch.isfinite(a.model._flat).all())
    assert D.STATS["host_warped"] == before


# ---- (5) the flag ---------------------------------------------------------------------------------------------------------------------------
def test_alpha_that_is_not_finite_flags_its_document_only():
    group = U.GROUPS[2]
    alphas = U.group_canvases(group)[1][1].copy()
    alphas[1, 0] = float("nan")
    grid, gl, ga, flags, _ = _launch(group, L.F32, alphas=alphas)
    h, w = U.table(group[1][0]).shape
    assert flags.tolist() == [0, 2, 0, 0]
    assert float(np.abs(grid[1]).sum()) == 0.0 and bool((gl[1, :h, :w] == 0).all()) and bool((ga[1, :h, :w] == 0).all())
    assert bool((gl[1, h:] == -1).all()) and bool((gl[1, :, w:] == -1).all())
    for b, (di, name) in enumerate(group):
        if b != 1:
            U.assert_document((grid, gl, ga), b, di, name)
