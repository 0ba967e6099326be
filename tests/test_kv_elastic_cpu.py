"""CPU: the elastic augmentation of key-value training -- `kv_warp.elastic_host` (the float64 statement) against the generator's
procedure restated with scipy itself, `bytescale` / `elastic_field` and the fixture of its fields, the kernel of csrc/warp.hip
built as plain C++ (-DMSAU_WARP_CPU: `msau_kv_elastic_train_cpu`, the same phases, lanes one after another) against the statement,
`KVTrainBatches(..., imresize="pillow")` and the refusal of a mixed group by `step_kv`."""
import ctypes as C
import dataclasses
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from msau_amd import _lib as L
from msau_amd import TrainEngine
from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import elastic_util as U
from tests import glyphs_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (1) the statement against scipy --------------------------------------------------------------------------------------------------
def _generator_elastic(di, name):
    """image_util.elastic_transform (after its field draw) and data_generator_text.py:326-344 with scipy: one-hot x 255 uint8
    planes, ONE map_coordinates(order=1) call over the 3-D index grid, > 64, the consistency loop"""
    ids, lab, aux = U.painted(di)
    el = U.elastic_of(di, name)
    eye = lambda v, n: np.eye(n, dtype="B")[v]
    image = np.concatenate([eye(ids, U.N_TOKEN), eye(lab, U.N_CLASS), eye(aux, U.N_CLASS)], axis=2) * np.uint8(255)
    shape = image.shape
    x, y, z = np.meshgrid(np.arange(shape[1]), np.arange(shape[0]), np.arange(shape[2]))
    dx = np.dstack([el.field_x] * shape[2]) * el.alpha_x
    dy = np.dstack([el.field_y] * shape[2]) * el.alpha_y
    indices = np.reshape(y + dy, (-1, 1)), np.reshape(x + dx, (-1, 1)), np.reshape(z, (-1, 1))
    res = ndimage.map_coordinates(image, indices, order=1).reshape(shape)
    assert res.dtype == np.uint8
    out = [np.where(res[:, :, :U.N_TOKEN] > 64, 1, 0).astype(np.uint8)]
    for tgt in (res[:, :, U.N_TOKEN:U.N_TOKEN + U.N_CLASS], res[:, :, U.N_TOKEN + U.N_CLASS:]):
        tgt = np.where(tgt > 64, 1.0, 0.0)
        a_map = tgt[:, :, 1]
        for m in range(2, U.N_CLASS):
            t_map = np.logical_and(tgt[:, :, m], np.logical_not(a_map))
            a_map = np.logical_or(a_map, t_map)
            tgt[:, :, m] = t_map
        tgt[:, :, 0] = np.logical_not(a_map)
        assert bool((tgt.sum(axis=2) == 1).all())                             # one-hot now
        out.append(np.argmax(tgt, axis=2).astype(np.int64))
    return out


@pytest.mark.parametrize("di,name", U.cases())
def test_statement_equals_the_generators_scipy_elastic(di, name):
    ref = _generator_elastic(di, name)
    el, want, dist = U.statement(di, name)
    assert int(U.left_out(di, name).sum()) == 0                               # zero pixels are left out
    for what, r, w in zip(("input", "labels", "aux"), ref, want):
        assert r.shape == w.shape and r.dtype == w.dtype, what
        assert np.array_equal(r, w), (what, int((r != w).sum()))
    assert int(want[0].sum(axis=2).max()) <= 3                                # at most three planes of a pixel


def test_the_cases_are_what_they_are_meant_to_be():
    assert U.table(U.BIG).shape == (52, 77) and U.table(4).shape == (44, 91)
    el = U.elastic_of(1, "gen002")
    assert int(el.field_y.max()) == 0 and int(el.field_x.max()) == 0          # a 1 x 1 grid: a zero field
    far = U.elastic_of(4, "gen01")
    assert 112 <= float(far.field_y.max()) * far.alpha_y <= 113 and int(U.statement(4, "gen01")[1][0].sum()) > 0
    for di, name in ((4, "gen0002"), (U.BIG, "gen0002"), (0, "rand0")):       # multi-hot and zero-hot pixels take part
        hot = U.statement(di, name)[1][0].sum(axis=2)
        assert int((hot > 1).sum()) > 0 and int((hot == 0).sum()) > 0
    assert sorted(c for g in U.GROUPS + [U.FAR] for c in g) == sorted(U.cases())      # every case is in one group


def test_zero_alpha_statement_is_the_one_hot_canvas():
    for di in range(6):
        ids, lab, aux = U.painted(di)
        for el in (KW.identity_elastic(ids.shape), dataclasses.replace(U.elastic_of(di, U.case_names(di)[0]), alpha_y=0.0, alpha_x=0.0)):
            hot, wl, wa = KW.elastic_host(ids, lab, aux, el, U.N_TOKEN, U.N_CLASS)
            assert np.array_equal(hot, np.eye(U.N_TOKEN, dtype=np.uint8)[ids]) and np.array_equal(wl, lab) and np.array_equal(wa, aux)


def test_elastic_checks_its_fields():
    z = np.zeros((3, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        KW.Elastic(z.astype(np.int32), z, 0.0, 0.0, (3, 4))
    with pytest.raises(ValueError):
        KW.Elastic(z, z[:2], 0.0, 0.0, (3, 4))
    with pytest.raises(ValueError):
        KW.Elastic(z, z, float("nan"), 0.0, (3, 4))
    with pytest.raises(ValueError):
        KW.elastic_values(np.zeros((4, 4), dtype=np.int32), KW.identity_elastic((3, 4)), [0])


# ---- (3) bytescale and the field draw ---------------------------------------------------------------------------------------------------
def test_bytescale():
    assert np.array_equal(KW.bytescale(np.full((2, 3), 0.37)), np.zeros((2, 3), dtype=np.uint8))          # cscale = 1: all cmin
    two = KW.bytescale(np.array([[-0.5, 0.25], [0.25, -0.5]]))
    assert two.dtype == np.uint8 and np.array_equal(two, [[0, 255], [255, 0]])
    f = np.random.RandomState(3).rand(5, 7) * 2 - 1
    want = np.floor((f - f.min()) * (255.0 / (f.max() - f.min())) + 0.5)
    got = KW.bytescale(f)
    assert np.array_equal(got, want.astype(np.uint8)) and int(got.min()) == 0 and int(got.max()) == 255


def test_elastic_field_draws_dx_then_dy_and_refuses_small_documents(monkeypatch):
    seen = []
    monkeypatch.setattr(KW, "imresize_bicubic", lambda field, shape: (seen.append(np.array(field)), np.zeros(shape, dtype=np.uint8))[1])
    el = KW.elastic_field((52, 77), 0.002, 0.0002, np.random.RandomState(9))
    rs = np.random.RandomState(9)
    sigma = 0.0025 * 52
    dx = ndimage.gaussian_filter(rs.rand(2, 3) * 2 - 1, sigma)
    dy = ndimage.gaussian_filter(rs.rand(2, 3) * 2 - 1, sigma)
    assert len(seen) == 2 and np.array_equal(seen[0], dy) and np.array_equal(seen[1], dx)      # (resized in the record's order: y, x)
    assert el.alpha_x == 0.002 * 52 and el.alpha_y == 0.0002 * 52 and el.out_shape == (52, 77)
    for shape in ((24, 100), (100, 24), (1, 1)):
        with pytest.raises(ValueError):
            KW.elastic_field(shape, 0.0002, 0.0002, np.random.RandomState(0))


# ---- (4) the fixture ----------------------------------------------------------------------------------------------------------------------
def test_regenerated_fields_equal_the_fixture():
    pytest.importorskip("PIL")
    f = U.fixture()
    for k, shape in enumerate(f["shapes"].tolist()):
        el = KW.elastic_field(shape, 0.0002, 0.002, np.random.RandomState(int(f["seed"]) + k))
        assert el.field_y.tobytes() == f[f"fy{k}"].tobytes() and el.field_x.tobytes() == f[f"fx{k}"].tobytes(), shape
        assert el.field_y.dtype == np.uint8 and el.field_y.shape == tuple(shape)
        assert el.alpha_x == 0.0002 * min(shape) and el.alpha_y == 0.002 * min(shape)
    assert int(f["fy1"].max()) == 255 and int(f["fy1"].min()) == 0 and len(np.unique(f["fx2"])) > 50      # bytescaled, then smooth


# ---- (5) the kernel's body as plain C++ -------------------------------------------------------------------------------------------------
GUARD = 64                                                                  # elements of sentinel around every output buffer


@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("elastic_cpu") / "libwarp_cpu.so")
    subprocess.run([cxx, "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-DMSAU_WARP_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "warp.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.msau_kv_elastic_train_ws_ints.restype = C.c_int64

    def run(group, dtype=L.F32, round_to=16, cs=None, alphas=None):
        (ids, lab, aux, sizes), (fields, alph) = U.group_canvases(group)
        alph = alph if alphas is None else np.ascontiguousarray(alphas, dtype=np.float64)
        B, H, W = ids.shape
        Ho, Wo = (-(-int(sizes[:, d].max()) // round_to) * round_to for d in (0, 1))
        Cs = -(-U.N_TOKEN // 8) * 8 if cs is None else cs
        el = np.float32 if dtype == L.F32 else np.uint16
        sentinel = el(7.0) if dtype == L.F32 else el(0x4242)
        grid = np.full(B * Ho * Wo * Cs + 2 * GUARD, sentinel, dtype=el)
        lab_o, aux_o = (np.full(B * Ho * Wo + 2 * GUARD, -77, dtype=np.int64) for _ in range(2))
        n_ws = int(lib.msau_kv_elastic_train_ws_ints(B, Ho, Wo))
        flags, ws = np.full(B + 2 * GUARD, -77, dtype=np.int32), np.full(n_ws + 2 * GUARD, -77, dtype=np.int32)
        ssz = sizes.astype(np.int32)
        p = lambda a, skip=0: C.c_void_p(a.ctypes.data + skip * a.itemsize)
        rc = lib.msau_kv_elastic_train_cpu(C.c_int(dtype), p(ids), p(lab), p(aux), p(ssz), p(fields), p(alph), B, H, W, Ho, Wo, U.N_TOKEN,
                                           Cs, U.N_CLASS, p(grid, GUARD), p(lab_o, GUARD), p(aux_o, GUARD), p(flags, GUARD), p(ws, GUARD))
        assert rc == 0
        for buf, fill in ((grid, sentinel), (lab_o, -77), (aux_o, -77), (flags, -77), (ws, -77)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())      # the guard bands
        inner = lambda a: a[GUARD:-GUARD]
        if dtype != L.F32:
            g16 = inner(grid)
            assert bool(np.isin(g16, (0, 0x3f80)).all())                    # every sentinel is gone
            grid_v = (g16 == 0x3f80).astype(np.float32)
        else:
            grid_v = inner(grid)
        return (grid_v.reshape(B, Ho, Wo, Cs), inner(lab_o).reshape(B, Ho, Wo), inner(aux_o).reshape(B, Ho, Wo), inner(flags),
                inner(ws))

    return run


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("gi", range(len(U.GROUPS)))
def test_cpu_form_of_kernel_ragged_groups(cpu_kernel, gi, dtype):
    group = U.GROUPS[gi]
    got = cpu_kernel(group, L.F32 if dtype == "fp32" else L.BF16)
    assert bool((got[3] == 0).all()) and bool((got[4] == 0).all())          # no flag, no tile's word
    for b, (di, name) in enumerate(group):
        U.assert_document(got, b, di, name)


def test_cpu_form_of_kernel_112_pixels_wide_channels_and_tight_canvas(cpu_kernel):
    got = cpu_kernel(U.FAR)
    assert int(got[3][0]) == 0
    U.assert_document(got, 0, *U.FAR[0])
    cs = -(-U.N_TOKEN // 8) * 8 + 16                                        # Cs larger than n_token: two more groups of zeros
    got = cpu_kernel(U.GROUPS[0], cs=cs)
    assert got[0].shape[-1] == cs
    for b, (di, name) in enumerate(U.GROUPS[0]):
        U.assert_document(got, b, di, name)
    for di, name in ((0, "rand0"), (3, "int"), (U.BIG, "gen002")):          # a document alone on a canvas of its own shape
        got = cpu_kernel([(di, name)], round_to=1)
        assert got[0].shape[1:3] == U.table(di).shape and int(got[3][0]) == 0
        U.assert_document(got, 0, di, name)


def test_cpu_form_of_kernel_flags_an_alpha_that_is_not_finite(cpu_kernel):
    group = U.GROUPS[2]
    (_, _, _, _), (_, alphas) = U.group_canvases(group)
    for bad, col, value in ((1, 0, float("nan")), (0, 1, float("inf")), (2, 1, -float("inf"))):
        a = alphas.copy()
        a[bad, col] = value
        grid, gl, ga, flags, _ = cpu_kernel(group, alphas=a)
        h, w = U.table(group[bad][0]).shape
        assert [int(f != 0) for f in flags] == [int(b == bad) for b in range(len(group))] and int(flags[bad]) == 2
        assert float(np.abs(grid[bad]).sum()) == 0.0 and bool((gl[bad, :h, :w] == 0).all()) and bool((ga[bad, :h, :w] == 0).all())
        assert bool((gl[bad, h:] == -1).all()) and bool((gl[bad, :, w:] == -1).all())
        for b, (di, name) in enumerate(group):
            if b != bad:
                U.assert_document((grid, gl, ga), b, di, name)


# ---- (6) KVTrainBatches -----------------------------------------------------------------------------------------------------------------
PATHS = [os.path.join(GU.KV, f"layout{di}.json") for di in range(3)]
CHARSET = os.path.join(GU.KV, "charset.txt")
FIELDS = ("shape", "scale", "v_scale", "h_scale", "pad", "lines", "reason")
ARRAYS = ("tokens", "label_rec", "line_rec", "glyph_rec")


def _same_table(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in FIELDS) and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ARRAYS)


def test_batches_refuse_elastic_without_imresize_and_with_other_warps():
    with pytest.raises(NotImplementedError, match="imresize"):
        D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, kwargs_dat={"elastic_tr": True})
    with pytest.raises(ValueError, match="imresize"):
        D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, kwargs_dat={"elastic_tr": True}, imresize="scipy")
    with pytest.raises(ValueError, match="imresize"):
        D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, imresize="PIL")
    for other in ("affine_tr", "rotate_tr", "rotateMod90_tr", "elastic_val"):
        with pytest.raises(NotImplementedError):
            D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, kwargs_dat={"elastic_tr": True, other: True}, imresize="pillow")


def test_batches_without_flags_take_no_draw_with_imresize():
    plain = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, seed=3)
    named = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, seed=3, kwargs_dat={"elastic_tr": False, "elastic_val_x": 0.01}, imresize="pillow")
    for _ in range(3):
        for a, b in zip(next(plain), next(named)):
            assert _same_table(a, b) and a.warp is None and b.warp is None
    assert plain.rng.getstate() == named.rng.getstate()


def test_batches_with_elastic_take_one_more_draw_per_document():
    pytest.importorskip("PIL")
    kw = {"elastic_tr": True, "elastic_val_x": 0.002, "elastic_value_y": 0.0007, "elastic_value_x": 0.5, "elastic_val_y": 0.5}
    it = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=4, shuffle=False, kwargs_dat=kw, imresize="pillow")
    rng = random.Random(4)
    tok_to_id, blank, n_token = D.load_charset(CHARSET)
    for a, path in zip(next(it), PATHS):
        ref = D.train_table(path, tok_to_id, blank, n_token, U.N_CLASS, 2.0, 4.0, 0.1, rng)
        want = KW.elastic_field(ref.shape, 0.002, 0.0007, np.random.RandomState(rng.getrandbits(32)))      # one draw, after the table's own
        assert _same_table(a, ref) and isinstance(a.warp, KW.Elastic) and a.warp.out_shape == ref.shape
        assert np.array_equal(a.warp.field_y, want.field_y) and np.array_equal(a.warp.field_x, want.field_x)
        assert (a.warp.alpha_y, a.warp.alpha_x) == (0.0007 * min(ref.shape), 0.002 * min(ref.shape))       # the generator's two spellings
    assert it.rng.getstate() == rng.getstate()
    mk = lambda: D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=11, kwargs_dat={"elastic_tr": True}, imresize="pillow")
    one, two = next(mk()), next(mk())                                       # a seeded run repeats
    assert all(np.array_equal(t.warp.field_y, u.warp.field_y) and np.array_equal(t.warp.field_x, u.warp.field_x) for t, u in zip(one, two))
    assert all(t.warp.alpha_x == 0.0002 * min(t.shape) == t.warp.alpha_y for t in one) and int(one[0].warp.field_y.max()) == 255


def test_batches_small_document_keeps_no_warp_but_takes_its_draw(monkeypatch):
    it = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 1, seed=5, shuffle=False, kwargs_dat={"elastic_tr": True}, imresize="pillow")
    small = U.table(0)                                                      # 23 x 31: under 25 pixels
    monkeypatch.setattr(it, "table", lambda path: dataclasses.replace(small))
    before = random.Random()
    before.setstate(it.rng.getstate())
    got = next(it)[0]
    assert got.warp is None and got.shape == (23, 31)
    before.getrandbits(32)
    assert it.rng.getstate() == before.getstate()                           # exactly one draw


# ---- (7) step_kv ----------------------------------------------------------------------------------------------------------------------------
def test_step_kv_refuses_a_mixed_group_on_the_host():
    eng = TrainEngine.__new__(TrainEngine)                                    # no GPU here: the method only reaches its first lines
    eng.use_graph = False
    t = U.table(0)
    mixed = [dataclasses.replace(t, warp=KW.identity_warp(t.shape)), dataclasses.replace(t, warp=KW.identity_elastic(t.shape)), t]
    with pytest.raises(ValueError, match="mixes"):
        eng.step_kv(mixed)


# ---- (8) the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name, proto in (("msau_kv_elastic_train", "int msau_kv_elastic_train("),
                        ("msau_kv_elastic_train_ws_ints", "int64_t msau_kv_elastic_train_ws_ints(")):
        assert name in L.EXPORTED_SYMBOLS and proto in header, name
    lib = L.load()
    assert lib.msau_kv_elastic_train is not None and int(lib.msau_version()) == 11
    assert int(lib.msau_kv_elastic_train_ws_ints(3, 33, 16)) == 3 * 3 * 1
