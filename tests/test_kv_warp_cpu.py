"""CPU: the affine / rotation augmentation of key-value training -- `kv_warp.warp_host` (the float64 statement) against the
generator's procedure restated with scipy itself, the geometry of `rotate_warp` / `affine_warp`, the kernel of csrc/warp.hip built
as plain C++ (-DMSAU_WARP_CPU: the same phases, lanes one after another) against the statement, and `KVTrainBatches` with the
generator's augmentation keys."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from msau_amd import _lib as L
from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import glyphs_util as GU
from tests import warp_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [13.7, -20.0, -45.0]


# ---- (a) the statement against scipy ------------------------------------------------------------------------------------------------
def _generator_warp(di, name):
    """data_generator_text.py:303-344 with scipy: one-hot x 255 uint8 planes, warped plane by plane, > 64, the consistency loop"""
    ids, lab, aux = U.painted(di)
    eye = lambda v, n: np.eye(n, dtype="B")[v]
    maps = np.concatenate([eye(ids, U.N_TOKEN), eye(lab, U.N_CLASS), eye(aux, U.N_CLASS)], axis=2) * np.uint8(255)
    warp = U.warp_of(name, ids.shape)
    if name.startswith("rot"):
        res = ndimage.rotate(maps, float(name[3:]))
    else:
        res = maps.copy()
        for d in range(maps.shape[2]):
            res[:, :, d] = ndimage.affine_transform(maps[:, :, d], warp.matrix, offset=warp.offset)
    assert res.dtype == np.uint8
    img = np.where(res[:, :, :U.N_TOKEN] > 64, 1, 0).astype(np.uint8)
    out = [img]
    for tgt in (res[:, :, U.N_TOKEN:U.N_TOKEN + U.N_CLASS], res[:, :, U.N_TOKEN + U.N_CLASS:]):
        tgt = np.where(tgt > 64, 1.0, 0.0)
        a_map = tgt[:, :, 1]
        for m in range(2, U.N_CLASS):
            t_map = np.logical_and(tgt[:, :, m], np.logical_not(a_map))
            a_map = np.logical_or(a_map, t_map)
            tgt[:, :, m] = t_map
        tgt[:, :, 0] = np.logical_not(a_map)
        assert bool((tgt.sum(axis=2) == 1).all())                         # one-hot now
        out.append(np.argmax(tgt, axis=2).astype(np.int64))
    return out


@pytest.mark.parametrize("di,name", U.cases())
def test_statement_equals_the_generators_scipy_warp(di, name):
    ref = _generator_warp(di, name)
    warp, want, dist = U.statement(di, name)
    assert ref[0].shape[:2] == warp.out_shape
    skip = U.left_out(di, name, 1e-6)
    assert int(skip.sum()) == 0                                           # no pixel is left out on these cases
    for what, r, w in zip(("input", "labels", "aux"), ref, want):
        assert r.shape == w.shape and r.dtype == w.dtype, what
        assert np.array_equal(r, w), (what, int((r != w).sum()))
    if name != "identity" and di < 2:
        assert int((want[0].sum(axis=2) > 1).sum()) > 0 and int((want[0].sum(axis=2) == 0).sum()) > 0       # multi-hot and zero-hot


def test_identity_statement_is_the_one_hot_canvas():
    for di in range(5):
        ids, lab, aux = U.painted(di)
        _, (hot, wl, wa), _ = U.statement(di, "identity")
        assert np.array_equal(hot, np.eye(U.N_TOKEN, dtype=np.uint8)[ids]) and np.array_equal(wl, lab) and np.array_equal(wa, aux)


# ---- (b) geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.DOC_SHAPES + [(44, 91)])
def test_rotate_warp_has_scipys_output_shape_and_centres(shape):
    for angle in ANGLES + [0.0, 90.0]:
        warp = KW.rotate_warp(shape, angle)
        got = ndimage.rotate(np.zeros(shape, dtype=np.uint8), angle)
        assert got.shape == warp.out_shape, (shape, angle)
        centre = warp.offset + warp.matrix @ ((np.array(warp.out_shape) - 1) / 2)
        assert np.allclose(centre, (np.array(shape) - 1) / 2, atol=1e-12)                 # the output's centre reads the input's
        assert np.allclose(warp.matrix @ warp.matrix.T, np.eye(2), atol=1e-12)
        # the same plane through scipy's affine_transform with this matrix and offset is scipy's rotation
        plane = (np.arange(shape[0] * shape[1]).reshape(shape) * 37 % 256).astype(np.uint8)
        mine = ndimage.affine_transform(plane, warp.matrix, offset=warp.offset, output_shape=warp.out_shape)
        assert np.array_equal(mine, ndimage.rotate(plane, angle))


def test_affine_warp_maps_its_three_points():
    for shape in [(23, 31), (37, 29), (44, 91)]:
        for value in (0.025, 0.1):
            warp = KW.affine_warp(shape, value, np.random.RandomState(5))
            pts1 = KW.affine_points(shape).astype(np.float64)
            alpha = min(shape) * value
            moved = np.float32(np.random.RandomState(5).uniform(-alpha, alpha, size=(3, 2))).astype(np.float64)
            got = pts1 @ warp.matrix.T + warp.offset
            assert np.abs(got - (pts1 + moved)).max() <= 1e-4                             # (the map is rounded to float32)
            assert warp.out_shape == shape
            assert np.array_equal(warp.matrix, warp.matrix.astype(np.float32).astype(np.float64))
    assert KW.affine_warp((2, 3), 0.1, np.random.RandomState(0)).out_shape == (2, 3)        # coinciding points: still a map
    assert KW.mod90_angle(-3.0) == -45.0 and KW.mod90_angle(17.0) == -45.0


# ---- (c) the kernel's body as plain C++ -----------------------------------------------------------------------------------------------
GUARD = 64                                                                  # elements of sentinel around every output buffer


@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("warp_cpu") / "libwarp_cpu.so")
    subprocess.run([cxx, "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-DMSAU_WARP_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "warp.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.msau_kv_warp_train_ws_ints.restype = C.c_int64

    def run(tables, warps, dtype=L.F32, round_to=16):
        ids, lab, aux, sizes = U.group_canvases(tables)
        B, H, W = ids.shape
        dsz, (Ho, Wo) = KW.warped_canvas(warps, round_to)
        Cs = -(-U.N_TOKEN // 8) * 8
        el = np.float32 if dtype == L.F32 else np.uint16
        sentinel = el(7.0) if dtype == L.F32 else el(0x4242)
        grid = np.full(B * Ho * Wo * Cs + 2 * GUARD, sentinel, dtype=el)
        lab_o, aux_o = (np.full(B * Ho * Wo + 2 * GUARD, -77, dtype=np.int64) for _ in range(2))
        n_ws = int(lib.msau_kv_warp_train_ws_ints(B, Ho, Wo))
        flags, ws = np.full(B + 2 * GUARD, -77, dtype=np.int32), np.full(n_ws + 2 * GUARD, -77, dtype=np.int32)
        rec = np.ascontiguousarray(np.stack([w.record() for w in warps]))
        ssz, dsz32 = sizes.astype(np.int32), dsz.astype(np.int32)
        p = lambda a, skip=0: C.c_void_p(a.ctypes.data + skip * a.itemsize)
        rc = lib.msau_kv_warp_train_cpu(C.c_int(dtype), p(ids), p(lab), p(aux), p(ssz), p(rec), p(dsz32), B, H, W, Ho, Wo, U.N_TOKEN, Cs,
                                        U.N_CLASS, p(grid, GUARD), p(lab_o, GUARD), p(aux_o, GUARD), p(flags, GUARD), p(ws, GUARD))
        assert rc == 0
        for buf, fill in ((grid, sentinel), (lab_o, -77), (aux_o, -77), (flags, -77), (ws, -77)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())      # the guard bands
        inner = lambda a: a[GUARD:-GUARD]
        if dtype != L.F32:
            g16 = inner(grid)
            assert bool(np.isin(g16, (0, 0x3f80)).all())
            grid_v = (g16 == 0x3f80).astype(np.float32)
        else:
            grid_v = inner(grid)
        return (grid_v.reshape(B, Ho, Wo, Cs), inner(lab_o).reshape(B, Ho, Wo), inner(aux_o).reshape(B, Ho, Wo), inner(flags),
                inner(ws))

    return run


def _assert_document(got, b, di, name):
    """document b of the kernel's outputs against the statement of (di, name); -> the number of pixels left out"""
    grid, lab, aux = got[:3]
    warp, want, _ = U.statement(di, name)
    ho, wo = warp.out_shape
    skip = U.left_out(di, name, U.KERNEL_MARGIN)
    n_skip = int(skip.sum())
    assert n_skip <= U.KERNEL_CAP * ho * wo, (di, name, n_skip)             # from the statement alone
    keep = ~skip
    hot = grid[b, :ho, :wo, :U.N_TOKEN]
    assert bool(np.isin(grid[b], (0.0, 1.0)).all())
    assert np.array_equal(hot[keep], want[0][keep].astype(np.float32)), (di, name, int((hot[keep] != want[0][keep]).sum()))
    assert np.array_equal(lab[b, :ho, :wo][keep], want[1][keep]), (di, name)
    assert np.array_equal(aux[b, :ho, :wo][keep], want[2][keep]), (di, name)
    # outside the warped extent and in the padded channels: zeros and -1, written over the sentinels
    outside = np.ones(grid.shape[1:3], dtype=bool)
    outside[:ho, :wo] = False
    assert float(np.abs(grid[b][outside]).sum()) == 0.0 and float(np.abs(grid[b, :, :, U.N_TOKEN:]).sum()) == 0.0
    assert bool((lab[b][outside] == -1).all()) and bool((aux[b][outside] == -1).all())
    assert bool((lab[b, :ho, :wo] >= 0).all()) and bool((aux[b, :ho, :wo] >= 0).all())
    return n_skip


@pytest.mark.parametrize("name", U.WARP_NAMES)
def test_cpu_form_of_kernel_ragged_group(cpu_kernel, name):
    docs = [0, 1, 2, 3, 4]
    tables = [U.table(di) for di in docs]
    warps = [U.statement(di, name)[0] for di in docs]
    got = cpu_kernel(tables, warps)
    assert bool((got[3] == 0).all()) and bool((got[4] == 0).all())          # no flag, no tile's word
    for b, di in enumerate(docs):
        _assert_document(got, b, di, name)


def test_cpu_form_of_kernel_mixed_warps_bf16_and_dense(cpu_kernel):
    names = ["rot-45", "identity", "rot13.7", "affine100"]
    got = cpu_kernel([U.table(di) for di in range(4)], [U.statement(di, n)[0] for di, n in enumerate(names)], dtype=L.BF16)
    assert bool((got[3] == 0).all())
    for b, n in enumerate(names):
        _assert_document(got, b, b, n)
    for di, n in ((0, "rot-20"), (3, "rot-45"), (2, "affine025")):          # a document alone on its own shape
        got = cpu_kernel([U.table(di)], [U.statement(di, n)[0]], round_to=1)
        assert got[0].shape[1:3] == U.statement(di, n)[0].out_shape and int(got[3][0]) == 0
        _assert_document(got, 0, di, n)


def test_cpu_form_of_kernel_reads_the_canvases_when_the_footprint_is_wide(cpu_kernel):
    """a map that shrinks the output 5-fold: a tile's windows span more than the LDS tile holds, so the kernel reads the canvases;
    the statement's margin is checked like everywhere else"""
    t, warp, want, keep = U.wide_case()
    grid, gl, ga, flags, _ = cpu_kernel([t], [warp])
    ho, wo = warp.out_shape
    assert int(flags[0]) == 0
    assert np.array_equal(grid[0, :ho, :wo, :U.N_TOKEN][keep], want[0][keep].astype(np.float32))
    assert np.array_equal(gl[0, :ho, :wo][keep], want[1][keep]) and np.array_equal(ga[0, :ho, :wo][keep], want[2][keep])


def test_cpu_form_of_kernel_flags(cpu_kernel):
    t = U.table(0)
    bad = KW.Warp(np.array([[1.0, float("nan")], [0.0, 1.0]]), np.zeros(2), t.shape)
    grid, gl, ga, flags, _ = cpu_kernel([t, t], [bad, KW.identity_warp(t.shape)])
    assert int(flags[0]) != 0 and int(flags[1]) == 0                        # a matrix that is not finite: flagged, nothing warped
    assert float(np.abs(grid[0]).sum()) == 0.0 and bool((gl[0, :23, :31] == 0).all())
    _assert_document((grid, gl, ga), 1, 0, "identity")


def test_abi_entry_is_declared():
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name, proto in (("msau_kv_warp_train", "int msau_kv_warp_train("), ("msau_kv_warp_train_ws_ints", "int64_t msau_kv_warp_train_ws_ints(")):
        assert name in L.EXPORTED_SYMBOLS and proto in header, name
    assert "warp.hip" in __import__("msau_amd.build", fromlist=["SOURCES"]).SOURCES


# ---- (d) KVTrainBatches -------------------------------------------------------------------------------------------------------------
PATHS = [os.path.join(GU.KV, f"layout{di}.json") for di in range(3)]
CHARSET = os.path.join(GU.KV, "charset.txt")
FIELDS = ("shape", "scale", "v_scale", "h_scale", "pad", "lines", "reason")
ARRAYS = ("tokens", "label_rec", "line_rec", "glyph_rec")


def _same_table(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in FIELDS) and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ARRAYS)


def test_batches_without_flags_are_todays_tables():
    plain = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, seed=3)
    off = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, seed=3, kwargs_dat={"affine_tr": False, "rotate_tr": False, "affine_value": 0.3})
    # today's iterator, draw by draw: one generator for the order and every table
    rng = random.Random(3)
    tok_to_id, blank, n_token = D.load_charset(CHARSET)
    order = []
    for _ in range(3):
        got_a, got_b = next(plain), next(off)
        for a, b in zip(got_a, got_b):
            if not order:
                order = list(PATHS)
                rng.shuffle(order)
                order.reverse()
            ref = D.train_table(order.pop(), tok_to_id, blank, n_token, U.N_CLASS, 2.0, 4.0, 0.1, rng)
            assert _same_table(a, ref) and _same_table(b, ref) and a.warp is None and b.warp is None
    assert plain.rng.getstate() == off.rng.getstate() == rng.getstate()


def test_batches_with_rotation_take_one_more_draw_per_document():
    rot = D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=4, shuffle=False, kwargs_dat={"rotate_tr": True})
    rng = random.Random(4)
    tok_to_id, blank, n_token = D.load_charset(CHARSET)
    for a, path in zip(next(rot), PATHS):
        ref = D.train_table(path, tok_to_id, blank, n_token, U.N_CLASS, 2.0, 4.0, 0.1, rng)
        angle = rng.uniform(-20, 20)                                        # exactly one draw, after the table's own
        want = KW.rotate_warp(ref.shape, angle)
        assert _same_table(a, ref) and a.warp.out_shape == want.out_shape
        assert np.array_equal(a.warp.matrix, want.matrix) and np.array_equal(a.warp.offset, want.offset)
    assert rot.rng.getstate() == rng.getstate()
    mod = next(D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=4, kwargs_dat={"rotateMod90_tr": True}))
    assert all(np.array_equal(t.warp.matrix, KW.rotate_warp(t.shape, -45.0).matrix) for t in mod)
    aff = next(D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=4, kwargs_dat={"affine_tr": True, "affine_value": 0.1}))
    again = next(D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 3, seed=4, kwargs_dat={"affine_tr": True, "affine_value": 0.1}))
    assert all(t.warp.out_shape == t.shape and np.array_equal(t.warp.matrix, u.warp.matrix) for t, u in zip(aff, again))
    assert not np.array_equal(aff[0].warp.matrix, np.eye(2))


@pytest.mark.parametrize("kw", [{"affine_tr": True, "rotate_tr": True}, {"affine_tr": True, "rotateMod90_tr": True}, {"elastic_tr": True},
                                {"affine_val": True}, {"rotate_val": True}, {"rotateMod90_val": True}, {"elastic_val": True}])
def test_refused_combinations_raise(kw):
    with pytest.raises(NotImplementedError):
        D.KVTrainBatches(PATHS, CHARSET, U.N_CLASS, 2, kwargs_dat=kw)
