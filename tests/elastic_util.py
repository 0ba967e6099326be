"""Inputs shared by tests/test_kv_elastic_cpu.py and tests/test_kv_elastic_gpu.py: the five documents of tests/warp_util.py and a
hand-made 52 x 77 table (a 2 x 3 field grid), the elastic warps of the issue -- the generator's fields from
tests/golden/kv/elastic_fields.npz (tools/elastic_fields.py) at the values 0.0002, 0.002 and 0.01, seeded random uint8 fields with
five pairs of alphas, integer displacements -- the statement's outputs for every (document, case), computed once and left unchanged,
and the pixels a comparison would have to leave out, found from the statement alone (there are none)."""
import functools
import os

import numpy as np

from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import glyphs_util as GU
from tests import warp_util as W

N_CLASS, N_TOKEN = W.N_CLASS, W.N_TOKEN
FIXTURE = os.path.join(GU.KV, "elastic_fields.npz")
BIG = 5                                                                     # the 52 x 77 document; 0 - 4 are warp_util's
FIXTURE_DOCS = {1: 0, 4: 1, BIG: 2}                                         # document -> index in the fixture
GEN_VALUES = {"gen0002": 0.0002, "gen002": 0.002, "gen01": 0.01}            # gen01 on 44 x 91: 0.44 * 255 = 112 pixels
RAND_ALPHAS = [(0.01, 0.013), (0.05, -0.02), (0.25, 0.125), (-1.0, 0.5), (0.0, 0.0)]   # (alpha_y, alpha_x)
FIELD_SEED = 31
# float64 sums of 4 terms <= 255 in another order differ by ~1e-13 grey levels: a plane this close to 64.5 is not pinned
MARGIN = 1e-9


def big_table() -> D.TrainTable:
    return W.grid_table((52, 77), [(0, 0, 30, 3, "Purchase order 77", 2, 3), (40, 0, 77, 3, "No. 2019/0815-b", 3, 1),
                                   (2, 6, 70, 9, "Supplier: Example Trading Company Ltd.", 5, 6), (5, 12, 25, 15, "Item", 1, 1),
                                   (30, 12, 50, 15, "Quantity", 1, 4), (55, 12, 75, 15, "Amount", 1, 2), (5, 18, 28, 21, "Paper A4, 80g", 7, 0),
                                   (30, 18, 44, 21, "12 box", 8, 1), (55, 18, 77, 21, "1,044.00 EUR", 9, 1), (5, 24, 29, 27, "Toner black", 7, 0),
                                   (30, 24, 42, 27, "3 pcs", 8, 1), (55, 24, 76, 27, "217.35 EUR", 9, 1), (0, 31, 40, 35, "Delivery within 14 days", 12, 13),
                                   (44, 31, 77, 35, "Total 1,261.35", 10, 5), (3, 38, 60, 41, "Payment: net 30 days, 2% discount", 14, 1),
                                   (0, 44, 22, 47, "Signature:", 4, 5), (26, 44, 70, 48, "J. Doe / accounting", 15, 1),
                                   (0, 49, 77, 52, "page 1 of 1 - printed 2019-03-07 - internal", 16, 2)])


@functools.lru_cache(maxsize=None)
def table(di: int) -> D.TrainTable:
    return big_table() if di == BIG else W.table(di)


@functools.lru_cache(maxsize=None)
def painted(di: int):
    if di != BIG:
        return W.painted(di)
    ids, lab, aux = D.paint_train_host(table(di))
    return ids.astype(np.int32), lab.astype(np.int64), aux.astype(np.int64)


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def case_names(di: int):
    """the cases of document di"""
    h, w = table(di).shape
    names = []
    if di in FIXTURE_DOCS:
        names += ["gen0002", "gen002"] + (["gen01"] if di == 4 else [])
    if di < 4:
        names += [f"rand{k}" for k in range(len(RAND_ALPHAS))] + ["int"]
    return names


@functools.lru_cache(maxsize=None)
def elastic_of(di: int, name: str) -> KW.Elastic:
    h, w = table(di).shape
    if name.startswith("gen"):
        k = FIXTURE_DOCS[di]
        assert tuple(fixture()["shapes"][k]) == (h, w)
        a = GEN_VALUES[name] * min(h, w)
        return KW.Elastic(fixture()[f"fy{k}"], fixture()[f"fx{k}"], a, a, (h, w))
    rs = np.random.RandomState(FIELD_SEED + 10 * di)
    fy, fx = (rs.randint(0, 256, size=(h, w)).astype(np.uint8) for _ in range(2))
    if name == "int":
        return KW.Elastic(fy % 4, fx % 4, 1.0, 1.0, (h, w))
    ay, ax = RAND_ALPHAS[int(name[4:])]
    return KW.Elastic(fy, fx, ay, ax, (h, w))


@functools.lru_cache(maxsize=None)
def statement(di: int, name: str):
    """-> (Elastic, (multi-hot uint8, labels, aux) of `elastic_host`, distance float64 [h, w]: how close the nearest plane of the
    statement -- of the ids, the labels or the aux labels -- comes to the threshold, in grey levels)"""
    ids, lab, aux = painted(di)
    el = elastic_of(di, name)
    want = KW.elastic_host(ids, lab, aux, el, N_TOKEN, N_CLASS)
    dist = np.full(el.out_shape, np.inf)
    for canvas, lo, hi in ((ids, 0, N_TOKEN), (lab, 1, N_CLASS), (aux, 1, N_CLASS)):
        present = [int(c) for c in np.unique(canvas) if lo <= c < hi]
        if present:
            dist = np.minimum(dist, np.abs(KW.elastic_values(canvas, el, present) - KW.ELASTIC_THRESHOLD).min(axis=-1))
    for a in want:
        a.setflags(write=False)
    dist.setflags(write=False)
    return el, want, dist


def left_out(di: int, name: str, margin: float = MARGIN) -> np.ndarray:
    """bool [h, w]: the pixels where the statement has a plane within `margin` grey levels of the threshold"""
    return statement(di, name)[2] <= margin


def cases():
    return [(di, name) for di in range(6) for name in case_names(di)]


# the ragged groups the kernel is run on: every case takes part in one; FAR is the 112-pixel case, on its own
GROUPS = ([[(4, g), (BIG, g), (1, g)] for g in ("gen0002", "gen002")]
          + [[(di, n) for di in range(4)] for n in [f"rand{k}" for k in range(len(RAND_ALPHAS))] + ["int"]])
FAR = [(4, "gen01")]
STEPPED = [(0, "rand2"), (1, "rand0"), (2, "int"), (3, "rand1")]            # the group of the step_kv test


def group_canvases(group):
    """-> (ids, lab, aux, sizes) of the painter on the host, and (fields, alphas) as `msau_kv_elastic_train` reads them"""
    ids, lab, aux, sizes = D.canvases_host([table(di) for di, _ in group])
    fields, alphas = KW.elastic_records([elastic_of(di, n) for di, n in group], sizes, ids.shape[1], ids.shape[2])
    return (ids, lab, aux, sizes), (fields, alphas)


def assert_document(got, b, di, name, n_token=N_TOKEN):
    """document b of the kernel's outputs (grid float [B, Ho, Wo, Cs], labels, aux) against the statement of (di, name): exact on
    every pixel, zeros and -1 written over the sentinels everywhere else"""
    grid, lab, aux = got[:3]
    el, want, _ = statement(di, name)
    h, w = el.out_shape
    assert int(left_out(di, name).sum()) == 0, (di, name)                   # from the statement alone: all pixels are kept
    assert bool(np.isin(grid[b], (0.0, 1.0)).all())                         # every sentinel is gone
    assert np.array_equal(grid[b, :h, :w, :n_token], want[0].astype(np.float32)), (di, name)
    assert np.array_equal(lab[b, :h, :w], want[1]) and np.array_equal(aux[b, :h, :w], want[2]), (di, name)
    outside = np.ones(grid.shape[1:3], dtype=bool)
    outside[:h, :w] = False
    assert float(np.abs(grid[b][outside]).sum()) == 0.0 and float(np.abs(grid[b, :, :, n_token:]).sum()) == 0.0
    assert bool((lab[b][outside] == -1).all()) and bool((aux[b][outside] == -1).all())
    assert int(grid[b].sum(axis=-1).max()) <= 3                             # at most three planes of a pixel
