"""Inputs shared by tests/test_kv_warp_cpu.py and tests/test_kv_warp_gpu.py: a ragged group of hand-made training tables (23 x 31
with text on its borders, 37 x 29, 2 x 3, 1 x 1), the warps of the issue (seeded affines at 0.025 and 0.1, rotations by 13.7, -20
and -45 degrees, the identity), the statement's outputs for every (document, warp) -- computed once and left unchanged -- and the
pixels that a comparison with an fp32 kernel may leave out, found from the statement alone."""
import functools

import numpy as np

from msau_amd.inference import glyphs as G
from msau_amd.training import kv_data as D
from msau_amd.training import kv_warp as KW
from tests import kv_train_util as T

N_CLASS = T.N_CLASS
TOK_TO_ID, BLANK, N_TOKEN = T.CHARSET
DOC_SHAPES = [(23, 31), (37, 29), (2, 3), (1, 1)]
WARP_NAMES = ["affine025", "affine100", "rot13.7", "rot-20", "rot-45", "identity"]
AFFINE_SEED = 7
KERNEL_MARGIN = 0.01                # grey levels around 64.5: fp32 sums of <= ~1000 terms of magnitude <= 255 (1e-3) + the 1e-4 tail
KERNEL_CAP = 0.001                  # of a case's pixels


def grid_table(shape, lines) -> D.TrainTable:
    """a training table straight from grid boxes: lines = [(x1, y1, x2, y2, text, label, aux_label)]"""
    boxes = np.array([l[:4] for l in lines], dtype=np.int64).reshape(len(lines), 4)
    count = np.array([len(l[4]) for l in lines], dtype=np.int64)
    tokens = np.array([TOK_TO_ID.get(ch, BLANK) for l in lines for ch in l[4]], dtype=np.int64)
    label_rec = np.array([[l[5], l[6]] if len(l[4]) else [0, 0] for l in lines], dtype=np.int32).reshape(len(lines), 2)
    line_rec, glyph_rec, why = G.span_records(boxes, count, shape, lambda: tokens)
    assert why == "", why
    dicts = [dict(box=list(l[:4]), text=l[4]) for l in lines]
    return D.TrainTable(tuple(shape), 1.0, 1.0, 1.0, 0, dicts, tokens, label_rec, line_rec, glyph_rec, why)


def documents():
    """the ragged group; the first document has text on its top, left, right and bottom borders"""
    d0 = grid_table((23, 31), [(0, 0, 14, 3, "Invoice no", 2, 3), (16, 0, 31, 3, "A-1047/x", 3, 1), (2, 5, 29, 8, "Total amount due", 5, 6),
                               (3, 10, 12, 13, "EUR", 1, 1), (14, 10, 30, 13, "1,234.50", 7, 0), (0, 15, 9, 17, "Date", 4, 5),
                               (11, 15, 29, 18, "2019-03-07", 9, 1), (0, 20, 22, 23, "Thank you, Inc.", 16, 2), (24, 19, 31, 23, "p.1", 0, 1)])
    d1 = grid_table((37, 29), [(1, 1, 20, 4, "Bill to:", 2, 2), (3, 6, 28, 9, "ACME Corp. GmbH", 6, 1), (0, 11, 29, 14, "Street 12, 4711 Town", 8, 1),
                               (5, 16, 11, 19, "Qty", 1, 3), (13, 16, 25, 19, "Price", 1, 4), (5, 21, 9, 24, "12", 10, 0),
                               (13, 21, 27, 24, "99.90 $", 11, 1), (2, 27, 26, 31, "net 30 days", 12, 13), (0, 33, 15, 37, "VAT 19%", 15, 1)])
    d2 = grid_table((2, 3), [(0, 0, 3, 1, "ab", 3, 1), (1, 1, 3, 2, "c", 1, 4)])
    d3 = grid_table((1, 1), [(0, 0, 1, 1, "x", 5, 1)])
    return [d0, d1, d2, d3]


def gold_table() -> D.TrainTable:
    return T.gold_tables(0)[0]


def warp_of(name: str, shape) -> KW.Warp:
    if name.startswith("affine"):
        return KW.affine_warp(shape, int(name[6:]) / 1000.0, np.random.RandomState(AFFINE_SEED))
    if name.startswith("rot"):
        return KW.rotate_warp(shape, float(name[3:]))
    return KW.identity_warp(shape)


def with_warp(table: D.TrainTable, warp) -> D.TrainTable:
    import dataclasses
    return dataclasses.replace(table, warp=warp)


@functools.lru_cache(maxsize=None)
def _tables():
    return tuple(documents() + [gold_table()])


def table(di: int) -> D.TrainTable:
    """document di: 0 - 3 the hand-made group, 4 the golden layout"""
    return _tables()[di]


@functools.lru_cache(maxsize=None)
def painted(di: int):
    ids, lab, aux = D.paint_train_host(table(di))
    return ids.astype(np.int32), lab.astype(np.int64), aux.astype(np.int64)


@functools.lru_cache(maxsize=None)
def statement(di: int, name: str):
    """-> (warp, (multi-hot uint8, labels, aux) of `warp_host`, distance float64 [ho, wo]: how close the nearest plane of the
    statement -- of the ids, the labels or the aux labels -- comes to the threshold, in grey levels)"""
    ids, lab, aux = painted(di)
    warp = warp_of(name, ids.shape)
    want = KW.warp_host(ids, lab, aux, warp, N_TOKEN, N_CLASS)
    dist = np.full(warp.out_shape, np.inf)
    for canvas, lo, hi in ((ids, 0, N_TOKEN), (lab, 1, N_CLASS), (aux, 1, N_CLASS)):
        present = [int(c) for c in np.unique(canvas) if lo <= c < hi]
        if present:
            dist = np.minimum(dist, np.abs(KW.plane_values(canvas, warp, present) - KW.THRESHOLD).min(axis=-1))
    for a in want:
        a.setflags(write=False)
    dist.setflags(write=False)
    return warp, want, dist


def left_out(di: int, name: str, margin: float) -> np.ndarray:
    """bool [ho, wo]: the pixels where the statement has a plane within `margin` grey levels of the threshold"""
    return statement(di, name)[2] <= margin


@functools.lru_cache(maxsize=None)
def wide_case():
    """-> (table, warp, statement outputs, keep bool [ho, wo]): the golden layout under a map that shrinks it about 5-fold, so a
    tile's windows span more source pixels than the kernel's LDS tile holds and it reads the canvases directly; `keep` leaves out the
    pixels within KERNEL_MARGIN of the threshold (at most KERNEL_CAP of them, asserted here from the statement alone)"""
    h, w = table(4).shape
    warp = KW.Warp(np.array([[4.7, 0.3], [-0.2, 5.1]]), np.array([1.5, 2.25]), (h // 5 + 3, w // 5 + 2))
    ids, lab, aux = painted(4)
    want = KW.warp_host(ids, lab, aux, warp, N_TOKEN, N_CLASS)
    dist = np.full(warp.out_shape, np.inf)
    for canvas, lo, hi in ((ids, 0, N_TOKEN), (lab, 1, N_CLASS), (aux, 1, N_CLASS)):
        present = [int(c) for c in np.unique(canvas) if lo <= c < hi]
        dist = np.minimum(dist, np.abs(KW.plane_values(canvas, warp, present) - KW.THRESHOLD).min(axis=-1))
    keep = dist > KERNEL_MARGIN
    assert int((~keep).sum()) <= KERNEL_CAP * keep.size and int(want[0].sum()) > 0
    return table(4), warp, want, keep


def cases(docs=range(5)):
    return [(di, name) for di in docs for name in WARP_NAMES]


def group_canvases(tables):
    """the painter's canvases of a group on the host, as `msau_kv_warp_train` reads them"""
    return D.canvases_host(list(tables))
