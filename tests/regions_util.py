"""Inputs shared by tests/test_regions_cpu.py and tests/test_regions_gpu.py: the golden key-value documents, seeded noisy class
maps, and the shapes that break naive labelling.  A document is (cls int [h, w], line_mask uint16 [h, w], char_mask uint16 [h, w],
boxes [[x1, y1, x2, y2]])."""
import copy
import json
import os

import numpy as np

from tests.golden_util import GOLDEN

KV = os.path.join(GOLDEN, "kv")


def load_gold():
    return np.load(os.path.join(KV, "kv.npz")), json.load(open(os.path.join(KV, "kv.json")))


def gold_doc(g, meta, di):
    """-> (document, lines) of golden document `di`, the class map being the reference's own prediction"""
    md = meta[f"d{di}"]
    lines = copy.deepcopy(md["lines"])
    cls = np.argmax(g[f"d{di}.pred"].astype(np.float32), -1)
    return (cls, g[f"d{di}.line_mask"], g[f"d{di}.char_mask"], [l["box"] for l in lines]), lines


def blocky_map(rng, h, w, n_class, flip=0.03):
    """blocks of 4 x 6 pixels of one class, then `flip` of the pixels redrawn"""
    small = rng.integers(0, n_class, size=(h // 4 + 1, w // 6 + 1))
    cls = np.kron(small, np.ones((4, 6), int))[:h, :w]
    return np.where(rng.random((h, w)) < flip, rng.integers(0, n_class, size=(h, w)), cls)


def synthetic_lines(rng, h, w, n_lines):
    """text lines painted as KVModel paints them: boxes 3 px high (clipped by the page), line ids over the box, character
    positions in cells; later lines overwrite earlier ones, and boxes may overlap and reach past the page"""
    lm, cm, boxes = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16), []
    for li in range(n_lines):
        y1 = int(rng.integers(0, max(h - 1, 1)))
        x1 = int(rng.integers(0, max(w - 1, 1)))
        y2, x2 = y1 + int(rng.integers(1, 4)), x1 + int(rng.integers(1, max(w // 2, 2)))
        boxes.append([x1, y1, x2, y2])
        lm[y1:y2, x1:x2 + 1] = li + 1                       # (the painter's last glyph may reach past the box)
        n_char = max((x2 - x1) // 2, 1)
        for k in range(n_char):
            cm[y1:y2, x1 + 2 * k:x1 + 2 * k + 2] = k + 1
    return lm, cm, boxes


def with_lines(cls, seed, n_lines=12):
    rng = np.random.default_rng(seed)
    h, w = cls.shape
    return (np.asarray(cls),) + synthetic_lines(rng, h, w, n_lines)


def spiral(h, w, c):
    """one 1-px-wide path winding inwards: turns 2 rows and 4 columns apart, so that neither 4-connectivity nor the 1 x 3
    closing bridges them"""
    m = np.zeros((h, w), int)
    top, bottom, left, right = 0, h - 1, 1, w - 2
    while left <= right and top <= bottom:
        m[top, left:right + 1] = c
        m[top:bottom + 1, right] = c
        if bottom - top < 4 or right - left < 12:
            break
        m[bottom, left + 4:right + 1] = c
        m[top + 2:bottom + 1, left + 4] = c
        top, bottom, left, right = top + 2, bottom - 2, left + 4, right - 4
    return m


def comb(h, w, c):
    """a spine along the bottom row and teeth 4 columns apart over the whole height"""
    m = np.zeros((h, w), int)
    m[h - 1, 1:w - 1] = c
    m[:, 1:w - 1:4] = c
    return m


def shape_cases(max_pixels):
    """[(name, document, n_class)]"""
    rng = np.random.default_rng(11)
    out = []
    out.append(("spiral", with_lines(spiral(61, 121, 3), 1), 5))
    out.append(("comb", with_lines(comb(60, 120, 2), 2), 4))
    out.append(("full", with_lines(np.full((40, 50), 2), 3), 3))
    out.append(("empty", with_lines(np.zeros((40, 50), int), 4), 6))
    single = np.zeros((30, 40), int)
    single[::2, 1::4] = 4                                     # isolated pixels, 4 apart: the closing leaves them alone
    out.append(("single_pixels", with_lines(single, 5), 6))
    border = np.zeros((20, 30), int)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 3
    border[:, 1] = border[:, -2] = 3
    out.append(("four_borders", with_lines(border, 6), 5))
    for k, (h, w) in enumerate([(1, 9), (2, 9), (3, 9), (9, 1), (9, 2), (9, 3), (1, 1), (3, 3), (2, 5)]):
        out.append((f"thin_{h}x{w}", with_lines(rng.integers(2, 4, size=(h, w)), 20 + k, n_lines=3), 4))
    out.append(("class_never_occurs", with_lines(np.where(blocky_map(rng, 30, 40, 6) == 4, 0, blocky_map(rng, 30, 40, 6)), 7), 6))
    out.append(("n_class_3", with_lines(blocky_map(rng, 30, 40, 3), 8), 3))
    out.append(("n_class_40", with_lines(blocky_map(rng, 48, 72, 40), 9), 40))
    w = 192
    h = max_pixels // w
    out.append(("pixel_limit", with_lines(blocky_map(rng, h, w, 5, flip=0.01), 10, n_lines=40), 5))
    return out


def pack_canvas(docs, n_class, seed=0, round_to=16, neighbours=True):
    """documents at the origin of one canvas -> (argmax uint8 [B,H,W], line uint16, char uint16, sizes int64 [B,2]).  Outside a
    document's extent the class canvas holds random classes right up to the extent (`neighbours`), the two masks zeros."""
    rng = np.random.default_rng(seed)
    H = -(-max(d[0].shape[0] for d in docs) // round_to) * round_to
    W = -(-max(d[0].shape[1] for d in docs) // round_to) * round_to
    B = len(docs)
    am = rng.integers(0, n_class, size=(B, H, W)).astype(np.uint8) if neighbours else np.zeros((B, H, W), np.uint8)
    lm, cm = np.zeros((B, H, W), np.uint16), np.zeros((B, H, W), np.uint16)
    for b, (cls, l, c, _boxes) in enumerate(docs):
        h, w = cls.shape
        am[b, :h, :w], lm[b, :h, :w], cm[b, :h, :w] = cls, l, c
    return am, lm, cm, np.array([d[0].shape for d in docs], dtype=np.int64)


def counts(table):
    """(regions of the document, most regions in one class, pairs of the document, most pairs in one class)"""
    nr = [len(t[0]) for t in table.values()]
    npair = [len(t[1]) for t in table.values()]
    return sum(nr), max(nr, default=0), sum(npair), max(npair, default=0)
