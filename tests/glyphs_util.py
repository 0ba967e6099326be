"""Inputs shared by tests/test_glyphs_cpu.py and tests/test_glyphs_gpu.py: a KVModel that only knows its charset, the golden
layouts, and seeded generated layouts (page coordinates, as a layout + OCR JSON holds them).  Most boxes are 3 units high, so
that the grid scale is 1 and a page unit is a pixel: overlaps and gaps fall where the generator puts them."""
import copy
import json
import os

import numpy as np

from msau_amd.inference import KVModel
from msau_amd.inference import glyphs as G
from tests.golden_util import GOLDEN

KV = os.path.join(GOLDEN, "kv")
ALPHABET = "abcXYZ :-./#" + "0123456789" + "é€@_"            # charset, digits (folded to '0'), outside the charset


def charset_model():
    km = KVModel()
    km.set_charset(os.path.join(KV, "charset.txt"))
    return km


def gold_layout(di):
    return json.load(open(os.path.join(KV, f"layout{di}.json")))


def _line(x1, y1, x2, y2, text):
    return {"box": [int(x1), int(y1), int(x2), int(y2)], "text": text, "type": 0, "value": 0}


def _text(rng, n):
    return "".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=n))


def random_layout(seed, n_lines=40, height=60, width=140):
    """lines thrown over a small page so that many overlap: 3-unit boxes, some 0, 1, 2, 4 or 6 high, zero-width boxes, empty
    texts, texts of 80 characters in boxes a few units wide"""
    rng = np.random.default_rng(seed)
    lines = []
    for li in range(n_lines):
        x1, y1 = int(rng.integers(0, width - 10)), int(rng.integers(0, height - 6))
        hgt = 3 if rng.random() < 0.7 else int(rng.choice([0, 1, 2, 4, 6]))
        kind = rng.random()
        if kind < 0.1:
            wid, n = 0, int(rng.integers(1, 6))                         # a zero-width box
        elif kind < 0.25:
            wid, n = int(rng.integers(2, 7)), 80                        # text far longer than its box is wide
        elif kind < 0.35:
            wid, n = int(rng.integers(5, 60)), 0                        # no text
        else:
            n = int(rng.integers(1, 25))
            wid = n * int(rng.integers(2, 7)) + int(rng.integers(0, 3))
        lines.append(_line(x1, y1, x1 + wid, y1 + hgt, _text(rng, n)))
    return {"lines": lines}


def layout_cases():
    """[(name, layout dict)]"""
    rng = np.random.default_rng(1)
    out = [("random_40", random_layout(7)), ("random_40_b", random_layout(8))]
    # a later line over an earlier one, its glyphs one column out of phase: its gaps fall on the earlier line's characters
    out.append(("gap_over_glyph", {"lines": [_line(10, 10, 50, 13, "abcdefghij"), _line(11, 9, 51, 12, "klmnopqrst"),
                                             _line(0, 0, 9, 3, "xyz")]}))
    out.append(("nested", {"lines": [_line(0, 0, 96, 3, _text(rng, 16)), _line(20, 0, 44, 3, "ab12"), _line(24, 1, 30, 2, "Q"),
                                     _line(20, 0, 44, 3, "")]}))
    out.append(("one_line", {"lines": [_line(100, 200, 160, 203, "one line 42")]}))
    out.append(("single_character", {"lines": [_line(5, 5, 9, 8, "7"), _line(30, 5, 60, 8, "")]}))
    out.append(("past_right_edge", {"lines": [_line(0, 0, 40, 3, "left"), _line(36, 6, 40, 9, _text(rng, 80)),
                                              _line(40, 12, 40, 15, _text(rng, 30))]}))
    out.append(("zero_height", {"lines": [_line(0, 0, 30, 3, "abc"), _line(5, 1, 35, 1, "hidden"), _line(0, 6, 30, 9, "def")]}))
    # more lines than the kernel stages at a time (256), the later chunks over the earlier ones
    many = [_line(int(rng.integers(0, 200)), int(rng.integers(0, 90)), 0, 0, _text(rng, int(rng.integers(1, 12)))) for _ in range(600)]
    for l in many:
        l["box"][2], l["box"][3] = l["box"][0] + 4 * len(l["text"]), l["box"][1] + 3
    out.append(("lines_600", {"lines": many}))
    return out


def big_layout():
    """a grid of 150 x 420 pixels: more than the region kernel's LDS form holds"""
    rng = np.random.default_rng(3)
    lines = [_line(x, y, x + 60, y + 3, _text(rng, 14)) for y in range(0, 130, 5) for x in range(0, 400, 70)]
    return {"lines": lines}


def unrepresentable_layouts():
    """[(name, layout dict)]: what `glyph_table` has to hand to the host painter"""
    rev = {"lines": [_line(0, 0, 40, 3, "fine"), _line(30, 6, 10, 9, "reversed"), _line(0, 12, 40, 15, "fine too")]}
    wide = {"lines": [_line(0, 0, 40, 3, "fine"), _line(40000, 6, 40040, 9, "far away"), _line(0, 12, 40, 15, "fine too")]}
    return [("reversed_box", rev), ("beyond_int16", wide)]


def write_layout(doc, path):
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return str(path)


def painter(km, doc, tmp_path, name="doc"):
    """`KVModel._generate_masks_from_label` on a layout dict (it reads a file)"""
    return km._generate_masks_from_label(write_layout(doc, os.path.join(str(tmp_path), name + ".json")))


def table_of(km, doc):
    return G.glyph_table(copy.deepcopy(doc), km.tok_to_id, km.blank_idx)


def canvases_want(tables, canvas):
    """what the kernel has to write for a group: `paint_host` inside every document, -1 / 0 / 0 outside"""
    B, (H, W) = len(tables), canvas
    ids = np.full((B, H, W), -1, dtype=np.int32)
    lm, cm = np.zeros((B, H, W), np.uint16), np.zeros((B, H, W), np.uint16)
    for b, t in enumerate(tables):
        h, w = t.shape
        c, l, p = G.paint_host(t)
        ids[b, :h, :w], lm[b, :h, :w], cm[b, :h, :w] = c, l, p
    return ids, lm, cm


def gap_pixels(table, masks):
    """pixels whose line id is a line that has NO glyph there while a character of an earlier line shows: the rule that a later
    line's box takes the line id between two of its glyphs but does not hide the character"""
    char_ids, line_ids, char_pos = masks[:3]
    n = 0
    ys, xs = np.nonzero((line_ids > 0) & (char_pos > 0))
    for y, x in zip(ys.tolist(), xs.tolist()):
        li = int(line_ids[y, x]) - 1
        g0, cnt = int(table.line_rec[li, 4]), int(table.line_rec[li, 5])
        g = table.glyph_rec[g0:g0 + cnt]
        if not ((g[:, 0] <= x) & (x < g[:, 1])).any():
            n += 1
    return n
