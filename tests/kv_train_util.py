"""Inputs shared by tests/test_kv_train_cpu.py and tests/test_kv_train_gpu.py: the charset, the golden settings and maps, training
tables of the golden and the generated layouts (tests/glyphs_util.py) with pseudo-random `type` / `value` from a seed, and the
hand-made cases of the label rules."""
import copy
import os
import random

import numpy as np

from msau_amd.training import kv_data as D
from tests import glyphs_util as U

N_CLASS = 17
GOLD = os.path.join(U.GOLDEN, "kv_train", "kv_train.npz")
SETTINGS = [(3.0, 3.0, 0.0, 100), (2.0, 4.0, 0.0, 101), (2.0, 4.0, 0.1, 102), (3.0, 3.0, 0.3, 103), (2.0, 2.5, 0.1, 104)]
CHARSET = D.load_charset(os.path.join(U.KV, "charset.txt"))            # (tok_to_id, blank_idx, n_token)


def table_of(doc, scale_min=3.0, scale_max=3.0, text_err=0.0, seed=0, n_class=N_CLASS):
    tok_to_id, blank, n_token = CHARSET
    doc = doc if isinstance(doc, str) else copy.deepcopy(doc)
    return D.train_table(doc, tok_to_id, blank, n_token, n_class, scale_min, scale_max, text_err, random.Random(seed))


def gold_path(di):
    return os.path.join(U.KV, f"layout{di}.json")


def gold_tables(si=0):
    smin, smax, err, seed = SETTINGS[si]
    return [table_of(gold_path(di), smin, smax, err, seed) for di in range(3)]


def with_labels(doc, seed):
    """the layout with `type` in {0, 1, 2} and `value` in [0, N_CLASS - 1) from a seed"""
    rng = np.random.default_rng(seed)
    doc = copy.deepcopy(doc)
    for line in doc["lines"]:
        line["type"], line["value"] = int(rng.integers(0, 3)), int(rng.integers(0, N_CLASS - 1))
    return doc


def labelled_cases():
    """[(name, layout dict)]: the generated layouts of glyphs_util with assigned labels"""
    return [(name, with_labels(doc, 11 + i)) for i, (name, doc) in enumerate(U.layout_cases())]


def _line(x1, y1, x2, y2, text, type_=0, value=0):
    return dict(U._line(x1, y1, x2, y2, text), type=type_, value=value)


def hand_cases():
    """[(name, layout dict)]; 3-unit lines at scale 3: a page unit is a pixel, the pad 9"""
    return [
        # 12 characters in a box 4 wide: the pitch is clamped to 1, glyphs 4 .. 11 lie beyond x2 with an id and label 0
        ("narrow_box", {"lines": [_line(0, 0, 60, 3, "a wide line of text", 1, 4), _line(10, 6, 14, 9, "abcXYZabcXYZ", 1, 7)]}),
        ("zero_over_label", {"lines": [_line(0, 0, 40, 3, "labelled", 1, 5), _line(10, 0, 30, 3, "plain", 0, 0)]}),
        ("empty_over_label", {"lines": [_line(0, 0, 40, 3, "labelled", 1, 5), _line(10, 0, 30, 3, "", 1, 9)]}),
        ("types", {"lines": [_line(0, 0, 30, 3, "type0", 0, 3), _line(0, 6, 30, 9, "type1", 1, 3), _line(0, 12, 30, 15, "type2", 2, 3),
                             _line(40, 0, 70, 3, "value0", 1, 0), _line(40, 6, 70, 9, "last", 2, N_CLASS - 2)]}),
        ("zero_height", {"lines": [_line(0, 0, 30, 3, "abc", 1, 2), _line(5, 1, 35, 1, "hidden", 1, 6), _line(0, 6, 30, 9, "def", 2, 0)]}),
    ]


def canvases_want(tables, round_to=16):
    return D.canvases_host(tables, round_to=round_to)


def all_tables():
    """[(name, table)]: golden documents of every setting, generated and hand-made layouts, the big layout"""
    out = [(f"s{si}.d{di}", t) for si in range(len(SETTINGS)) for di, t in enumerate(gold_tables(si))]
    out += [(name, table_of(doc, seed=i)) for i, (name, doc) in enumerate(labelled_cases() + hand_cases())]
    out.append(("big", table_of(with_labels(U.big_layout(), 5))))
    out.append(("big_jitter", table_of(with_labels(U.big_layout(), 6), 2.0, 4.0, 0.2, seed=9)))
    return out
