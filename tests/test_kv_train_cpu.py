"""Key-value training tables on the CPU (msau_amd/training/kv_data.py): `paint_train_host(train_table(layout))` against the
reference generator's golden maps (tests/golden/kv_train, tools/gen_kv_train_goldens.py) and against the plain loop
`paint_train_painter`, the label rules on hand-made layouts, the argument checks, the C ABI, and the kernel of csrc/paint.hip
built as plain C++ (-DMSAU_PAINT_CPU: the same phases, lanes one after another) against `paint_train_host`.  Every comparison
is integer equality."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from msau_amd.training import kv_data as D
from tests import glyphs_util as U
from tests import kv_train_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_maps(got, want, what):
    for plane, g_, w in zip(("ids", "labels", "aux"), got, want):
        assert g_.shape == w.shape, (what, plane, g_.shape, w.shape)
        assert np.array_equal(g_, w), (what, plane, int((g_ != w).sum()))


# ---- 1: the reference generator's maps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(T.SETTINGS)))
@pytest.mark.parametrize("di", [0, 1, 2])
def test_table_equals_reference_generator(si, di):
    g = np.load(T.GOLD)
    assert g["settings"].tolist() == [list(s) for s in T.SETTINGS] and int(g["n_class"]) == T.N_CLASS
    tok_to_id, blank, n_token = T.CHARSET
    assert int(g["n_token"]) == n_token
    smin, smax, err, seed = T.SETTINGS[si]
    rng = random.Random(seed)
    t = D.train_table(T.gold_path(di), tok_to_id, blank, n_token, T.N_CLASS, smin, smax, err, rng)
    assert rng.random() == float(g[f"s{si}.d{di}.next"])                   # the draws consumed
    assert t.ok, t.reason                                                   # no fallback on the goldens
    want = [g[f"s{si}.d{di}.{name}"] for name in ("ids", "labels", "aux")]
    assert t.shape == want[0].shape
    _assert_maps(D.paint_train_host(t), want, (si, di))
    _assert_maps(D.paint_train_painter(t), want, (si, di, "painter"))


def test_goldens_are_what_they_are_for():
    g = np.load(T.GOLD)
    assert os.path.getsize(T.GOLD) < os.path.getsize(os.path.join(U.KV, "kv.npz")) // 4
    shapes = {g[f"s{si}.d0.ids"].shape for si in range(len(T.SETTINGS))}
    assert len(shapes) >= 4                                                 # the scale and the pad are drawn
    for si in range(len(T.SETTINGS)):
        for di in range(3):
            lab, aux = g[f"s{si}.d{di}.labels"], g[f"s{si}.d{di}.aux"]
            assert lab.max() > 0 and aux.max() > 0 and (lab != aux).any()  # two different label maps
    blank = T.CHARSET[1]
    # OCR errors: more blanks in the ids at text_err 0.3 than at 0 (same scale)
    assert sum(int((g[f"s3.d{di}.ids"] == blank).sum()) for di in range(3)) > sum(int((g[f"s0.d{di}.ids"] == blank).sum()) for di in range(3))
    # a dict is left as it was, and gives the table of its file
    doc = U.gold_layout(0)
    before = [list(ln["box"]) for ln in doc["lines"]]
    t = T.table_of(doc, 2.0, 4.0, 0.1, seed=102)
    t2 = T.table_of(T.gold_path(0), 2.0, 4.0, 0.1, seed=102)
    assert [ln["box"] for ln in doc["lines"]] == before
    assert np.array_equal(t.line_rec, t2.line_rec) and np.array_equal(t.glyph_rec, t2.glyph_rec) and np.array_equal(t.label_rec, t2.label_rec)
    assert t.label_rec.dtype == np.int32 and t.label_rec.shape == (len(t.line_rec), 2)


# ---- 2: the gather against the loop --------------------------------------------------------------------------------------------
def test_gather_equals_loop_on_generated_layouts():
    for name, doc in T.labelled_cases():
        for kw in (dict(), dict(scale_min=2.0, scale_max=4.0, text_err=0.2, seed=3)):
            t = T.table_of(doc, **kw)
            assert t.ok, (name, t.reason)
            _assert_maps(D.paint_train_host(t), D.paint_train_painter(t), name)
    t = T.table_of(dict(T.labelled_cases())["random_40"])
    assert len(set(t.label_rec[:, 0].tolist())) > 5 and len(set(t.label_rec[:, 1].tolist()) | {0, 1}) > 4
    text = "".join(l["text"] for l in t.lines)                              # digits are not folded to '0'
    assert any(ch.isdigit() and ch != "0" for ch in text)
    assert int((t.tokens == T.CHARSET[0]["0"]).sum()) == text.count("0")


def test_label_rules_on_hand_made_layouts():
    maps = {}
    for name, doc in T.hand_cases():
        t = T.table_of(doc)
        assert t.ok and t.scale == 1.0, (name, t.reason)
        maps[name] = D.paint_train_host(t)
        _assert_maps(maps[name], D.paint_train_painter(t), name)
    P = 9                                                                   # the pad of a 3-unit median
    ids, lab, aux = maps["narrow_box"]
    row = slice(P + 6, P + 9)
    assert (lab[row, P + 10:P + 14] == 8).all() and (aux[row, P + 10:P + 14] == 8).all()
    assert (ids[row, P + 14:P + 22] > 0).all() and not lab[row, P + 14:P + 22].any() and not aux[row, P + 14:P + 22].any()
    ids, lab, aux = maps["zero_over_label"]
    assert (lab[P:P + 3, P:P + 10] == 6).all() and not lab[P:P + 3, P + 10:P + 30].any() and (lab[P:P + 3, P + 30:P + 40] == 6).all()
    assert not aux[P:P + 3, P + 10:P + 30].any()
    ids, lab, aux = maps["empty_over_label"]
    assert (lab[P:P + 3, P:P + 40] == 6).all() and (aux[P:P + 3, P:P + 40] == 6).all()
    ids, lab, aux = maps["types"]
    assert [int(lab[P + y, P + 1]) for y in (0, 6, 12)] == [4, 4, 4] and [int(aux[P + y, P + 1]) for y in (0, 6, 12)] == [0, 4, 1]
    assert (int(lab[P, P + 41]), int(aux[P, P + 41])) == (0, 1) and (int(lab[P + 6, P + 41]), int(aux[P + 6, P + 41])) == (16, 1)
    ids, lab, aux = maps["zero_height"]
    assert 7 not in lab and 7 not in aux and (lab[P:P + 3, P:P + 30] == 3).all()


def test_draws_follow_the_generator():
    """the scale draw is consumed at equal bounds, the error draw at text_err 0; a hit consumes a choice and gives the blank"""
    tok_to_id, blank, n_token = T.CHARSET
    doc = {"lines": [T._line(0, 0, 40, 3, "abcd", 1, 2), T._line(0, 6, 40, 9, "", 1, 2), T._line(0, 12, 40, 15, "XY", 2, 2)]}
    rng, twin = random.Random(5), random.Random(5)
    D.train_table(doc, tok_to_id, blank, n_token, T.N_CLASS, 3.0, 3.0, 0.0, rng)
    for _ in range(1 + 6):
        twin.random()
    assert rng.random() == twin.random()
    t = T.table_of(doc, text_err=1.0)                                      # every character replaced
    assert t.tokens.tolist() == [blank] * 6
    rng, twin = random.Random(5), random.Random(5)
    D.train_table(doc, tok_to_id, blank, n_token, T.N_CLASS, 3.0, 3.0, 1.0, rng)
    twin.random()
    for _ in range(6):
        twin.random()
        twin.choice(range(n_token))
    assert rng.random() == twin.random()
    assert D.train_table(doc, tok_to_id, blank, n_token, T.N_CLASS).ok    # rng None: a fresh generator


# ---- 4: argument checks and the fallback ---------------------------------------------------------------------------------------
def test_label_beyond_n_class_raises():
    doc = {"lines": [T._line(0, 0, 40, 3, "abcd", 1, T.N_CLASS - 1)]}
    with pytest.raises(ValueError, match="n_class"):
        T.table_of(doc)
    doc["lines"][0]["type"] = 0                                            # the final map alone
    with pytest.raises(ValueError, match="n_class"):
        T.table_of(doc)
    assert T.table_of(doc, n_class=T.N_CLASS + 1).ok
    doc["lines"][0]["text"] = ""                                           # paints nothing: no label
    assert T.table_of(doc).ok


def test_unrepresentable_documents_are_reported_and_painted_by_the_loop():
    for name, doc in U.unrepresentable_layouts():
        t = T.table_of(T.with_labels(doc, 2))
        assert not t.ok and t.reason and t.line_rec is None and t.glyph_rec is None, name
        with pytest.raises(ValueError):
            D.paint_train_host(t)
    good = T.gold_tables()[0]
    bad = T.table_of(T.with_labels(U.unrepresentable_layouts()[0][1], 2))
    ids, lab, aux = D.paint_train_painter(bad)                             # the fallback
    assert ids.shape == bad.shape and lab.max() > 0
    records, off, sizes, canvas = D.pack_train_tables([good, bad, good])
    n = len(good.line_rec)
    assert records[off["line_off"]:off["line_off"] + 4].tolist() == [0, n, n, 2 * n]
    assert off["glyphs"] - off["labels"] == 2 * 2 * n and off["labels"] - off["lines"] == 8 * 2 * n and off["glyphs"] % 2 == 0
    assert np.array_equal(records[off["labels"]:off["glyphs"]].reshape(-1, 2), np.concatenate([good.label_rec, good.label_rec]))
    want = D.canvases_host([good, bad, good])
    assert np.array_equal(want[1][1, :bad.shape[0], :bad.shape[1]], lab) and (want[1][1, bad.shape[0]:] == -1).all()
    # the wire: a few bytes per character
    glyphs, lines = len(good.glyph_rec), len(good.line_rec)
    records, _o, _s, _c = D.pack_train_tables([good], round_to=1)
    assert records.nbytes <= 8 * glyphs + 40 * lines + 64


def test_batches_iterate_over_epochs_and_validation_is_deterministic():
    paths = [T.gold_path(di) for di in range(3)]
    it = D.KVTrainBatches(paths, os.path.join(U.KV, "charset.txt"), T.N_CLASS, batch_size=2, seed=4)
    groups = [next(it) for _ in range(3)]                                   # two epochs
    assert all(len(g_) == 2 and all(t.ok for t in g_) for g_ in groups)
    assert len({t.shape for g_ in groups for t in g_}) == 6                 # every table has its own jitter
    again = D.KVTrainBatches(paths, os.path.join(U.KV, "charset.txt"), T.N_CLASS, batch_size=2, seed=4)
    assert [t.shape for g_ in groups for t in g_] == [t.shape for _ in range(3) for t in next(again)]
    val = it.validation()
    assert [len(g_) for g_ in val] == [2, 1]
    for t, want in zip([t for g_ in val for t in g_], T.gold_tables(0)):
        assert t.shape == want.shape and np.array_equal(t.glyph_rec, want.glyph_rec) and np.array_equal(t.label_rec, want.label_rec)
    from msau_amd import training
    assert training.KVTrainBatches is D.KVTrainBatches and training.train_table is D.train_table
    assert training.paint_train_host is D.paint_train_host


# ---- 5: the C ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_training_symbols_and_version_stays():
    from msau_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name, proto in (("msau_kv_paint_train", "int msau_kv_paint_train("), ("msau_label_hist", "int msau_label_hist("),
                        ("msau_unet_ce", "int msau_unet_ce("), ("msau_unet_ce_ws_floats", "int64_t msau_unet_ce_ws_floats(")):
        assert name in L.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
        assert proto in header, name
    assert lib.msau_version() == 11
    assert lib.msau_unet_ce_ws_floats(1) >= 2 and lib.msau_unet_ce_ws_floats(1 << 30) >= lib.msau_unet_ce_ws_floats(1)


# ---- 3: the kernel's body as plain C++ ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("paint_train_cpu") / "libpaint_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_PAINT_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "paint.hip"), "-o", out], check=True)
    lib = C.CDLL(out)

    def run(tables, round_to=16):
        records, off, sizes, (H, W) = D.pack_train_tables(tables, round_to=round_to)
        B = len(tables)
        rng = np.random.default_rng(0)                                    # the kernel clears nothing: start from garbage
        ids = rng.integers(-5, 1 << 20, size=(B, H, W)).astype(np.int32)
        lab, aux = (rng.integers(-3, 40, size=(B, H, W)).astype(np.int64) for _ in range(2))
        base = records.ctypes.data
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        at = lambda name: C.c_void_p(base + 4 * off[name])
        rc = lib.msau_kv_paint_train_cpu(at("lines"), at("glyphs"), at("labels"), at("line_off"), at("glyph_off"), at("sizes"),
                                         B, H, W, p(ids), p(lab), p(aux))
        assert rc == 0
        return (ids, lab, aux), (H, W)

    return run


@pytest.fixture(scope="module")
def named_tables():
    return T.all_tables()


def test_cpu_form_of_kernel_dense(cpu_kernel, named_tables):
    assert any(len(t.line_rec) > 256 for _, t in named_tables)             # more than one staging pass
    for name, t in named_tables:
        got, canvas = cpu_kernel([t], round_to=1)
        assert canvas == t.shape
        _assert_maps(got, T.canvases_want([t], round_to=1)[:3], name)


def test_cpu_form_of_kernel_ragged(cpu_kernel, named_tables):
    tables = [t for _, t in named_tables]
    assert len({t.shape for t in tables}) > 8
    got, canvas = cpu_kernel(tables)
    want = T.canvases_want(tables)
    assert want[0].shape[1:] == canvas
    _assert_maps(got, want[:3], "ragged")
    for b, t in enumerate(tables):
        h, w = t.shape
        outside = np.ones(canvas, bool)
        outside[:h, :w] = False
        assert all((g_[b][outside] == -1).all() for g_ in got) and all((g_[b, :h, :w] >= 0).all() for g_ in got)
    # a document without a table: an empty document of its shape for the kernel
    small, large = tables[2], tables[-1]
    bad = T.table_of(T.with_labels(U.unrepresentable_layouts()[0][1], 2))
    for group in ([small, large], [large, small], [small, bad, large]):
        got, canvas = cpu_kernel(group)
        keep = [b for b, t in enumerate(group) if t.ok]
        want = T.canvases_want(group)
        _assert_maps([g_[keep] for g_ in got], [w[keep] for w in want[:3]], "pair")
        for b, t in enumerate(group):
            if not t.ok:
                h, w = t.shape
                for g_ in got:
                    assert (g_[b, :h, :w] == 0).all() and (g_[b, h:] == -1).all() and (g_[b, :, w:] == -1).all()

