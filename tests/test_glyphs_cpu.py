"""Glyph tables on the CPU (msau_amd/inference/glyphs.py): `paint_host(glyph_table(layout))` against the host painter
`KVModel._generate_masks_from_label` and the reference's golden masks, the documents the table must refuse, the wire size, the
C ABI, and the kernel of csrc/paint.hip built as plain C++ (-DMSAU_PAINT_CPU: the same phases, lanes one after another) against
`paint_host`.  Every comparison is integer equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from msau_amd.inference import glyphs as G
from tests import glyphs_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def km():
    return U.charset_model()


def _assert_same_document(km, doc, tmp_path, name):
    """table and painter agree on everything the painter returns -> (table, the painter's masks)"""
    want = U.painter(km, doc, tmp_path, name)
    t = U.table_of(km, doc)
    assert t.ok, (name, t.reason)
    got = G.paint_host(t)
    for plane, g_, w in zip(("char_ids", "line_ids", "char_pos"), got, want[:3]):
        assert g_.dtype == np.uint16 and g_.shape == w.shape, (name, plane)
        assert np.array_equal(g_, w), (name, plane, int((g_ != w).sum()))
    assert t.lines == want[3] and t.scale == want[4] and t.bg_pad == want[5] and tuple(t.text_bbox) == tuple(want[6]), name
    assert t.shape == want[0].shape
    return t, want


# ---- 1: the golden layouts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("di", [0, 1, 2])
def test_paint_host_equals_painter_and_reference_on_golden_layouts(km, tmp_path, di):
    t, _ = _assert_same_document(km, U.gold_layout(di), tmp_path, f"layout{di}")
    g = np.load(os.path.join(U.KV, "kv.npz"))
    c, l, p = G.paint_host(t)
    assert np.array_equal(c, g[f"d{di}.input_mask"]) and np.array_equal(l, g[f"d{di}.line_mask"]) and np.array_equal(p, g[f"d{di}.char_mask"])
    # by path as by dict, and a dict is left as it was
    doc = U.gold_layout(di)
    before = [list(ln["box"]) for ln in doc["lines"]]
    t2 = G.glyph_table(doc, km.tok_to_id, km.blank_idx)
    t3 = G.glyph_table(os.path.join(U.KV, f"layout{di}.json"), km.tok_to_id, km.blank_idx)
    assert [ln["box"] for ln in doc["lines"]] == before
    for other in (t2, t3):
        assert np.array_equal(other.line_rec, t.line_rec) and np.array_equal(other.glyph_rec, t.glyph_rec) and other.lines == t.lines


def test_golden_tables_have_the_counted_lines_and_glyphs(km):
    ts = [U.table_of(km, U.gold_layout(di)) for di in range(3)]
    assert [len(t.line_rec) for t in ts] == [11, 26, 9] and [len(t.glyph_rec) for t in ts] == [96, 257, 115]


# ---- 2: generated layouts ----------------------------------------------------------------------------------------------------
def test_paint_host_equals_painter_on_generated_layouts(km, tmp_path):
    cases = U.layout_cases()
    names = [n for n, _ in cases]
    for must in ("random_40", "gap_over_glyph", "nested", "one_line", "single_character", "past_right_edge", "zero_height", "lines_600"):
        assert must in names
    gaps = {}
    for name, doc in cases:
        t, want = _assert_same_document(km, doc, tmp_path, name)
        gaps[name] = U.gap_pixels(t, want)
    # the cases are what their names say
    assert gaps["gap_over_glyph"] > 0 and gaps["random_40"] > 0, gaps      # a later line's gap over an earlier line's character
    by = dict(cases)
    t = U.table_of(km, by["past_right_edge"])
    assert int(t.glyph_rec[:, 1].max()) > t.shape[1]                        # a span runs past column w
    assert (t.line_rec[:, 2] == t.line_rec[:, 0]).any()                     # a zero-width box with text
    t = U.table_of(km, by["zero_height"])
    assert ((t.line_rec[:, 3] == t.line_rec[:, 1]) & (t.line_rec[:, 5] > 0)).any()
    t = U.table_of(km, by["random_40"])
    assert (t.line_rec[:, 5] == 0).any() and (t.line_rec[:, 5] == 80).any()  # empty text, text far longer than its box
    toks = set(t.glyph_rec[:, 2].view(np.uint16).tolist())
    assert km.blank_idx in toks and km.tok_to_id["0"] in toks               # outside the charset, digits
    assert len(U.table_of(km, by["one_line"]).line_rec) == 1 and len(U.table_of(km, by["single_character"]).glyph_rec) == 1
    # overlapping line pairs of the random layout (rows and columns both)
    r = t.line_rec[t.line_rec[:, 5] > 0]
    pairs = sum(1 for i in range(len(r)) for j in range(i) if r[i, 1] < r[j, 3] and r[j, 1] < r[i, 3] and r[i, 6] < r[j, 7] and r[j, 6] < r[i, 7])
    assert pairs >= 10, pairs


def test_spans_are_the_painters_expressions(km):
    """the span of every glyph, recomputed per character with the painter's own expressions"""
    for _name, doc in U.layout_cases()[:3] + [("g", U.gold_layout(1))]:
        t = U.table_of(km, doc)
        for li, line in enumerate(t.lines):
            x1, y1, x2, y2 = line["box"]
            g0, n = int(t.line_rec[li, 4]), int(t.line_rec[li, 5])
            assert n == len(line["text"])
            if n == 0:
                continue
            pitch = max(1.0 * (x2 - x1) / n, 1.0)
            glyph_w = min(max(0.9 * pitch, 1.0), int((y2 - y1) * 1.2))
            for k in range(n):
                xs = x1 + k * pitch
                assert (int(xs), int(xs + glyph_w)) == tuple(int(v) for v in t.glyph_rec[g0 + k, :2])


# ---- 3: documents the table cannot represent ------------------------------------------------------------------------------------
def test_unrepresentable_documents_are_reported_not_painted(km):
    for name, doc in U.unrepresentable_layouts():
        t = U.table_of(km, doc)
        assert not t.ok and t.reason and t.line_rec is None and t.glyph_rec is None, name
        with pytest.raises(ValueError):
            G.paint_host(t)
    # in a group such a document takes part as one without lines: the kernel paints nothing wrong into it
    good = U.table_of(km, U.gold_layout(0))
    bad = U.table_of(km, U.unrepresentable_layouts()[0][1])
    records, off, sizes, canvas = G.pack_tables([good, bad, good])
    B = 3
    assert records[off["line_off"]:off["line_off"] + B + 1].tolist() == [0, 11, 11, 22]
    assert records[off["glyph_off"]:off["glyph_off"] + B + 1].tolist() == [0, 96, 96, 192]
    # a reversed box whose line has no text paints nothing in the painter either: representable
    empty_rev = {"lines": [U._line(0, 0, 40, 3, "fine"), U._line(30, 6, 10, 9, "")]}
    assert U.table_of(km, empty_rev).ok


# ---- 5: the wire ----------------------------------------------------------------------------------------------------------------
def test_wire_size_of_the_golden_documents(km):
    ts = [U.table_of(km, U.gold_layout(di)) for di in range(3)]
    glyphs, lines = 0, 0
    for t in ts:
        records, _off, _sizes, canvas = G.pack_tables([t], round_to=1)
        assert canvas == t.shape
        assert records.nbytes <= 8 * len(t.glyph_rec) + 32 * len(t.line_rec) + 64
        glyphs, lines = glyphs + len(t.glyph_rec), lines + len(t.line_rec)
    assert (glyphs, lines) == (468, 46)
    records, _off, sizes, canvas = G.pack_tables(ts)
    assert canvas == (80, 128) and sizes.tolist() == [[44, 91], [70, 128], [31, 102]]
    assert records.nbytes <= 8 * glyphs + 32 * lines + 64
    assert records.nbytes < 3 * 8 * 80 * 128 // 10                          # against 8 bytes per canvas pixel and document
    assert G.LINE_BYTES <= 32 and G.GLYPH_BYTES <= 8
    assert ts[0].line_rec.dtype == np.int32 and ts[0].line_rec.shape[1] * 4 == G.LINE_BYTES
    assert ts[0].glyph_rec.dtype == np.int16 and ts[0].glyph_rec.shape[1] * 2 == G.GLYPH_BYTES


# ---- 6: the C ABI and the flag -----------------------------------------------------------------------------------------------------
def test_library_exports_paint_symbol_and_version_stays():
    from msau_amd import _lib as L
    from msau_amd import build as B
    lib = L.load()
    assert "msau_kv_paint" in L.EXPORTED_SYMBOLS and lib.msau_kv_paint is not None
    assert lib.msau_version() == 11
    assert "int msau_kv_paint(" in open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    assert "paint.hip" in B.SOURCES


def test_device_masks_needs_device_post(km):
    f = os.path.join(U.KV, "layout0.json")
    for call in (lambda: km.predict((f, None), device_masks=True), lambda: km.predict_batch([f], device_masks=True),
                 lambda: km.run_test([f], "", device_masks=True), lambda: km.run_test([f], "", batch_size=2, device_masks=True)):
        with pytest.raises(ValueError, match="device_post"):
            call()


# ---- 4: the kernel's body as plain C++ ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("paint_cpu") / "libpaint_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_PAINT_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "paint.hip"), "-o", out], check=True)
    lib = C.CDLL(out)

    def run(tables, round_to=16):
        records, off, sizes, (H, W) = G.pack_tables(tables, round_to=round_to)
        B = len(tables)
        rng = np.random.default_rng(0)                                    # the kernel clears nothing: start from garbage
        ids = rng.integers(-5, 70, size=(B, H, W)).astype(np.int32)
        lm, cm = (rng.integers(0, 65536, size=(B, H, W)).astype(np.uint16) for _ in range(2))
        base = records.ctypes.data
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        at = lambda name: C.c_void_p(base + 4 * off[name])
        rc = lib.msau_kv_paint_cpu(at("lines"), at("glyphs"), at("line_off"), at("glyph_off"), at("sizes"), B, H, W, p(ids), p(lm), p(cm))
        assert rc == 0
        return (ids, lm, cm), (H, W)

    return run


def _assert_canvases(got, want, what):
    for plane, g_, w in zip(("ids", "line_ids", "char_pos"), got, want):
        assert g_.shape == w.shape and np.array_equal(g_, w), (what, plane, int((g_ != w).sum()))


def _all_tables(km):
    return [(f"layout{di}", U.table_of(km, U.gold_layout(di))) for di in range(3)] + \
           [(name, U.table_of(km, doc)) for name, doc in U.layout_cases()] + [("big", U.table_of(km, U.big_layout()))]


def test_cpu_form_of_kernel_dense(km, cpu_kernel):
    for name, t in _all_tables(km):
        got, canvas = cpu_kernel([t], round_to=1)
        assert canvas == t.shape
        _assert_canvases(got, U.canvases_want([t], canvas), name)


def test_cpu_form_of_kernel_ragged(km, cpu_kernel):
    named = _all_tables(km)
    tables = [t for _, t in named]
    assert len({t.shape for t in tables}) > 5                               # documents of different sizes on one canvas
    got, canvas = cpu_kernel(tables)
    want = U.canvases_want(tables, canvas)
    _assert_canvases(got, want, "ragged")
    for b, t in enumerate(tables):                                          # outside every document, beside a larger neighbour
        h, w = t.shape
        outside = np.ones(canvas, bool)
        outside[:h, :w] = False
        assert (got[0][b][outside] == -1).all() and not got[1][b][outside].any() and not got[2][b][outside].any()
        assert (got[0][b][:h, :w] >= 0).all()
    # small first, large second and the other way round; and with a document that has no table
    small, large = tables[2], tables[-1]
    bad = U.table_of(km, U.unrepresentable_layouts()[0][1])
    for group in ([small, large], [large, small], [small, bad, large]):
        got, canvas = cpu_kernel(group)
        want = U.canvases_want([t for t in group if t.ok], canvas)
        keep = [b for b, t in enumerate(group) if t.ok]
        _assert_canvases([g_[keep] for g_ in got], want, "pair")
        for b, t in enumerate(group):
            if not t.ok:                                                    # an empty document of its shape
                h, w = t.shape
                assert (got[0][b, :h, :w] == 0).all() and (got[0][b, h:] == -1).all() and (got[0][b, :, w:] == -1).all()
                assert not got[1][b].any() and not got[2][b].any()
