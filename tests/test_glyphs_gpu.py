"""The mask painter on the device (csrc/paint.hip) against `paint_host`, integer for integer, and KVModel's `device_masks=True`
path against `device_post=True` alone: results, `eval_results` and printed output, with and without fallbacks."""
import json
import os

import numpy as np
import pytest
import torch

from msau_amd.inference import glyphs as G
from msau_amd.inference import regions as R
from tests import glyphs_util as U
from tests.test_regions_gpu import _kv_model, _labels

pytestmark = pytest.mark.gpu
KV = U.KV


@pytest.fixture(scope="module")
def km():
    return U.charset_model()


def _device(tables, round_to=16):
    records, off, sizes, canvas = G.pack_tables(tables, round_to=round_to)
    # the kernel clears nothing: make sure the allocator hands it used memory
    junk = [torch.full((len(tables),) + canvas, 0x5A5A, dtype=dt, device="cuda") for dt in (torch.int32, torch.int16, torch.int16)]
    del junk
    ids, lm, cm = G.paint_device(records, off, sizes, canvas)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int32 and lm.dtype == torch.int16 and cm.dtype == torch.int16
    return (ids.cpu().numpy(), lm.cpu().numpy().view(np.uint16), cm.cpu().numpy().view(np.uint16)), canvas


def _assert_canvases(got, want, what):
    for plane, g_, w in zip(("ids", "line_ids", "char_pos"), got, want):
        assert g_.shape == w.shape and np.array_equal(g_, w), (what, plane, int((g_ != w).sum()))


def _named_tables(km):
    return [(f"layout{di}", U.table_of(km, U.gold_layout(di))) for di in range(3)] + \
           [(name, U.table_of(km, doc)) for name, doc in U.layout_cases()]


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_paint_host_dense(km):
    for name, t in _named_tables(km):
        got, canvas = _device([t], round_to=1)
        assert canvas == t.shape
        _assert_canvases(got, U.canvases_want([t], canvas), name)


def test_kernel_equals_paint_host_ragged(km):
    tables = [t for _, t in _named_tables(km)]
    got, canvas = _device(tables)
    _assert_canvases(got, U.canvases_want(tables, canvas), "ragged")
    for b, t in enumerate(tables):
        h, w = t.shape
        outside = np.ones(canvas, bool)
        outside[:h, :w] = False
        assert (got[0][b][outside] == -1).all() and not got[1][b][outside].any() and not got[2][b][outside].any()
    for group in ([tables[2], tables[3]], [tables[3], tables[2]], tables[::-1]):
        got, canvas = _device(group)
        _assert_canvases(got, U.canvases_want(group, canvas), "group")


def test_kernel_on_a_document_beyond_the_region_kernels_pixel_limit(km):
    big = U.table_of(km, U.big_layout())
    assert big.ok and big.shape[0] * big.shape[1] > R.device_limits()["max_pixels"]
    got, canvas = _device([big], round_to=1)
    _assert_canvases(got, U.canvases_want([big], canvas), "big dense")
    group = [U.table_of(km, U.gold_layout(0)), big, U.table_of(km, U.layout_cases()[0][1])]
    got, canvas = _device(group)
    _assert_canvases(got, U.canvases_want(group, canvas), "big ragged")


def test_consecutive_launches_leave_no_state(km):
    tables = [t for _, t in _named_tables(km)]
    a, _ = _device(tables[:4])
    b, _ = _device(tables[4:8])
    a2, _ = _device(tables[:4])
    _assert_canvases(a2, a, "again")
    _assert_canvases(b, U.canvases_want(tables[4:8], b[0].shape[1:]), "between")


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def _reset():
    for s in (R.STATS, G.STATS):
        for k in s:
            s[k] = 0


def _end_to_end(km, tmp_path, capsys, files, labels, many, arms=((True, False), (True, True))):
    out = {}
    for post, masks in arms:
        kw = dict(device_post=post, device_masks=masks)
        res = {}
        res["predict"] = [km.predict((f, None), **kw) for f in files]
        res["predict_batch"] = km.predict_batch(files, **kw)
        for bs in (1, 4):
            capsys.readouterr()
            r = km.run_test(many, str(tmp_path), label_dir=labels, batch_size=bs, **kw)
            res[f"run_test_{bs}"] = (r, json.loads(json.dumps(km.eval_results)), capsys.readouterr().out)
        out[masks] = res
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kvmodel_device_masks_equals_device_post(dtype, tmp_path, capsys):
    model = _kv_model(dtype, tmp_path)
    files = [os.path.join(KV, f"layout{i}.json") for i in range(3)]
    labels = _labels(tmp_path, files)
    many = files + files[:2]                                             # batch 4: a group of 4 and a group of 1
    _reset()
    out = _end_to_end(model, tmp_path, capsys, files, labels, many)
    assert out[True] == out[False]
    assert out[True]["predict"] == [(r, None) for r in out[True]["predict_batch"]]
    assert sum(c["num_label"] for c in out[True]["run_test_4"][1]) > 0 and "layout1" in out[True]["run_test_4"][2]
    assert any(r for r in out[True]["predict_batch"])                    # fields were found: the comparison is not of empty results
    assert R.STATS["fallbacks"] == 0 and G.STATS["host_painted"] == 0
    # predict x 3, predict_batch, run_test at 1 (5 documents) and at 4 (two groups): 16 documents in 11 launches
    assert G.STATS["documents"] == 16 and G.STATS["calls"] == 11
    assert G.STATS["h2d_bytes"] < 16 * 8 * 31 * 102 // 4                 # far below 8 bytes per pixel of the smallest document


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_kvmodel_device_masks_region_overflow_falls_back_exactly(tmp_path, capsys, monkeypatch):
    """lists far too short for the golden net's class maps: every document overflows and the host table takes over, from host
    masks painted then"""
    model = _kv_model("fp32", tmp_path)
    files = [os.path.join(KV, f"layout{i}.json") for i in range(3)]
    labels = _labels(tmp_path, files)
    want = _end_to_end(model, tmp_path, capsys, files, labels, files + files[:2], arms=((True, False),))[False]
    monkeypatch.setattr(R, "DEFAULT_CAP_REGIONS", 8)
    _reset()
    out = _end_to_end(model, tmp_path, capsys, files, labels, files + files[:2])
    assert R.STATS["fallbacks"] > 0 and G.STATS["host_painted"] == 0
    assert out[True] == out[False] == want


def test_kvmodel_unrepresentable_document_in_a_group(tmp_path, capsys):
    model = _kv_model("fp32", tmp_path)
    name, doc = U.unrepresentable_layouts()[0]
    assert not U.table_of(model, doc).ok
    bad = U.write_layout(doc, tmp_path / (name + ".json"))
    files = [os.path.join(KV, "layout0.json"), bad, os.path.join(KV, "layout2.json")]
    want = model.predict_batch(files, device_post=True)
    want_one = model.predict((bad, None), device_post=True)
    _reset()
    got = model.predict_batch(files, device_post=True, device_masks=True)
    assert got == want
    assert G.STATS["host_painted"] == 1 and G.STATS["documents"] == 3 and G.STATS["calls"] == 1
    assert model.predict((bad, None), device_post=True, device_masks=True) == want_one
    assert G.STATS["host_painted"] == 2
    # the canvases the forward read: the host painter's masks for that document, paint_host's for the others
    docs = [model._doc_for_paint(f) for f in files]
    records, off, sizes, canvas = G.pack_tables([t for _, t in docs])
    canv = G.paint_device(records, off, sizes, canvas)
    G.upload_host_masks(canv, 1, docs[1][0][:3])
    ids, lm, cm = canv[0].cpu().numpy(), canv[1].cpu().numpy().view(np.uint16), canv[2].cpu().numpy().view(np.uint16)
    for b, f in enumerate(files):
        c, l, p = model._generate_masks_from_label(f)[:3]
        h, w = c.shape
        assert np.array_equal(ids[b, :h, :w], c) and np.array_equal(lm[b, :h, :w], l) and np.array_equal(cm[b, :h, :w], p)
        assert (ids[b, h:] == -1).all() and (ids[b, :, w:] == -1).all() and not lm[b, h:].any() and not lm[b, :, w:].any()
