"""A confidence per region on the CPU: the scored form of the kernel of csrc/regions.hip built as plain C++ (-DMSAU_REGIONS_CPU, as
tests/test_regions_cpu.py builds the file) against `regions_host(..., probs=)`, integer for integer; the rows it may and may not
write; the 64-bit sum of the large form; `field_confidences` and the selection it shares with `fields_from_regions`; the
quantisation in fp32 and in float64.  Nothing here has a tolerance: every compared quantity is an integer or a float64 computed
from integers."""
import copy
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from msau_amd.inference import KVModel, post_process_kv, post_process_kv_scored
from msau_amd.inference import regions as R
from tests import regions_util as U
from tests.regions_large_util import large_cases
from tests.regions_scored_util import doc_probs, full_doc, pack_probs, quarter_doc, score_rows, scored_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("regions_scored_cpu") / "libregions_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_REGIONS_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "regions.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lim = (C.c_int32 * 6)()
    lib.msau_kv_regions_limits(lim)
    max_pixels = int(lim[0])

    def run(docs, probs, n_class, cap_regions=R.DEFAULT_CAP_REGIONS, cap_pairs=R.DEFAULT_CAP_PAIRS, ragged=True, outside=None,
            large=False, buffers=None):
        """the scored LDS launch (then, with `large`, the scored large one for the documents over the pixel limit) and the
        unscored ones on buffers of their own -> dict of the arrays of both; `buffers`: a former result whose arrays are reused"""
        am, lm, cm, sizes = U.pack_canvas(docs, n_class, round_to=16 if ragged else 1, neighbours=ragged)
        pr = pack_probs(probs, am.shape, n_class, outside)
        B, H, W = am.shape
        boxes = np.array([b for d in docs for b in d[3]] or [[0, 0, 0, 0]], dtype=np.int32)
        off = np.cumsum([0] + [len(d[3]) for d in docs]).astype(np.int32)
        ext = np.ascontiguousarray(sizes.astype(np.int32))
        out = {}
        for form in ("scored", "plain"):
            if buffers is not None:
                bufs = buffers[form]
            else:
                bufs = dict(header=np.zeros((B, n_class, 4), np.int32), ovf=np.zeros(B, np.int32),
                            reg=np.full((B, cap_regions, 8), -7, np.int32), pairs=np.full((B, cap_pairs, 4), -7, np.int32))
                if form == "scored":
                    bufs["scores"] = np.full((B, cap_regions), -1, np.int64)
            tail = (_p(ext) if ragged else None, B, H, W, n_class)
            outs = (_p(bufs["header"]), _p(bufs["reg"]), cap_regions, _p(bufs["pairs"]), cap_pairs)
            if form == "scored":
                ins, outs = (_p(am), _p(pr), _p(lm), _p(cm), _p(boxes), _p(off)), outs + (_p(bufs["scores"]), _p(bufs["ovf"]))
                fns = (lib.msau_kv_regions_scored_cpu, lib.msau_kv_regions_large_scored_cpu)
            else:
                ins, outs = (_p(am), _p(lm), _p(cm), _p(boxes), _p(off)), outs + (_p(bufs["ovf"]),)
                fns = (lib.msau_kv_regions_cpu, lib.msau_kv_regions_large_cpu)
            assert fns[0](*ins, *tail, *outs) == 0
            if large:
                listed = [b for b, d in enumerate(docs) if d[0].size > max_pixels]
                share = [(n_class - 2) * docs[b][0].size for b in listed]
                ws_off = np.concatenate([[0], np.cumsum(share)[:-1]]).astype(np.int64)
                ws = np.zeros(int(sum(share)), np.int32)
                assert fns[1](*ins, *tail, _p(np.array(listed, np.int32)), len(listed), _p(ws_off), _p(ws), C.c_int64(ws.size), *outs) == 0
            out[form] = bufs
        return out

    run.lib, run.max_pixels = lib, max_pixels
    return run


def _assert_equals_host(out, docs, probs, n_class):
    """flags clear, scores equal to the host statement's as int64, and header / regions / pairs the unscored entry's bytes"""
    s, p = out["scored"], out["plain"]
    assert s["ovf"].tolist() == [0] * len(docs) and p["ovf"].tolist() == [0] * len(docs)
    for name in ("header", "reg", "pairs"):
        assert s[name].tobytes() == p[name].tobytes(), name
    for b, (d, pr) in enumerate(zip(docs, probs)):
        table, want = R.regions_host(*d, n_class, probs=pr)
        assert R.table_from_records(s["header"][b], s["reg"][b], s["pairs"][b], n_class) == table
        assert table == R.regions_host(*d, n_class)                      # the table does not depend on probs
        for c in range(2, n_class):
            roff, nr = s["header"][b, c, 0], s["header"][b, c, 1]
            got = s["scores"][b, roff:roff + nr]
            assert got.dtype == np.int64 and np.array_equal(got, np.array(want[c], dtype=np.int64)), (b, c)
            assert (s["reg"][b, roff:roff + nr, 7] == c).all()


# ---- scores against the host statement -------------------------------------------------------------------------------------
def test_scored_cpu_form_equals_host_statement_on_shapes(cpu_kernel):
    cases = scored_cases(cpu_kernel.max_pixels)
    names = [c[0] for c in cases]
    for must in ("spiral", "comb", "blocky", "pixel_limit", "n_class_40", "thin_1x9", "ties"):
        assert must in names
    regions = 0
    for name, doc, n_class, pr in cases:
        assert np.array_equal(np.argmax(pr, -1), doc[0]) or name == "ties", name
        out = cpu_kernel([doc], [pr], n_class, ragged=False)
        _assert_equals_host(out, [doc], [pr], n_class)
        regions += int(out["scored"]["header"][0, 0, 0])
    assert regions > 1000


def test_scored_cpu_form_sums_the_gap_pixels_with_their_own_probability(cpu_kernel):
    """1 x 3 closing: a gap pixel of another class belongs to the region and counts with the probability of the region's class
    it has, so the patched-up region scores lower than its pixel count at p = 1"""
    cls = np.zeros((3, 12), int)
    cls[1, 2:9] = 2
    cls[1, 5] = 0                                                        # the gap
    pr = np.zeros((3, 12, 3), np.float32)
    pr[..., 0] = 1.0
    pr[1, 2:9] = (0.0, 0.0, 1.0)
    pr[1, 5] = (0.75, 0.0, 0.25)
    doc = U.with_lines(cls, 1, n_lines=2)
    out = cpu_kernel([doc], [pr], 3, ragged=False)
    _assert_equals_host(out, [doc], [pr], 3)
    assert out["scored"]["reg"][0, 0, 6] == 7 and out["scored"]["scores"][0, 0] == 6 * 65536 + 16384


# ---- guard rows ------------------------------------------------------------------------------------------------------------
def test_scored_cpu_form_writes_its_reserved_rows_and_no_other(cpu_kernel):
    rng = np.random.default_rng(31)
    many = U.with_lines(U.blocky_map(rng, 48, 72, 6, flip=0.2), 32)
    few = U.with_lines(U.blocky_map(rng, 48, 72, 6, flip=0.0), 33)
    p_many, p_few = doc_probs(rng, many[0], 6), doc_probs(rng, few[0], 6)
    n_many, n_few = U.counts(R.regions_host(*many, 6))[0], U.counts(R.regions_host(*few, 6))[0]
    assert n_many > 4 * n_few > 0
    out = cpu_kernel([many], [p_many], 6, ragged=False)
    _assert_equals_host(out, [many], [p_many], 6)
    sc, hd = out["scored"]["scores"], out["scored"]["header"]
    rows = score_rows(hd[0], 6)
    assert len(rows) == n_many == hd[0, 0, 0]
    assert (sc[0, rows] >= 0).all()
    assert (np.delete(sc[0], rows) == -1).all()
    # the same buffers again, a map of fewer regions: its reserved rows hold its own sums, no row beyond them is touched
    before = sc.copy()
    out = cpu_kernel([few], [p_few], 6, ragged=False, buffers=out)
    _assert_equals_host(out, [few], [p_few], 6)
    rows = score_rows(out["scored"]["header"][0], 6)
    assert len(rows) == n_few
    assert np.array_equal(np.delete(out["scored"]["scores"][0], rows), np.delete(before[0], rows))


def test_scored_cpu_form_overflow_leaves_scores_alone(cpu_kernel):
    """a document whose region list is too short: flagged, and not a score row written (its class slices are not reserved in range)"""
    rng = np.random.default_rng(34)
    doc = U.with_lines(U.blocky_map(rng, 48, 72, 6, flip=0.2), 35)
    pr = doc_probs(rng, doc[0], 6)
    out = cpu_kernel([doc], [pr], 6, ragged=False, cap_regions=4)
    assert out["scored"]["ovf"][0] & R.OVF_REGIONS and out["plain"]["ovf"].tolist() == out["scored"]["ovf"].tolist()
    written = out["scored"]["scores"][0] != -1
    assert written.sum() <= 4                                            # (a class that reserved inside the list wrote its rows)


# ---- ragged canvas ---------------------------------------------------------------------------------------------------------
def test_scored_cpu_form_ragged_canvas_nothing_leaks_in(cpu_kernel):
    cases = [c for c in scored_cases(cpu_kernel.max_pixels) if c[2] <= 6 and c[0] not in ("pixel_limit", "ties")]
    assert len(cases) >= 8
    docs = [c[1] for c in cases]
    rng = np.random.default_rng(36)
    probs = [doc_probs(rng, d[0], 6) for d in docs]                      # (every document at n_class = 6)
    out = cpu_kernel(docs, probs, 6, ragged=True, outside=1.0)           # p = 1 for every class outside the documents
    _assert_equals_host(out, docs, probs, 6)


# ---- saturation and the large form -----------------------------------------------------------------------------------------
def test_scored_cpu_form_saturation_at_the_pixel_limit(cpu_kernel):
    doc, pr = full_doc(cpu_kernel.max_pixels // 192, 192)
    assert doc[0].size == cpu_kernel.max_pixels
    out = cpu_kernel([doc], [pr], 3, ragged=False)
    _assert_equals_host(out, [doc], [pr], 3)
    s = out["scored"]
    assert s["header"][0, 2].tolist()[:2] == [0, 1]
    pixels = int(s["reg"][0, 0, 6])
    assert pixels == (cpu_kernel.max_pixels // 192) * 190 and s["scores"][0, 0] == pixels * 65536


def test_scored_large_cpu_form_sums_in_64_bits(cpu_kernel):
    doc, pr = full_doc(260, 260)
    out = cpu_kernel([doc], [pr], 3, ragged=False, large=True)
    _assert_equals_host(out, [doc], [pr], 3)
    s = out["scored"]
    assert int(s["reg"][0, 0, 6]) == 260 * 258 == 67080
    assert int(s["scores"][0, 0]) == 67080 * 65536 > 2 ** 32


@pytest.mark.parametrize("name", [c[0] for c in large_cases()])
def test_scored_large_cpu_form_equals_host_statement(cpu_kernel, name):
    _, doc, n_class = next(c for c in large_cases() if c[0] == name)
    assert doc[0].size > cpu_kernel.max_pixels
    pr = doc_probs(np.random.default_rng(37), doc[0], n_class)
    _assert_equals_host(cpu_kernel([doc], [pr], n_class, ragged=False, large=True), [doc], [pr], n_class)


def test_scored_large_cpu_form_in_a_ragged_group(cpu_kernel):
    """a small and a large document on one canvas, p = 1 outside: the LDS launch scores the small one, the large launch the other"""
    rng = np.random.default_rng(38)
    docs = [U.with_lines(U.blocky_map(rng, 48, 72, 5), 39), next(c[1] for c in large_cases() if c[0] == "300x256")]
    probs = [doc_probs(rng, d[0], 5) for d in docs]
    out = cpu_kernel(docs, probs, 5, ragged=True, outside=1.0, large=True)
    _assert_equals_host(out, docs, probs, 5)


def test_scored_cpu_entries_refuse_null_probs_or_scores(cpu_kernel):
    lib = cpu_kernel.lib
    doc, pr = full_doc(8, 8)
    am, lm, cm, sizes = U.pack_canvas([doc], 3, round_to=1, neighbours=False)
    boxes, off = np.array(doc[3], np.int32), np.array([0, len(doc[3])], np.int32)
    header, ovf = np.zeros((1, 3, 4), np.int32), np.zeros(1, np.int32)
    reg, pairs, scores = np.zeros((1, 8, 8), np.int32), np.zeros((1, 8, 4), np.int32), np.full((1, 8), -1, np.int64)
    for probs_p, scores_p in ((None, _p(scores)), (_p(pr), None)):
        assert lib.msau_kv_regions_scored_cpu(_p(am), probs_p, _p(lm), _p(cm), _p(boxes), _p(off), None, 1, 8, 8, 3, _p(header), _p(reg), 8,
                                              _p(pairs), 8, scores_p, _p(ovf)) != 0
        assert (scores == -1).all() and not header.any()


def test_library_and_header_name_the_scored_entries():
    from msau_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    for name in ("msau_kv_regions_scored", "msau_kv_regions_large_scored"):
        assert name in L.EXPORTED_SYMBOLS and f"int {name}(" in header
    lib = L.load()
    assert lib.msau_kv_regions_scored is not None and lib.msau_kv_regions_large_scored is not None and lib.msau_version() == 11
    assert R.device_limits()["region_ints"] == 8


# ---- field_confidences -----------------------------------------------------------------------------------------------------
def _norm(o):
    return json.loads(json.dumps(o, default=lambda v: v.item() if hasattr(v, "item") else list(v)))


@pytest.mark.parametrize("di", [0, 1, 2])
def test_field_confidences_on_the_golden_documents(di):
    g, meta = U.load_gold()
    n_class = meta["n_class"]
    doc, lines = U.gold_doc(g, meta, di)
    pr = doc_probs(np.random.default_rng(40 + di), doc[0], n_class)
    table, scores = R.regions_host(*doc, n_class, probs=pr)
    values = R.fields_from_regions(table, lines, n_class)
    assert _norm(values) == meta[f"d{di}"]["values"]                      # the reference's own values, as before the selection moved
    conf = R.field_confidences(table, scores, copy.deepcopy(lines), n_class)
    assert len(conf) == n_class and sum(c is not None for c in conf) > 0
    for c in range(n_class):
        if values[c][1] is None:
            assert conf[c] is None
        else:
            assert isinstance(conf[c], float) and 0.0 <= conf[c] <= 1.0
    kv = post_process_kv_scored(values, conf)
    plain = post_process_kv(values)
    assert list(kv) == list(plain) and {k: v["text"] for k, v in kv.items()} == plain == meta[f"d{di}"]["kv"]
    assert [v["confidence"] for v in kv.values()] == [conf[idx] for idx in range(3, n_class, 2)]


def test_fields_from_regions_still_equals_extract_value_on_noisy_maps():
    """the selection is shared now (`select_regions`): values and line ids as `_extract_value` gives them, on maps where lines are
    shared between fields and the multi-line fields have extra regions"""
    g, meta = U.load_gold()
    n_class = meta["n_class"]
    rng = np.random.default_rng(41)
    fields = extras = 0
    for t in range(12):
        di = t % 3
        lm, cm = g[f"d{di}.line_mask"], g[f"d{di}.char_mask"]
        cls = U.blocky_map(rng, *lm.shape, n_class)
        l1, l2, l3 = (copy.deepcopy(meta[f"d{di}"]["lines"]) for _ in range(3))
        want, _ = KVModel._extract_value(lm, cm, l1, np.eye(n_class, dtype=np.float32)[cls], n_class, pred_class=cls)
        pr = doc_probs(rng, cls, n_class)
        table, scores = R.regions_host(cls, lm, cm, [l["box"] for l in l2], n_class, probs=pr)
        got = R.fields_from_regions(table, l2, n_class)
        assert _norm(got) == _norm(want) and l1 == l2, t
        conf = R.field_confidences(table, scores, l3, n_class)
        assert l3 == l2
        assert [c is not None for c in conf] == [v[1] is not None for v in got]
        kept = R.select_regions(table, l3, n_class)[0]
        for c in range(2, n_class):
            if conf[c] is not None:                                       # restated from the definition, in exact integers
                num, den = sum(scores[c][k] for k in kept[c]), 65536 * sum(table[c][0][k][6] for k in kept[c])
                assert conf[c] == num / den and 0 < num <= den
                fields += 1
                extras += len(kept[c]) - 1
    assert fields > 30 and extras > 5


def test_field_confidence_of_one_region_at_three_quarters():
    doc, pr, lines = quarter_doc()
    table, scores = R.regions_host(*doc, 4, probs=pr)
    assert [len(table[c][0]) for c in (2, 3)] == [0, 1] and scores[3] == [table[3][0][0][6] * 49152]
    values = R.fields_from_regions(table, lines, 4)
    assert values[3][0] == "hello world"
    assert R.field_confidences(table, scores, lines, 4) == [None, None, None, 0.75]
    assert post_process_kv_scored(values, [None, None, None, 0.75]) == {"bank_name": {"text": "hello world", "confidence": 0.75}}


def test_regions_host_without_probs_is_unchanged_and_checks_probs():
    doc, pr, _ = quarter_doc()
    assert isinstance(R.regions_host(*doc, 4), dict)
    with pytest.raises(ValueError):
        R.regions_host(*doc, 4, probs=pr.astype(np.float64))
    with pytest.raises(ValueError):
        R.regions_host(*doc, 4, probs=pr[:, :, :3])


# ---- quantisation ----------------------------------------------------------------------------------------------------------
def test_quantisation_is_bit_equal_in_fp32_and_float64():
    rng = np.random.default_rng(42)
    tiny = np.array([0.0, 1.0, 2.0 ** -17, 3 * 2.0 ** -17, 5 * 2.0 ** -17, 2.0 ** -18, 1.0 - 2.0 ** -24, 0.5, 0.75,
                     np.finfo(np.float32).tiny, 1e-45, 1e-40, 2.0 ** -126, 2.0 ** -149], dtype=np.float32)
    p = np.concatenate([tiny, rng.random(100000, dtype=np.float32),
                        (rng.integers(0, 65536, size=20000) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -17)])   # ties
    assert p.dtype == np.float32 and p.min() >= 0 and p.max() <= 1
    q32 = np.rint(p * np.float32(65536.0))
    assert q32.dtype == np.float32
    q64 = np.rint(p.astype(np.float64) * 65536)
    assert np.array_equal(q32.astype(np.int64), q64.astype(np.int64)) and np.array_equal(q64.astype(np.int64), R.quantise(p))
    assert np.array_equal(p.astype(np.float64) * 65536, (p * np.float32(65536.0)).astype(np.float64))     # the product is exact
    assert R.quantise(tiny[:6]).tolist() == [0, 65536, 0, 2, 2, 0]        # ties go to the even integer
    assert int(R.quantise(np.float32(2.0 ** -149))) == 0
