"""Region tables on the CPU: the host path (`regions_host` + `fields_from_regions`) against the reference's golden values and
against `KVModel._extract_value`, the closing and the numbering against scipy, the C ABI, and the kernel of csrc/regions.hip
built as plain C++ (-DMSAU_REGIONS_CPU: the same phases, lanes one after another) against `regions_host`."""
import copy
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage as ndi

from msau_amd.inference import KVModel, post_process_kv
from msau_amd.inference.morph_util import r_closing
from msau_amd.inference import regions as R
from tests import regions_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm(o):
    return json.loads(json.dumps(o, default=lambda v: v.item() if hasattr(v, "item") else list(v)))


@pytest.fixture(scope="module")
def gold():
    return U.load_gold()


# ---- 1: pinned to the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("di", [0, 1, 2])
def test_host_path_reproduces_reference_values(gold, di):
    g, meta = gold
    doc, lines = U.gold_doc(g, meta, di)
    values = R.fields_from_regions(R.regions_host(*doc, meta["n_class"]), lines, meta["n_class"])
    assert _norm(values) == meta[f"d{di}"]["values"]
    assert post_process_kv(values) == meta[f"d{di}"]["kv"]


# ---- 2: equal to _extract_value where lines are shared between fields -------------------------------------------------
def test_host_path_equals_extract_value_on_noisy_maps(gold):
    g, meta = gold
    n_class = meta["n_class"]
    rng = np.random.default_rng(0)
    shared = 0
    for t in range(30):
        di = t % 3
        md = meta[f"d{di}"]
        lm, cm = g[f"d{di}.line_mask"], g[f"d{di}.char_mask"]
        cls = U.blocky_map(rng, *lm.shape, n_class)
        pred = np.eye(n_class, dtype=np.float32)[cls]
        l1, l2 = copy.deepcopy(md["lines"]), copy.deepcopy(md["lines"])
        want, _ = KVModel._extract_value(lm, cm, l1, pred, n_class, pred_class=cls)
        table = R.regions_host(cls, lm, cm, [l["box"] for l in l2], n_class)
        got = R.fields_from_regions(table, l2, n_class)
        assert _norm(got) == _norm(want), t
        assert l1 == l2                                                  # the same line ids were set
        # lines under more than one class's regions: the character-span branch
        owners = {}
        for c, (_comps, pairs) in table.items():
            for (_k, v), p in pairs.items():
                if p[0] > 0:
                    owners.setdefault(v, set()).add(c)
        shared += sum(len(s) > 1 for s in owners.values())
    assert shared > 30, shared


def test_claimed_twice_branch_is_reached(gold):
    """a line under the kept regions of two fields: both fields take a character span, as `_extract_value` does"""
    g, meta = gold
    n_class = meta["n_class"]
    lm, cm = g["d1.line_mask"], g["d1.char_mask"]
    lines = copy.deepcopy(meta["d1"]["lines"])
    li = int(np.argmax([l["box"][2] - l["box"][0] for l in lines]))
    x1, y1, x2, y2 = lines[li]["box"]
    mid = (x1 + x2) // 2
    cls = np.zeros(lm.shape, int)
    cls[y1:y2, x1:mid] = 3
    cls[y1:y2, mid:x2] = 4
    l1, l2 = copy.deepcopy(lines), copy.deepcopy(lines)
    want, _ = KVModel._extract_value(lm, cm, l1, np.eye(n_class, dtype=np.float32)[cls], n_class, pred_class=cls)
    got = R.fields_from_regions(R.regions_host(cls, lm, cm, [l["box"] for l in l2], n_class), l2, n_class)
    assert _norm(got) == _norm(want)
    text = lines[li]["text"]
    assert got[3][0] and got[4][0] and got[3][0] != text and got[4][0] != text and got[3][0] in text and got[4][0] in text


# ---- 3: closing and numbering ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4, 7, 33])
def test_closing_written_out_equals_r_closing(w):
    rng = np.random.default_rng(w)
    for h in (1, 2, 5):
        for density in (0.2, 0.5, 0.9):
            m = rng.random((h, w)) < density
            want = r_closing(m, (1, 3))
            assert np.array_equal(R.closing_1x3(m), want)
            assert not want[:, 0].any() and not want[:, -1].any()
    if w <= 4:                                                           # every mask of one row
        for bits in range(1 << w):
            m = np.array([[(bits >> i) & 1 for i in range(w)]], dtype=bool)
            assert np.array_equal(R.closing_1x3(m), r_closing(m, (1, 3)))


def test_region_numbering_is_scipys(gold):
    g, meta = gold
    rng = np.random.default_rng(3)
    cls = U.blocky_map(rng, 40, 60, 6, flip=0.1)
    lm, cm, boxes = U.synthetic_lines(rng, 40, 60, 10)
    table = R.regions_host(cls, lm, cm, boxes, 6)
    for c in range(2, 6):
        lab, n = ndi.label(r_closing(cls == c, (1, 3)))
        comps = table[c][0]
        assert len(comps) == n
        firsts = [fy * 60 + fx for fy, fx, *_ in comps]
        assert firsts == sorted(firsts)
        for k, (fy, fx, y0, y1, x0, x1, npix) in enumerate(comps):
            assert lab[fy, fx] == k + 1 and (fy * 60 + fx) == np.flatnonzero(lab == k + 1)[0]
            assert (slice(y0, y1), slice(x0, x1)) == ndi.find_objects(lab)[k] and npix == int((lab == k + 1).sum())


# ---- 4: the C ABI ---------------------------------------------------------------------------------------------------
def test_library_exports_region_symbols_and_version_stays():
    from msau_amd import _lib as L
    lib = L.load()
    assert "msau_kv_regions" in L.EXPORTED_SYMBOLS and "msau_kv_regions_limits" in L.EXPORTED_SYMBOLS
    assert lib.msau_kv_regions is not None and lib.msau_kv_regions_limits is not None
    assert lib.msau_version() == 11
    lim = R.device_limits()
    assert lim["max_pixels"] >= 24576 and lim["region_ints"] == 8 and lim["pair_ints"] == 4
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    assert "int msau_kv_regions(" in header and "int msau_kv_regions_limits(" in header


def test_pack_masks_and_pack_ids_unchanged():
    from msau_amd.data.ragged import pack_ids, pack_masks
    a, b = np.arange(6, dtype=np.uint16).reshape(2, 3) + 65530, np.ones((5, 2), np.uint16)
    ids, sizes = pack_ids([a, b])
    assert ids.dtype.is_signed and tuple(ids.shape) == (2, 16, 16) and int(ids[0, 0, 0]) == 65530 and int(ids[0, 5, 5]) == -1
    t, sizes2 = pack_masks([a, b])
    assert sizes2.tolist() == sizes.tolist() == [[2, 3], [5, 2]] and tuple(t.shape) == (2, 16, 16) and t.element_size() == 2
    back = t.numpy().view(np.uint16)
    assert np.array_equal(back[0, :2, :3], a) and np.array_equal(back[1, :5, :2], b)
    back[0, :2, :3] = 0
    back[1, :5, :2] = 0
    assert not back.any()
    with pytest.raises(ValueError):
        pack_masks([])


# ---- the kernel's body as plain C++ ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("regions_cpu") / "libregions_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_REGIONS_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "regions.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lim = (C.c_int32 * 6)()
    lib.msau_kv_regions_limits(lim)

    def run(docs, n_class, cap_regions=R.DEFAULT_CAP_REGIONS, cap_pairs=R.DEFAULT_CAP_PAIRS, ragged=True):
        am, lm, cm, sizes = U.pack_canvas(docs, n_class)
        B, H, W = am.shape
        boxes = np.array([b for d in docs for b in d[3]] or [[0, 0, 0, 0]], dtype=np.int32)
        off = np.cumsum([0] + [len(d[3]) for d in docs]).astype(np.int32)
        ext = np.ascontiguousarray(sizes.astype(np.int32))
        header, ovf = np.zeros((B, n_class, 4), np.int32), np.zeros(B, np.int32)
        reg, pairs = np.zeros((B, cap_regions, 8), np.int32), np.zeros((B, cap_pairs, 4), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.msau_kv_regions_cpu(p(am), p(lm), p(cm), p(boxes), p(off), p(ext) if ragged else None, B, H, W, n_class,
                                     p(header), p(reg), cap_regions, p(pairs), cap_pairs, p(ovf))
        assert rc == 0
        return [R.table_from_records(header[b], reg[b], pairs[b], n_class) if ovf[b] == 0 else None for b in range(B)], ovf.tolist()

    run.limits = list(lim)
    return run


def test_cpu_form_of_kernel_on_goldens_and_net_map(gold, cpu_kernel):
    g, meta = gold
    n_class = meta["n_class"]
    docs = [U.gold_doc(g, meta, di)[0] for di in range(3)]
    d0 = docs[0]
    docs.append((np.argmax(g["net.pred_nhwc"], -1),) + d0[1:])
    want = [R.regions_host(*d, n_class) for d in docs]
    got, ovf = cpu_kernel(docs, n_class)
    assert ovf == [0] * 4
    assert got == want
    assert U.counts(want[3])[0] == 929


def test_cpu_form_of_kernel_on_shapes(cpu_kernel):
    max_pixels = cpu_kernel.limits[0]
    for name, doc, n_class in U.shape_cases(max_pixels):
        want = R.regions_host(*doc, n_class)
        got, ovf = cpu_kernel([doc], n_class)
        assert ovf == [0], (name, ovf)
        assert got[0] == want, name
    # one ragged canvas, neighbours holding other classes right up to every extent
    cases = [c for c in U.shape_cases(max_pixels) if c[2] <= 6 and c[0] != "pixel_limit"]
    docs = [c[1] for c in cases]
    got, ovf = cpu_kernel(docs, 6)
    assert ovf == [0] * len(docs)
    assert got == [R.regions_host(*d, 6) for d in docs]


def test_cpu_form_of_kernel_overflow_flags(gold, cpu_kernel):
    g, meta = gold
    rng = np.random.default_rng(5)
    quiet = U.gold_doc(g, meta, 1)[0]
    noise = (rng.integers(0, 17, size=(70, 128)),) + quiet[1:]
    big = U.with_lines(U.blocky_map(rng, 130, 192, 17), 3)                # 24 960 pixels: above the limit
    assert big[0].size > cpu_kernel.limits[0]
    assert U.counts(R.regions_host(*noise, 17))[0] > 2048
    caps = dict(cap_regions=2048, cap_pairs=2048)
    got, ovf = cpu_kernel([quiet, noise, big, quiet], 17, **caps)
    assert ovf[0] == 0 and ovf[3] == 0 and ovf[1] & R.OVF_REGIONS and ovf[2] == R.OVF_PIXELS
    assert got[0] == got[3] == R.regions_host(*quiet, 17) and got[1] is None and got[2] is None
    # a pair list that is too short, a region list that just fits
    nr, _, npair, _ = U.counts(R.regions_host(*quiet, 17))
    got, ovf = cpu_kernel([quiet], 17, cap_regions=nr, cap_pairs=npair - 1)
    assert ovf == [R.OVF_PAIRS]
    got, ovf = cpu_kernel([quiet], 17, cap_regions=nr, cap_pairs=npair)
    assert ovf == [0] and got[0] == R.regions_host(*quiet, 17)
    # a line id beyond the box list
    bad = (quiet[0], quiet[1], quiet[2], quiet[3][:3])
    assert cpu_kernel([bad], 17)[1] == [R.OVF_LINES]
