"""The large form of the region kernel (csrc/regions.hip, `msau_kv_regions_large`: the labels in a workspace, not in LDS) built as
plain C++ (-DMSAU_REGIONS_CPU, as tests/test_regions_cpu.py builds the file) against `regions_host`, integer for integer, on
documents of more pixels than the LDS form holds.  Before a comparison every test asserts, from scipy's own counts, that the
document is over the pixel limit and fits the per-class limits and the capacities it passes: a refusal cannot hide a wrong table."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from msau_amd.inference import regions as R
from tests import regions_util as U
from tests.regions_large_util import large_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("regions_large_cpu") / "libregions_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_REGIONS_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "regions.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lim = (C.c_int32 * 6)()
    lib.msau_kv_regions_limits(lim)
    max_pixels = int(lim[0])

    def run(docs, n_class, cap_regions=R.DEFAULT_CAP_REGIONS, cap_pairs=R.DEFAULT_CAP_PAIRS, ragged=True, listed=None, short_by=0,
            neighbours=True):
        """the LDS launch, then the large one for `listed` (default: the documents over the pixel limit)
        -> (tables, flags, state after the first launch, state after the second, status of the second)"""
        am, lm, cm, sizes = U.pack_canvas(docs, n_class, round_to=16 if ragged else 1, neighbours=neighbours and ragged)
        B, H, W = am.shape
        boxes = np.array([b for d in docs for b in d[3]] or [[0, 0, 0, 0]], dtype=np.int32)
        off = np.cumsum([0] + [len(d[3]) for d in docs]).astype(np.int32)
        ext = np.ascontiguousarray(sizes.astype(np.int32))
        header, ovf = np.zeros((B, n_class, 4), np.int32), np.zeros(B, np.int32)
        reg, pairs = np.full((B, cap_regions, 8), -7, np.int32), np.full((B, cap_pairs, 4), -7, np.int32)
        args = (_p(am), _p(lm), _p(cm), _p(boxes), _p(off), _p(ext) if ragged else None, B, H, W, n_class)
        outs = (_p(header), _p(reg), cap_regions, _p(pairs), cap_pairs, _p(ovf))
        assert lib.msau_kv_regions_cpu(*args, *outs) == 0
        first = [a.copy() for a in (header, reg, pairs, ovf)]
        if listed is None:
            listed = [b for b, d in enumerate(docs) if d[0].size > max_pixels]
        share = [(n_class - 2) * docs[min(b, B - 1)][0].size for b in listed]
        ws_off = np.concatenate([[0], np.cumsum(share)[:-1]]).astype(np.int64)
        ws_ints = int(sum(share)) - short_by
        ws = np.full(max(ws_ints, 1) + 64, -99, np.int32)                  # 64 guard words behind what the call is told of
        rc = lib.msau_kv_regions_large_cpu(*args, _p(np.array(listed, np.int32)), len(listed), _p(ws_off), _p(ws), C.c_int64(ws_ints), *outs)
        assert (ws[max(ws_ints, 0):] == -99).all()
        tables = [R.table_from_records(header[b], reg[b], pairs[b], n_class) if ovf[b] == 0 else None for b in range(B)]
        return tables, ovf.tolist(), first, [header, reg, pairs, ovf], rc

    run.max_pixels = max_pixels
    run.max_regions, run.max_pairs = int(lim[1]), int(lim[2])
    return run


def _assert_large_fits(run, want, doc, cap_regions=R.DEFAULT_CAP_REGIONS, cap_pairs=R.DEFAULT_CAP_PAIRS):
    nr, nr_class, npair, npair_class = U.counts(want)
    assert doc[0].size > run.max_pixels
    assert nr <= cap_regions and nr_class <= run.max_regions, (nr, nr_class)
    assert npair <= cap_pairs and npair_class <= run.max_pairs, (npair, npair_class)
    assert all(0 <= int(v) <= len(doc[3]) for v in np.unique(doc[1]))


def _check(run, doc, n_class, ragged):
    want = R.regions_host(*doc, n_class)
    _assert_large_fits(run, want, doc)
    got, ovf, first, _, rc = run([doc], n_class, ragged=ragged)
    assert first[3].tolist() == [R.OVF_PIXELS]                          # the LDS form refuses it, as before
    assert rc == 0 and ovf == [0], ovf
    assert got[0] == want
    return want


@pytest.fixture(scope="module")
def cases():
    return large_cases()


@pytest.mark.parametrize("name", [c[0] for c in large_cases()])
def test_large_cpu_form_equals_regions_host(cpu_kernel, cases, name):
    _, doc, n_class = next(c for c in cases if c[0] == name)
    want = _check(cpu_kernel, doc, n_class, ragged=False)
    nr, nr_class, npair, _ = U.counts(want)
    if name in ("spiral", "comb"):
        c = 3 if name == "spiral" else 2
        assert nr == 1 and want[c][0][0][6] == int(R.closing_1x3(doc[0] == c).sum()) > 1000
    if name == "full":
        assert want[2][0] == [(0, 1, 0, 160, 1, 159, 160 * 158)]
    if name == "empty":
        assert nr == 0
    if name in ("overflow_test_map", "257x191", "300x256"):
        assert nr > 1000 and nr_class > 90 and npair > 100                 # many regions per class, lines shared between them
    if name.startswith("thin") and not name.endswith("x1"):
        assert nr > 100
    if name != "overflow_test_map":                                       # (that one: in the ragged group below)
        _check(cpu_kernel, doc, n_class, ragged=True)


def test_large_cpu_form_ragged_group_leaves_small_documents_alone(cpu_kernel, cases):
    g, meta = U.load_gold()
    by = {c[0]: c[1] for c in cases}
    small = [U.gold_doc(g, meta, 1)[0], U.with_lines(U.blocky_map(np.random.default_rng(40), 48, 72, 17), 41)]
    docs = [small[0], by["257x191"], small[1], by["overflow_test_map"]]
    want = [R.regions_host(*d, 17) for d in docs]
    for b in (1, 3):
        _assert_large_fits(cpu_kernel, want[b], docs[b])
    got, ovf, first, last, rc = cpu_kernel(docs, 17)
    assert rc == 0 and first[3].tolist() == [0, R.OVF_PIXELS, 0, R.OVF_PIXELS] and ovf == [0] * 4
    assert got == want
    for b in (0, 2):                                                      # header rows, both lists, flag: not a word changed
        for a0, a1 in zip(first, last):
            assert np.array_equal(a0[b], a1[b])
    # only the listed document is redone
    got, ovf, first, last, rc = cpu_kernel(docs, 17, listed=[3])
    assert rc == 0 and ovf == [0, R.OVF_PIXELS, 0, 0] and got[3] == want[3] and got[0] == want[0] and got[2] == want[2]
    for a0, a1 in zip(first, last):
        assert np.array_equal(a0[1], a1[1])


def test_large_cpu_form_overflow_flags(cpu_kernel, cases):
    big = next(c[1] for c in cases if c[0] == "overflow_test_map")
    want = R.regions_host(*big, 17)
    _assert_large_fits(cpu_kernel, want, big)
    nr, _, npair, _ = U.counts(want)
    assert cpu_kernel([big], 17, cap_regions=nr - 1, cap_pairs=npair)[1] == [R.OVF_REGIONS]
    assert cpu_kernel([big], 17, cap_regions=nr, cap_pairs=npair - 1)[1] == [R.OVF_PAIRS]
    got, ovf, *_ = cpu_kernel([big], 17, cap_regions=nr, cap_pairs=npair)
    assert ovf == [0] and got[0] == want
    # one class with more regions than a class may have
    rng = np.random.default_rng(6)
    noise = U.with_lines(rng.integers(0, 4, size=(160, 160)), 7)
    assert noise[0].size > cpu_kernel.max_pixels and U.counts(R.regions_host(*noise, 4))[1] > cpu_kernel.max_regions
    assert cpu_kernel([noise], 4)[1] == [R.OVF_REGIONS]
    # a line id beyond the document's boxes
    assert cpu_kernel([big[:3] + (big[3][:3],)], 17)[1] == [R.OVF_LINES]
    # in a group, a flagged large document leaves the other large document's table complete
    got, ovf, *_ = cpu_kernel([noise, big], 17)
    assert ovf == [R.OVF_REGIONS, 0] and got[0] is None and got[1] == want


def test_large_cpu_form_refuses_bad_arguments(cpu_kernel, cases):
    big = next(c[1] for c in cases if c[0] == "overflow_test_map")
    *_, first, last, rc = cpu_kernel([big], 17, short_by=1)                # a workspace share one int too small
    assert rc != 0
    for a0, a1 in zip(first, last):
        assert np.array_equal(a0, a1)                                     # refused before anything was written
    assert cpu_kernel([big], 17, listed=[1])[4] != 0                      # a document outside [0, B)
    assert cpu_kernel([big, big], 17, listed=[0, 0])[4] != 0              # listed twice
    assert cpu_kernel([big], 17, listed=[0])[4] == 0


def test_library_and_header_name_the_large_entry():
    from msau_amd import _lib as L
    assert "msau_kv_regions_large" in L.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    assert "int msau_kv_regions_large(" in header
    lib = L.load()
    assert lib.msau_kv_regions_large is not None and lib.msau_version() == 11
    assert "large_documents" in R.STATS
