"""Entity-level predictions by box vote without a GPU: the numpy statement `box_vote_host` against a brute-force loop over pixels,
the kernel of csrc/boxvote.hip built as plain C++ (-DMSAU_BOXVOTE_CPU: the same clipping, classification and summary, lanes one
after another) against `box_vote_host`, the argument checks of the ABI function through that build, and `document_word_boxes` on the
golden FUNSD documents.  Every comparison is integer equality (tests/box_vote_util.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from msau_amd.data import entities as E
from tests import box_vote_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _owner(bx, extent):
    return E.owner_host(bx, U.B, U.H, U.W, extent)


# ---- the numpy statement against the loop over pixels --------------------------------------------------------------------
@pytest.mark.parametrize("Cn,Cs", U.COMBOS)
def test_host_statement_against_brute_force(Cn, Cs):
    bx, tie, big = U.boxes(Cn)
    for kind in U.KINDS:
        x = U.logits(kind, Cn, Cs, "bf16")
        for zero_as, extent, owned in U.settings():
            owner = _owner(bx, extent) if owned else None
            want = U.brute_vote(U.first_max_classes(x, Cn, zero_as), bx, Cn, owner, extent)
            got = E.box_vote_host(x, bx, Cn, zero_as, owner, extent)
            U.assert_same(got, want, f"{kind} C={Cn} zero_as={zero_as} extent={extent is not None} owned={owned}")
            assert (got[3][0] == 0).all() and int(got[3].sum()) <= len(bx)
    many = U.many_boxes(Cn)
    U.assert_same(E.box_vote_host(x, many, Cn), U.brute_vote(U.first_max_classes(x, Cn), many, Cn), "many boxes")


@pytest.mark.parametrize("Cn,Cs", U.COMBOS)
def test_table_holds_what_it_promises(Cn, Cs):
    """the areas on the wave and workgroup edges, the 257 voting pixels under the owner map, and the two kinds of tie"""
    bx, tie, big = U.boxes(Cn)
    areas = [(y1 - y0) * (x1 - x0) for _b, y0, y1, x0, x1 in E.clip_boxes(bx, U.B, U.H, U.W) if y1 > y0 and x1 > x0]
    assert {1, 63, 64, 65, 255, 256, 260, U.H * U.W} <= set(areas)
    x = U.logits("ties", Cn, Cs, "f32")
    pred, votes, hist, _ = E.box_vote_host(x, bx, Cn)
    assert hist[tie, 0] == hist[tie, Cn - 1] == 4 and pred[tie] == 0 and votes[tie].tolist() == [4, 8]
    b, y0, _y1, x0, _x1 = U.TIE_BOX
    assert x[b, y0, x0 + 3, 0] == x[b, y0, x0 + 3, Cn - 1] == 2          # the pixel whose two channels tie went to class 0
    owned = E.box_vote_host(x, bx, Cn, owner=_owner(bx, None))
    assert owned[1][big].tolist()[1] == 257
    assert int(owned[1][:, 1].sum()) == int((_owner(bx, None) >= 0).sum())       # every owned pixel votes for exactly one box
    assert np.isnan(U.logits("nan", Cn, Cs, "bf16")[..., :Cn]).sum() == 2


# ---- the kernel's body as plain C++ ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_kernel(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the host C++ compiler that msau_amd.build uses for its stamp object"
    out = str(tmp_path_factory.mktemp("boxvote_cpu") / "libboxvote_cpu.so")
    subprocess.run([cxx, "-O1", "-g", "-Wall", "-DMSAU_BOXVOTE_CPU", "-shared", "-fPIC", "-x", "c++",
                    os.path.join(ROOT, "msau_amd", "csrc", "boxvote.hip"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.msau_box_vote_cpu.restype = C.c_int
    lib.msau_box_vote_cpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p, C.c_char_p]

    def run(x, dtype, bx, Cn, Cs, zero_as=None, owner=None, extent=None, hist=True, counts=None, count=True):
        """-> (pred, votes, hist or None, counts or None); the outputs sit between guard bands"""
        n = len(bx)
        store = U.to_storage(x, dtype)
        bx = np.ascontiguousarray(bx, np.int32)
        bufs = {"pred": U.guarded((n,)), "votes": U.guarded((n, 2)), "hist": U.guarded((n, Cn))}
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        at = lambda name: C.c_void_p(bufs[name].ctypes.data + 4 * U.GUARD)
        if count and counts is None:
            counts = np.zeros((Cn, Cn), np.int64)
        own = None if owner is None else np.ascontiguousarray(owner, np.int32)
        ext = None if extent is None else np.ascontiguousarray(extent, np.int32)
        msg = C.create_string_buffer(160)
        rc = lib.msau_box_vote_cpu(0 if dtype == "f32" else 1, p(store), p(bx), n, p(own), at("pred"), at("votes"),
                                   at("hist") if hist else None, p(counts) if count else None, U.B, U.H, U.W, Cn, Cs,
                                   -1 if zero_as is None else zero_as, p(ext), msg)
        assert rc == 0, msg.value
        if not hist:
            assert (bufs["hist"] == U.SENTINEL).all()
        return (U.check_guarded(bufs["pred"], (n,), "pred"), U.check_guarded(bufs["votes"], (n, 2), "votes"),
                U.check_guarded(bufs["hist"], (n, Cn), "hist") if hist else None, counts if count else None)

    run.lib = lib
    return run


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("Cn,Cs", U.COMBOS)
def test_cpu_form_of_kernel_on_the_table(cpu_kernel, Cn, Cs, dtype):
    bx, _tie, _big = U.boxes(Cn)
    for kind in U.KINDS:
        x = U.logits(kind, Cn, Cs, dtype)
        for zero_as, extent, owned in U.settings():
            owner = _owner(bx, extent) if owned else None
            want = E.box_vote_host(x, bx, Cn, zero_as, owner, extent)
            got = cpu_kernel(x, dtype, bx, Cn, Cs, zero_as, owner, extent)
            U.assert_same(got, want, f"{kind} {dtype} C={Cn} zero_as={zero_as} extent={extent is not None} owned={owned}")


def test_cpu_form_of_kernel_optional_outputs_many_boxes_and_accumulation(cpu_kernel):
    Cn, Cs = 5, 8
    bx, _tie, _big = U.boxes(Cn)
    x = U.logits("random", Cn, Cs, "bf16")
    want = E.box_vote_host(x, bx, Cn)
    U.assert_same(cpu_kernel(x, "bf16", bx, Cn, Cs, hist=False), want, "hist = NULL")
    U.assert_same(cpu_kernel(x, "bf16", bx, Cn, Cs, count=False), want, "counts = NULL")
    many = U.many_boxes(Cn)
    U.assert_same(cpu_kernel(x, "bf16", many, Cn, Cs), E.box_vote_host(x, many, Cn), "5000 boxes")
    counts = np.zeros((Cn, Cn), np.int64)
    cpu_kernel(x, "bf16", bx, Cn, Cs, counts=counts)
    cpu_kernel(x, "bf16", many, Cn, Cs, zero_as=1, counts=counts)
    assert np.array_equal(counts, want[3] + E.box_vote_host(x, many, Cn, zero_as=1)[3])


def test_argument_checks_of_the_abi_function(cpu_kernel):
    lib = cpu_kernel.lib
    x = np.zeros((U.B, U.H, U.W, 72), np.float32)
    bx = np.zeros((2, 6), np.int32)
    pred, votes = np.full(2, U.SENTINEL, np.int32), np.full((2, 2), U.SENTINEL, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(n=2, Cn=5, Cs=8, zero_as=-1, logits=x, pr=pred, vt=votes, dtype=0):
        msg = C.create_string_buffer(160)
        rc = lib.msau_box_vote_cpu(dtype, p(logits), p(bx), n, None, p(pr), p(vt), None, None, U.B, U.H, U.W, Cn, Cs, zero_as, None, msg)
        return rc, msg.value.decode()

    assert call()[0] == 0 and (pred == -1).all()                       # two empty boxes
    for kw, word in ((dict(Cn=65, Cs=72), "C = 65"), (dict(zero_as=5), "zero_as = 5"), (dict(pr=None), "null"), (dict(vt=None), "null"),
                     (dict(logits=None), "null"), (dict(Cn=9, Cs=8), "C = 9"), (dict(Cs=12), "Cs = 12"), (dict(Cn=0), "C = 0"),
                     (dict(n=-1), "n = -1"), (dict(dtype=2), "dtype")):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and msg.startswith("box_vote: ") and word in msg, (kw, rc, msg)
    pred[:] = U.SENTINEL
    assert call(n=0, pr=None, vt=None, logits=None)[0] == 0            # n = 0: nothing is needed and nothing is touched
    assert call(n=0)[0] == 0 and (pred == U.SENTINEL).all()
    header = open(os.path.join(ROOT, "include", "msau_hip.h")).read()
    assert "int msau_box_vote(" in header
    from msau_amd import _lib
    from msau_amd.build import SOURCES
    assert "msau_box_vote" in _lib.EXPORTED_SYMBOLS and "boxvote.hip" in SOURCES


# ---- word boxes of the golden documents -----------------------------------------------------------------------------------
def test_document_word_boxes_on_golden_documents():
    from msau_amd.data import funsd as F
    from msau_amd.data import raster
    golden = os.path.join(ROOT, "tests", "golden", "funsd")
    train, inv = F.get_preprocessed_list_word_msau(os.path.join(golden, "train"))
    test, _ = F.get_preprocessed_list_word_msau(os.path.join(golden, "test"), inv_dict_charset=inv)
    docs = train + test
    assert len(docs) == 3
    names = sorted({lab for d in docs for lab in d["labels"]})
    for d in docs:
        d = dict(d, labels=np.array([names.index(lab) for lab in d["labels"]]))
        words = d["cells_word"]
        geo = F.chargrid_geometry(words)
        wb = raster.document_word_boxes(d, sample=2)
        assert wb.dtype == np.int32 and wb.shape == (len(words), 6) and (wb[:, 0] == 2).all()
        chars = {}
        for wi, _j, y0, y1, x0, x1 in F.word_char_boxes(words, geo):
            chars.setdefault(wi, []).append((y0, y1, x0, x1))
        assert chars, "the golden documents have text"
        for wi, (_s, y0, y1, x0, x1, v) in enumerate(wb.tolist()):
            assert v == int(d["labels"][d["word_to_textline"][wi]]) + 1
            assert y1 > y0 and x1 > x0
            if wi in chars:
                cover = np.zeros((y1 - y0, x1 - x0), bool)
                for cy0, cy1, cx0, cx1 in chars[wi]:
                    assert y0 <= cy0 and cy1 <= y1 and x0 <= cx0 and cx1 <= x1
                    cover[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0] = True
                assert cover.all(), "the word box lies within the union of its characters' boxes"
            else:
                assert x0 == int((words[wi].x - geo["min_x"]) / geo["min_scale"])
                assert x1 - x0 == max(int(words[wi].w / geo["min_scale"]), 1)
        # the same canvas as the character list the grid is painted from
        assert raster.document_boxes(d)[2:] == (geo["H"], geo["W"])
