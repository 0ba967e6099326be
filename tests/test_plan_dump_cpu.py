"""tools/plan_dump.py --descriptors on the CPU: the dump of a plan's launch descriptors is free of addresses, its diff is exact and
names what differs, and every pointer of a built training plan lies in a live allocation.  Plans: the `small` geometry
(1 x 33 x 26, 13 channels) and `cfg1` (2 x 128 x 128); nothing is launched."""
import copy
import ctypes as C
import importlib.util
import json
import os
import sys

import pytest

from msau_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(HERE, "..", "tools", "plan_dump.py"))
PD = importlib.util.module_from_spec(spec)
spec.loader.exec_module(PD)

NAMES = ("small.f32.train", "small.bf16.train", "cfg1.bf16.train")


@pytest.fixture(scope="module")
def built():
    """name -> two builds of the same plan, both alive"""
    cases = {c[0]: c for c in PD.cases()}
    return {n: (PD.build_plan(cases[n], "cpu"), PD.build_plan(cases[n], "cpu")) for n in NAMES}


@pytest.fixture(scope="module")
def dumps(built):
    return {n: [dict(PD.launch_lists(p), **PD.descriptors(p)) for p in pair] for n, pair in built.items()}


def raw_pointers(plan):
    """every non-null pointer field of every launch record, as the address it holds"""
    types = PD.struct_of_kind(L)
    out = []
    for arr, n, _ in (plan._fwd_seq, plan._bwd_seq):
        for i in range(n):
            T = types[arr[i].kind & 0xff]
            s = T.from_address(arr[i].args)
            out += [getattr(s, f) for f, t in T._fields_ if t is C.c_void_p and getattr(s, f)]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_two_builds_of_a_plan_dump_equal_although_every_address_differs(built, dumps, name):
    a, b = built[name]
    pa, pb = raw_pointers(a), raw_pointers(b)
    assert len(pa) == len(pb) > 100 and not set(pa) & set(pb)
    da, db = dumps[name]
    assert da == db
    assert len(da["fwd_desc"]) == a._fwd_seq[1] > 0 and len(da["bwd_desc"]) == a._bwd_seq[1] > 0
    assert len(da["pack"]) == len(a._pack_entries) > 0 and len(da["unpack"]) == len(a._unpack_entries) == len(da["unpack_stage"]) > 0
    # the kinds of these plans' records, each with its own struct
    assert {r["type"] for r in da["fwd_desc"] + da["bwd_desc"]} >= {"ConvDesc", "WgradDesc", "ConvPairDesc", "ReduceArgs", "CsumArgs"}


@pytest.mark.parametrize("name", NAMES)
def test_every_pointer_of_a_training_plan_lies_in_an_allocation(built, dumps, name):
    """descriptors() raises for a pointer into no live allocation, so the dump existing is the statement; here also that it has
    resolved every pointer there is, and that the placeholder of a rider that was never patched (the value 1) is named"""
    plan = built[name][0]
    d = dumps[name][0]
    resolved = [v for r in d["fwd_desc"] + d["bwd_desc"] for v in r["fields"].values() if isinstance(v, list)]
    assert len(resolved) == len(raw_pointers(plan))
    assert all(len(v) == 2 and v[0] >= 0 and v[1] >= 0 for v in resolved)
    arr, n, _ = plan._bwd_seq
    i = next(i for i in range(n) if arr[i].kind & 0xff == L.OP_WGRAD)
    w = L.WgradDesc.from_address(arr[i].args)
    keep = w.slabs
    w.slabs = 1
    try:
        with pytest.raises(ValueError, match=rf"bwd\[{i}\] WgradDesc\.slabs = 0x1 lies in no live allocation"):
            PD.descriptors(plan)
    finally:
        w.slabs = keep
    assert PD.descriptors(plan) == {k: d[k] for k in PD.DESC_KEYS}


def test_an_unknown_launch_kind_is_an_error_not_a_skip(built):
    plan = built["small.f32.train"][0]
    arr = plan._fwd_seq[0]
    keep = arr[0].kind
    arr[0].kind = 0x7f | L.OP_SIDE
    try:
        with pytest.raises(ValueError, match=r"fwd\[0\]: unknown launch kind 127"):
            PD.descriptors(plan)
    finally:
        arr[0].kind = keep


def test_diff_names_plan_record_and_field_and_exits_1(dumps, tmp_path, capsys, monkeypatch):
    good = {n: dict(d[0], build_s=0.0) for n, d in dumps.items()}
    bad = copy.deepcopy(good)
    name = "cfg1.bf16.train"
    i = next(i for i, r in enumerate(bad[name]["bwd_desc"]) if r["type"] == "ConvDesc" and r["fields"]["mask_b"] is not None)
    was_pad, was_ptr = bad[name]["bwd_desc"][i]["fields"]["pad_t"], list(bad[name]["bwd_desc"][i]["fields"]["mask_b"])
    bad[name]["bwd_desc"][i]["fields"]["pad_t"] = was_pad + 1                  # an integer field
    bad[name]["bwd_desc"][i]["fields"]["mask_b"][1] += 64                       # a pointer's byte offset
    pa, pb = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    json.dump(good, open(pa, "w"))
    json.dump(bad, open(pb, "w"))

    def run(*argv):
        monkeypatch.setattr(sys, "argv", ["plan_dump.py", *argv])
        with pytest.raises(SystemExit) as e:
            PD.main()
        return e.value.code, capsys.readouterr().out.splitlines()

    code, out = run("--diff", pa, pa)
    assert code == 0 and out == ["3 plans compared, 0 differences"]
    code, out = run("--diff", pa, pb)
    assert code == 1
    assert out == [f"{name} bwd_desc[{i}] pad_t: {was_pad} against {was_pad + 1}",
                   f"{name} bwd_desc[{i}] mask_b: {was_ptr} against {[was_ptr[0], was_ptr[1] + 64]}",
                   "3 plans compared, 2 differences"]
    # there is no class of allowed differences: --allow-count does not reach the descriptors
    code, out = run("--diff", pa, pb, "--allow-count", "conv_kernel<bf16,CT1,PT16>")
    assert code == 1 and len(out) == 3
    # a dump without descriptors against one with them is a difference, not a smaller comparison
    json.dump({n: {k: v for k, v in d.items() if k not in PD.DESC_KEYS} for n, d in good.items()}, open(pb, "w"))
    code, out = run("--diff", pa, pb)
    assert code == 1 and out[0] == "cfg1.bf16.train: descriptors in only one of the dumps"
