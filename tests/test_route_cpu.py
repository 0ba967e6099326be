"""conv2d routing on the CPU: msau_conv2d_launch_info / msau_conv2d_rider_slabs of the built library against the routing table of the
commit before conv_route (tests/golden/routes.npz, written by tools/route_table.py), and the refusals of msau_conv2d itself."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from msau_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("route_table", os.path.join(HERE, "..", "tools", "route_table.py"))
RT = importlib.util.module_from_spec(spec)
spec.loader.exec_module(RT)


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(HERE, "golden", "routes.npz"))
    assert all(z[k].dtype == np.int32 for k in z.files)
    desc, want = RT.grid_rows(z["triples"].tolist(), z["flat"].tolist(), z["strided"].tolist()), z["out"]
    assert desc.shape[1] == len(RT.FIELDS) and want.shape == (len(desc), 9)
    return desc, want, RT.evaluate(L, desc)


def test_table_reproduced(table):
    """every row equal, apart from the documented class ("conv2d routing"): info[6] named the lean family for a descriptor
    the fixture's own msau_conv2d refused or sent to the box-list / NCHW instance"""
    desc, want, got = table
    rows = np.nonzero((want != got).any(axis=1))[0]
    bad = [i for i in rows if not RT.allowed_difference(desc[i], want[i], got[i])]
    assert not bad, [(dict(zip(RT.FIELDS, desc[i].tolist())), want[i].tolist(), got[i].tolist()) for i in bad[:5]]
    assert len(rows) < len(desc) // 4


def test_table_covers_the_router(table):
    """the fixture is a thinned grid: every answer the router can give, and every group of instances of every family, has rows
    in it -- in the fixture and in what the built library says"""
    desc, want, got = table
    col = {n: desc[:, i] for i, n in enumerate(RT.FIELDS)}
    f, bf16 = col["flags"], col["dtype"] == L.BF16
    tiles = col["B"] * (-(-col["Hout"] // 16)) * (-(-col["Wout"] // 16))
    for out in (want, got):
        lean, chunked, rows = (out[:, 6] == n for n in (1, 2, 3))
        groups = {
            "info[7] bit %d" % b: out[:, 7] & (1 << b) != 0 for b in range(8)}
        groups.update({"a set flag accepted, %d" % flag: (f & flag != 0) & (out[:, 7] & bit != 0) for flag, bit in RT.INFO7_BIT.items()})
        groups["rider slabs"] = out[:, 8] > 0
        groups.update({
            "lean 1x1": lean & (col["k"] == 1) & (col["C2"] == 0) & (f & ~63 == 0),
            "lean 3x3": lean & (col["k"] == 3) & (col["dil"] == 1) & (col["stride"] * col["ups"] == 1) & (col["C2"] == 0) & (f & ~63 == 0),
            "lean 3x3 fp32": lean & ~bf16 & (col["k"] == 3),
            "lean over concat": lean & (col["C2"] != 0) & (f & ~63 == 0),
            "lean 4x4": lean & (col["k"] == 4) & (f & ~63 == 0),
            "lean 4x4 head": lean & (f == RT.HEAD),
            "lean dilation 2": lean & (col["dil"] == 2), "lean dilation 4": lean & (col["dil"] == 4), "lean dilation 8": lean & (col["dil"] == 8),
            "lean transposed": lean & (col["ups"] == 2), "lean stride 2": lean & (col["stride"] == 2),
            "lean DOUT 1x1": lean & (f & RT.DOUT != 0) & (col["k"] == 1), "lean DOUT 3x3": lean & (f & RT.DOUT != 0) & (col["k"] == 3),
            "lean split": lean & (out[:, 0] >= 2) & (col["C1"] >= 32) & (col["C2"] == 0) & (col["dil"] == 1) & (tiles < 512) & (f & ~63 == 0),
            "lean split 64 channels": lean & (out[:, 0] == 4) & (col["C1"] == 64) & (col["dil"] == 1) & (tiles < 512),
            "lean LRN": lean & (f & RT.LRN != 0), "lean LRN dilated": lean & (f & RT.LRN != 0) & (col["dil"] > 1),
            "lean POOL over concat": lean & (f & RT.POOL != 0) & (col["C2"] != 0), "lean POOL split": lean & (f & RT.POOL != 0) & (col["C2"] == 0),
            "lean IDS": lean & (f & RT.IDS != 0),
            "chunked 64-channel chunks": chunked & (col["dil"] == 1), "chunked dilation 8": chunked & (col["dil"] == 8),
            "rows 3x3": rows & (col["k"] == 3) & (col["C2"] == 0) & (f == 0) & (col["ups"] == 1), "rows ACCUM": rows & (f == 8),
            "rows LRN": rows & (f == RT.LRN), "rows over concat": rows & (col["C2"] != 0), "rows 4x4": rows & (col["k"] == 4),
            "rows DOUT 3x3": rows & (f & RT.DOUT != 0) & (col["k"] == 3), "rows DOUT 1x1": rows & (f & RT.DOUT != 0) & (col["k"] == 1),
            "rows DOUT + WGRAD": rows & (f & RT.WGRAD != 0),
            "rows transposed 16 -> 8": rows & (col["ups"] == 2) & (col["C1"] == 16),
            "tile": (out[:, 6] == 0) & (f & ~(63 | RT.ELU | RT.EXTENT) == 0)})
        missing = [name for name, sel in groups.items() if not sel.any()]
        assert not missing, missing


def test_extent_runs_on_the_tile_kernel(table):
    desc, _, got = table
    flags = desc[:, RT.FIELDS.index("flags")]
    sel = (flags & RT.EXTENT != 0) & (flags & RT.OWNER == 0) & (got[:, 0] >= 0)
    assert sel.sum() > 1000 and (got[sel, 6] == 0).all()


def test_conv2d_refuses_before_any_launch(table):
    """a set flag whose info[7] bit is clear (MSAU_CONV_WGRAD: no rider slabs): msau_conv2d says which flag, and launches nothing --
    there is no device here, a launch would be a HIP error, not MSAU_ERR_ARG"""
    desc, _, got = table
    lib = L.load()
    flags = desc[:, RT.FIELDS.index("flags")]
    keep = (ctypes.c_char * 64)()
    n, d = 0, None
    rows = desc.tolist()
    for i in np.nonzero(got[:, 0] >= 0)[0]:
        f = int(flags[i])
        if not RT.refused(f, int(got[i, 7]), int(got[i, 8])):
            continue
        d, dtype = RT.descriptor(L, rows[i], keep, d)
        assert lib.msau_conv2d(None, dtype, ctypes.byref(d)) == -1, dict(zip(RT.FIELDS, rows[i]))      # MSAU_ERR_ARG
        m = re.match(r"conv2d: MSAU_CONV_(\w+) is (not implemented for this launch|the )", lib.msau_last_error().decode())
        assert m and f & getattr(RT, m.group(1)), (lib.msau_last_error(), f)
        n += 1
    assert n > 1000
