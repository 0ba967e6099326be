"""conv_pair routing on the CPU: the four queries of msau_conv_pair of the built library against the routing table of the commit
before pair_route (tests/golden/pair_routes.npz, written by tools/pair_route_table.py), and the refusals of msau_conv_pair itself."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from msau_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_route_table", os.path.join(HERE, "..", "tools", "pair_route_table.py"))
PT = importlib.util.module_from_spec(spec)
spec.loader.exec_module(PT)


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(HERE, "golden", "pair_routes.npz"))
    assert np.array_equal(z["sizes"], PT.SIZES) and z["out"].dtype == np.int64
    flag_sets, switches = [tuple(s) for s in z["flag_sets"].tolist()], [str(s) for s in z["switches"]]
    rows = PT.grid_rows(flag_sets)
    assert z["out"].shape == (len(switches), len(rows), 4)
    return rows, flag_sets, switches, z["out"], PT.evaluate(L, rows, switches, flag_sets)


def test_table_reproduced(table):
    """every row of every block equal in all four answers: there is no class of allowed differences"""
    rows, _, switches, want, got = table
    bad = np.argwhere((want != got).any(axis=2))
    assert not len(bad), [(switches[b], dict(zip(PT.FIELDS, rows[i].tolist())), want[b, i].tolist(), got[b, i].tolist()) for b, i in bad[:5]]


def test_table_covers_the_router(table):
    """under the default environment every instance of the row family, every group of tile instances, rider slabs and both layouts
    of the mask planes for one shape have rows -- in the fixture and in what the built library says"""
    rows, flag_sets, switches, want, got = table
    assert switches[0] == "" and list(flag_sets) == list(PT.FLAG_SETS)
    col = {n: rows[:, i] for i, n in enumerate(PT.FIELDS)}
    s, planes, riders, wide = col["set"], col["planes"], col["riders"], col["W"] >= 120
    FWD, POOL, CPL, CPLZ, BWD, LRNB, WG1, LRNB_WG1, DCP = 0, 1, 2, 3, 5, 6, 7, 8, 9          # indices into FLAG_SETS
    for out in (want[0], got[0]):
        assert ((out[:, 0] != 0) == (out[:, 1] != 0)).all() and np.isin(out[:, 1], (0, 1, 2)).all()
        tile, rowk = out[:, 1] == 1, out[:, 1] == 2
        groups = {"rider slabs": out[:, 3] > 0}
        for C in (8, 16):
            here = rowk & (col["dtype"] == L.BF16) & (col["C"] == C)
            fwd = [("forward", FWD), ("COUPLE", CPL), ("COUPLE, pooled z", CPLZ)] + ([("POOL", POOL)] if C == 16 else [])
            bwd = [("backward", BWD), ("LRN_BWD", LRNB)] + ([("WGRAD1", WG1), ("LRN_BWD + WGRAD1", LRNB_WG1)] if C == 8 else [])
            for name, k in fwd:                                  # (a rider is taken only with its operands: riders == 1)
                for p in (0, 1):
                    groups[f"rows C{C} {name} planes {p}"] = here & (s == k) & (planes == p) & ((riders == 1) | (k == FWD))
            for name, k in bwd:
                groups[f"rows C{C} {name}"] = here & (s == k) & (planes == 1) & ((riders == 1) | (k == BWD))
        for dt in (L.F32, L.BF16):
            for C in (8, 16):
                for name, k in (("forward", FWD), ("POOL", POOL), ("backward", BWD)):
                    for p in (0, 1):
                        for w in (0, 1):
                            if not (w and dt == L.F32 and C == 16):         # (no wide fp32 tile at 16 channels: LDS)
                                groups[f"tile dtype {dt} C{C} {name} planes {p} wide {w}"] = \
                                    tile & (col["dtype"] == dt) & (col["C"] == C) & (s == k) & (planes == p) & (wide == w)
        for name, k in (("forward", FWD), ("POOL", POOL), ("backward", BWD), ("COUPLE", CPL), ("COUPLE, pooled z", CPLZ), ("DCOUPLE", DCP)):
            for p in (0, 1):
                groups[f"tile bf16 C32 {name} planes {p}"] = tile & (col["dtype"] == L.BF16) & (col["C"] == 32) & (s == k) & (planes == p) \
                    & ((riders == 1) | (k in (FWD, BWD)))
        missing = [name for name, sel in groups.items() if not sel.any()]
        assert not missing, missing
        # one shape whose planes are ballots for the row family and bytes for the tile family, which MSAU_PAIR_TILES asks for
        shape = (col["dtype"] == L.BF16) & (col["C"] == 8) & (col["B"] == 2) & (col["H"] == 84) & (col["W"] == 64)
        assert set(out[shape & rowk, 2].tolist()) == {2 * 84 * 3 * 32}
        assert set(out[shape & tile & (col["tiles"] == 1), 2].tolist()) == {2 * 84 * 64}


def test_conv_pair_refuses_before_any_launch(table):
    """a descriptor no instance takes: msau_conv_pair says "unsupported shape or flags" and launches nothing -- there is no device
    here, a launch would be a HIP error, not MSAU_ERR_ARG.  (Every mandatory pointer of the grid's descriptors is set.)"""
    rows, flag_sets, switches, _, got = table
    lib = L.load()
    keep = (ctypes.c_char * 64)()
    listed = rows.tolist()
    n = 0
    for b in PT.each_block(lib, switches):
        d = None
        for i in np.nonzero(got[b, :, 1] == 0)[0]:
            d, dtype = PT.descriptor(L, listed[i], keep, flag_sets, d)
            assert lib.msau_conv_pair(None, dtype, ctypes.byref(d)) == -1, (switches[b], dict(zip(PT.FIELDS, listed[i])))      # MSAU_ERR_ARG
            assert lib.msau_last_error().startswith(b"conv_pair: unsupported shape or flags"), lib.msau_last_error()
            n += 1
    assert n > 300000
