"""Weight-gradient routing on the CPU: msau_wgrad_route, msau_wgrad_geometry, msau_conv2d_wgrad_groupable and msau_owner_slabs of the
built library against the table of the commit before the families got the _case / _launch contract (tests/golden/wgrad_routes.npz,
written by tools/wgrad_route_table.py), row by row and field by field.  One class of rows may differ: a box-list descriptor
(MSAU_CONV_OWNER) of a shape or with flags the box-list launch has always refused is now refused by the route."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from msau_amd import _lib as L
from tests import wgrad_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("wgrad_route_table", os.path.join(HERE, "..", "tools", "wgrad_route_table.py"))
WT = importlib.util.module_from_spec(spec)
spec.loader.exec_module(WT)

OWNER_TEXT = b"wgrad: MSAU_CONV_OWNER is the 3x3 C -> 8 conv of the net's input, no other flag but EXTENT"


@pytest.fixture(scope="module")
def table():
    axes, want_sweep, want_sub = WT.load(os.path.join(HERE, "golden", "wgrad_routes.npz"))
    sweep, sub = WT.rows_of(axes)
    assert want_sweep.shape == (len(sweep), len(WT.COLS)) and want_sub.shape == (len(axes["switches"]), len(sub), len(WT.COLS))
    assert want_sweep.dtype == np.int64 and axes["switches"][0] == ""
    got_sweep, got_sub = WT.evaluate(L, sweep, sub, axes["switches"], axes["shapes"])
    return axes, sweep, sub, (want_sweep, want_sub), (got_sweep, got_sub)


def _owner_launch_refuses(shape, flags):
    """what msau_conv2d_wgrad has always answered MSAU_ERR_ARG to under MSAU_CONV_OWNER ('same' geometry: the pad is 1 at 3x3)"""
    C1, C2, Cout, k, dil, stride = shape
    return not (Cout == 8 and C2 == 0 and k == 3 and dil == 1 and stride == 1 and not flags & ~(WT.OWNER | WT.EXTENT))


def test_table_reproduced_but_for_the_box_list_refusals(table):
    axes, sweep, sub, (want_sweep, want_sub), (got_sweep, got_sub) = table
    bad = np.argwhere((want_sweep != got_sweep).any(axis=1))
    assert not len(bad), [(dict(zip(WT.SWEEP_FIELDS, sweep[i].tolist())), want_sweep[i].tolist(), got_sweep[i].tolist()) for i, in bad[:5]]
    moved = [WT.ROUTE, WT.FAMILY, WT.SLICES, WT.ERR]
    same = [c for c in range(len(WT.COLS)) if c not in moved]
    listed, n = sub.tolist(), 0
    for b, i in np.argwhere((want_sub != got_sub).any(axis=2)):
        w, g, row = want_sub[b, i], got_sub[b, i], listed[i]
        what = (axes["switches"][b], WT.describe_sub(axes, row), w.tolist(), g.tolist())
        assert row[2] & WT.OWNER and _owner_launch_refuses(axes["shapes"][row[0]], row[2]), what
        assert w[moved].tolist() == [0, U.OWNER, 1, 0] and g[moved].tolist() == [-1, 0, 0, WT.error_hash(OWNER_TEXT)], what
        assert np.array_equal(w[same], g[same]), what                        # the geometry and msau_owner_slabs among them
        n += 1
    print(f"\n{n} box-list rows the route now refuses")
    assert n > 0
    # ... and every box-list row is either such a row or still the box-list family's
    own = np.asarray([bool(r[2] & WT.OWNER) for r in listed])
    refused = np.asarray([_owner_launch_refuses(axes["shapes"][r[0]], r[2]) for r in listed])
    for b in range(len(axes["switches"])):
        assert (got_sub[b][own & refused][:, WT.ROUTE] == -1).all() and (got_sub[b][own & ~refused][:, WT.FAMILY] == U.OWNER).all()


def test_table_covers_the_router(table):
    """under the default environment every family, every instance of WGRAD_TILE_TABLE and every instance of WLEAN_TABLE has a row in
    each type the table lists it for -- in what the built library says"""
    axes, sweep, sub, _, (got_sweep, got_sub) = table
    named, families = set(), set()
    for rows, out, shape_of, dtype_at in ((sweep.tolist(), got_sweep, lambda r: r[:6], 7), (sub.tolist(), got_sub[0], lambda r: axes["shapes"][r[0]], 1)):
        for i in np.nonzero(out[:, WT.FAMILY])[0]:
            (C1, C2, Cout, k, dil, stride), fam, dtype = shape_of(rows[i]), int(out[i, WT.FAMILY]), rows[i][dtype_at]
            families.add(fam)
            if fam == U.GENERIC:
                named.add((dtype, "tile", int(out[i, 2]), int(out[i, 3])))
            elif fam in (U.LEAN, U.SPECIAL, U.IN64, U.IN64_IDS):
                named.add((dtype, "lean", (U.IN64 if fam == U.IN64_IDS else fam, int(out[i, 6]) // 8, Cout // 8, k, dil, stride)))
    assert families == {U.GENERIC, U.LEAN, U.SPECIAL, U.IN64, U.IN64_IDS, U.ROWS, U.OWNER}
    missing = [(dtype, p) for dtype in (L.F32, L.BF16) for p in U.TILE_TABLE[dtype] if (dtype, "tile") + p not in named]
    missing += [(dtype, p) for dtype in (L.F32, L.BF16) for p in U.LEAN_TABLE[dtype] if (dtype, "lean", p) not in named]
    # bf16 64 -> 8 3x3 is the 64 -> 8 kernel's unless the process started with MSAU_WGRAD_IN64=0 (read once: no block can set it)
    assert missing == [(L.BF16, (U.LEAN, 8, 1, 3, 1, 1))], missing
    extra = [k for k in named if k[1] == "tile" and k[2:] not in U.TILE_TABLE[k[0]] or k[1] == "lean" and k[2] not in U.LEAN_TABLE[k[0]]]
    assert not extra, extra


def test_conv2d_wgrad_refuses_a_box_list_descriptor_by_its_shape_then_by_its_context():
    """no device here: both refusals come before any launch.  The shape is the route's to refuse (it reads no pointer), the context
    behind x1 the launch's; a descriptor wrong in both reports the shape"""
    lib, ctx, keep = L.load(), L.OwnerCtx(), (ctypes.c_char * 64)()
    d, dtype = WT.sub_descriptor(L, (0, L.BF16, WT.OWNER, 2, 33, 61, 5), ((64, 0, 8, 3, 1, 1),))
    d.x1, d.g, d.slabs = ctypes.addressof(ctx), ctypes.addressof(keep), ctypes.addressof(keep)
    assert lib.msau_conv2d_wgrad(None, dtype, ctypes.byref(d)) == -1 and lib.msau_last_error().startswith(b"wgrad: bad MSAU_CONV_OWNER context")
    d.flags |= WT.RELU_IN
    assert lib.msau_conv2d_wgrad(None, dtype, ctypes.byref(d)) == -1 and lib.msau_last_error() == OWNER_TEXT


def test_every_switch_moves_a_row(table):
    axes, _, _, (_, want_sub), (_, got_sub) = table
    for out in (want_sub, got_sub):
        for b in range(1, len(axes["switches"])):
            assert (out[b] != out[0]).any(), axes["switches"][b]
