"""The routing table of msau_conv2d over a descriptor grid, or the comparison of two such tables.

    python tools/route_table.py [--pkg-root DIR] OUT.npz
    python tools/route_table.py --diff parent.npz branch.npz

For every descriptor of the grid: `msau_conv2d_launch_info`'s info[0..7] and `msau_conv2d_rider_slabs` (both run without a device).
Written as int32 arrays: the axes of the grid that come from the plans (`triples`, `flat`, `strided`: `grid_rows` rebuilds
the descriptors [N, len(FIELDS)] from them) and `out` [N, 9].  --pkg-root: the directory that holds the `msau_amd` package to
import, with its built library -- the way to compare a change of the dispatch against its parent; tests/golden/routes.npz is the
table of the commit before conv_route, tests/test_route_cpu.py holds the built library to it.

The grid: both dtypes, B in {1, 2, 16}, nine image sizes, the channel triples (C1, C2, Cout) of the forward and data-gradient
descriptors of the five baseline plans (tools/plan_dump.py's GEOM, training, both dtypes) plus (192,0,64), (136,0,8), (768,0,8),
k in {1, 3, 4}, dilation in {1, 2, 4, 8}, stride / ups in {(1,1), (2,1), (1,2)}, and the flag sets (flags, flags2) those plans'
descriptors carry after ConvOp.bind, each also with the flag of every input feed (_feed_nchw / _feed_ids / _feed_owner) where it
has no fused output, plus one set per single flag.  Skipped as invalid: a dilation or a stride / ups with k != 3, both together,
a stride / ups with a second source or with a flag set no transposed conv or its data gradient carries.  --picked keeps the
plans' channel triples listed in PICKED only (the fixture: what fits the size limit of a committed file and a test of a few
seconds; chosen so that every bit of info[7], rider slabs and every group of instances of every family occur, which
tests/test_route_cpu.py asserts).

--diff: rows must be equal, except where only info[6] differs and the first table named a family its own msau_conv2d did not
launch ("conv2d routing"): `allowed_difference`.  Exit status 1 otherwise.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

FIELDS = ("dtype", "B", "Hin", "Win", "Hout", "Wout", "C1", "C2", "Cout", "k", "dil", "pad_t", "pad_l", "stride", "ups", "flags", "flags2")
SIZES = ((8, 8), (20, 18), (33, 26), (56, 32), (64, 32), (128, 112), (128, 128), (336, 256), (512, 384))
EXTRA_TRIPLES = ((192, 0, 64), (136, 0, 8), (768, 0, 8))
# flag -> its bit of info[7] (MSAU_CONV_WGRAD has none: msau_conv2d_rider_slabs answers for it)
HEAD, DOUT, LRN, POOL, IDS, OWNER, NCHW, WGRAD, ELU, EXTENT = 64, 128, 256, 512, 1024, 2048, 4096, 8192, 32768, 65536
INFO7_BIT = {HEAD: 1, DOUT: 2, LRN: 4, POOL: 8, IDS: 16, OWNER: 32, NCHW: 64, EXTENT: 128}
# the fixture's triples: 8 -> 8 (rows, lean, 4x4 + head, LRN, 16 x 32 tile), 8 -> 16 (DOUT, WGRAD rider, dilated LRN, stride 2),
# 8 + 8 -> 8 (rows / lean over concat, POOL), 16 -> 8 and 64 -> 32 (transposed convs; chunked dilation 8), 16 -> 32 and 32 -> 64
# (dilated, DOUT, stride 2), 32 -> 32 and 64 -> 64 (channel split, POOL), 32 + 32 -> 32 (POOL), 64 -> 8 (IDS, NCHW, OWNER)
PICKED = ((8, 0, 8), (8, 0, 16), (8, 8, 8), (16, 0, 8), (16, 0, 32), (32, 0, 32), (32, 32, 32), (32, 0, 64), (64, 0, 8), (64, 0, 32),
          (64, 0, 64))
SINGLES = (1, 2, 4, 8, 16, 32, HEAD, DOUT, LRN, POOL, IDS, OWNER, NCHW, WGRAD, ELU, EXTENT)


def plan_sets(picked):
    """(channel triples, flag sets of stride-1 descriptors, flag sets of transposed convs and their data gradients) of the baseline plans"""
    import torch
    from msau_amd import _lib as L
    from msau_amd.model import param_shapes
    from msau_amd.plan import ConvOp, Plan
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from plan_dump import BASE, GEOM
    triples, flat, strided = set(), set(), set()
    for over, B, H, W in GEOM.values():
        for dt in (L.F32, L.BF16):
            cfg = dict(BASE, **over)
            shapes = param_shapes(cfg)
            poff, off = {}, 0
            for k, s in shapes.items():
                poff[k] = off
                off += -(-int(np.prod(s)) // 4) * 4
            plan = Plan(cfg, B, H, W, dt, torch.device("cpu"), poff, dict(shapes))
            for op in plan.ops:
                if isinstance(op, ConvOp):
                    for d in [op.fdesc] + [dd for dd in op.ddesc if dd is not None]:
                        triples.add((d.C1, d.C2, d.Cout))
                        (flat if d.stride * d.ups == 1 else strided).add((d.flags, d.flags2))
    triples = sorted(triples)
    if picked:
        assert set(PICKED) <= set(triples), sorted(set(PICKED) - set(triples))
        triples = sorted(PICKED)
    fused = HEAD | DOUT | LRN | POOL
    flat |= {(f | feed, 0) for f, _ in list(flat) if not f & fused for feed in (NCHW, IDS, OWNER)}
    flat |= {(f | EXTENT, f2) for f, f2 in list(flat) if not f & (fused | NCHW | IDS)}             # a ragged plan's descriptors
    flat |= {(f, 0) for f in SINGLES} | {(0, 0)}
    strided |= {(f | EXTENT, f2) for f, f2 in list(strided)} | {(0, 0)}
    return triples + [t for t in EXTRA_TRIPLES if t not in triples], sorted(flat), sorted(strided)


def grid_rows(triples, flat, strided):
    rows = []
    for dtype in (0, 1):
        for B in (1, 2, 16):
            for H, W in SIZES:
                for C1, C2, Cout in triples:
                    for k in (1, 3, 4):
                        for dil in (1, 2, 4, 8):
                            for stride, ups in ((1, 1), (2, 1), (1, 2)):
                                if (dil > 1 or stride * ups > 1) and (k != 3 or (dil > 1 and stride * ups > 1)):
                                    continue
                                if stride * ups > 1 and C2:
                                    continue
                                if stride * ups == 1:                       # SAME: the pads of msau_amd.plan.same_pads
                                    Ho, Wo, pt, pl = H, W, (k - 1) * dil // 2, (k - 1) * dil // 2
                                elif ups == 2:                              # transposed conv: (H, W) -> (2H, 2W)
                                    Ho, Wo, pt, pl = 2 * H, 2 * W, 1, 1
                                else:                                       # ... and its data gradient: (H, W) -> (H / 2, W / 2)
                                    Ho, Wo, pt, pl = (H + 1) // 2, (W + 1) // 2, 1, 1
                                for f, f2 in (flat if stride * ups == 1 else strided):
                                    rows.append((dtype, B, H, W, Ho, Wo, C1, C2, Cout, k, dil, pt, pl, stride, ups, f, f2))
    return np.asarray(rows, dtype=np.int32)


def descriptor(L, row, keep, d=None):
    """the msau_conv_desc of a grid row (`d`: one to fill again); every operand pointer is the address of `keep` (no launch reads it)"""
    dtype, B, Hin, Win, Hout, Wout, C1, C2, Cout, k, dil, pad_t, pad_l, stride, ups, flags, flags2 = row
    if d is None:
        d = L.ConvDesc()
        p = ctypes.addressof(keep)
        for name in ("x1", "x2", "wpack", "add", "mask_a", "mask_b", "y", "y2", "mask_b2", "head_probs", "head_argmax", "pool_y",
                     "wg_x1", "wg_slabs", "extent"):
            setattr(d, name, p)
        d.lrn_k, d.lrn_beta, d.lrn_alpha_over_n = 1.0, 0.75, 1e-4
    d.B, d.Hin, d.Win, d.Hout, d.Wout = B, Hin, Win, Hout, Wout
    d.C1, d.C2, d.Cout, d.KH, d.KW, d.dil = C1, C2, Cout, k, k, dil
    d.pad_t, d.pad_l, d.stride, d.ups, d.flags, d.flags2 = pad_t, pad_l, stride, ups, flags, flags2
    d.head_classes = min(Cout, 5)
    return d, dtype


def evaluate(L, desc):
    """out [N, 9]: info[0..7] and msau_conv2d_rider_slabs of every row of `desc` (a row the geometry refuses: -1 throughout)"""
    lib = L.load()
    keep = (ctypes.c_char * 64)()
    info = (L.i32 * 8)()
    out = np.full((len(desc), 9), -1, dtype=np.int32)
    d = None
    for i, row in enumerate(desc.tolist()):
        d, dtype = descriptor(L, row, keep, d)
        if lib.msau_conv2d_launch_info(dtype, ctypes.byref(d), info) == 0:
            out[i, :8] = info[:]
            out[i, 8] = lib.msau_conv2d_rider_slabs(dtype, ctypes.byref(d))
    return out


def refused(flags, info7, slabs):
    """does msau_conv2d refuse a descriptor with these flags, by its own launch_info / rider_slabs?"""
    return any(flags & f and not info7 & bit for f, bit in INFO7_BIT.items()) or bool(flags & WGRAD and slabs <= 0)


def allowed_difference(row, a, b):
    """The one difference a table may show against the table of the commit before conv_route: info[6].  That commit derived it from
    the lean family's applicability query, not from the launch, and so named the lean family (1) for descriptors its msau_conv2d
    refused (a set flag's info[7] bit clear, or no rider slabs) or sent to the box-list / NCHW instance -- now 0."""
    flags = int(row[FIELDS.index("flags")])
    same_but6 = np.array_equal(np.delete(a, 6), np.delete(b, 6))
    return same_but6 and a[6] == 1 and b[6] == 0 and (bool(flags & (OWNER | NCHW)) or refused(flags, int(a[7]), int(a[8])))


def diff(pa, pb):
    A, B = np.load(pa), np.load(pb)
    if any(not np.array_equal(A[k], B[k]) for k in ("triples", "flat", "strided")):
        print("the two tables are over different grids")
        return 1
    desc, oa, ob = grid_rows(A["triples"], A["flat"], A["strided"]).tolist(), A["out"], B["out"]
    bad = allowed = 0
    for i in np.nonzero((oa != ob).any(axis=1))[0]:
        if allowed_difference(desc[i], oa[i], ob[i]):
            allowed += 1
            continue
        bad += 1
        if bad <= 40:
            print(dict(zip(FIELDS, desc[i])), oa[i].tolist(), "against", ob[i].tolist())
    print(f"{len(desc)} descriptors compared, {allowed} info[6] corrections (a family the first table's msau_conv2d did not launch), {bad} differences")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--picked", action="store_true")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(*args.diff))
    sys.path.insert(0, os.path.abspath(args.pkg_root))
    from msau_amd import _lib as L
    triples, flat, strided = (np.asarray(a, dtype=np.int32) for a in plan_sets(args.picked))
    desc = grid_rows(triples.tolist(), flat.tolist(), strided.tolist())
    np.savez_compressed(args.out, triples=triples, flat=flat, strided=strided, out=evaluate(L, desc))
    print(f"{len(desc)} descriptors -> {args.out}")


if __name__ == "__main__":
    main()
