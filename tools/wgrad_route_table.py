"""The routing table of msau_conv2d_wgrad over a descriptor grid, or the comparison of two such tables.

    python tools/wgrad_route_table.py [--pkg-root DIR] OUT.npz
    python tools/wgrad_route_table.py --diff parent.npz branch.npz

For every descriptor of the grid what the host says about it without a device, as the COLS columns of an int64 array: the status and
info[0..8) of `msau_wgrad_route`; the status and every field of `msau_wgrad_geometry`; `msau_conv2d_wgrad_groupable(d, d)` and
`(d, d')`, d' = d with one more slab; `msau_owner_slabs(d)`; and, where the route refuses, the crc32 of `msau_last_error`.  Only these
entry points and `msau_reload_env` are called, so the same file runs against any revision of the library (--pkg-root: the directory
that holds the `msau_amd` package to import, with its built library).  tests/golden/wgrad_routes.npz is the table of the commit
before the weight gradient's families got the _case / _launch contract; tests/test_wgrad_route_cpu.py holds the built library to it.
The file holds the grid's axes and the answers (column by column), not the descriptors: `sweep_rows` and `sub_rows` rebuild them.  No pointer of a
descriptor is set: none of these entry points may read one.

Two grids.  `sweep` [N, COLS], default environment: the sweep of tests/test_wgrad_cpu.py -- CINS x their C1 | C2 splits x COUTS x KS x
DILS x STRIDES x 'same' / 'valid' geometry x both dtypes at B = 2, 33 x 61, no flag, one slab.  `sub` [blocks, M, COLS]: the channel
shapes of SHAPES ('same' geometry) x both dtypes x FLAG_SETS x B in BATCHES x SIZES x nslabs in NSLABS, once under the default
environment and once per switch of SWITCHES: the switches of conv_rows.hip that the routing reads, which the library reads again
after msau_reload_env().  SIZES puts the row family's task count (B x strips of 30 columns x segments of 8 rows) on both sides of
MSAU_ROWS_MIN_TASKS = 16: 33 x 61 is 15 tasks at B = 1 and 30 at B = 2, 18 x 30 at B = 8 exactly 16; 12 x 20 is one tile row, the others
more.  MSAU_WGRAD_IN64 is read once per process: not a block -- write a second table in a process started with MSAU_WGRAD_IN64=0.

--diff: names the block, the descriptor and the field of every difference (the first 40).  Exit status 1 on any.
"""
import argparse
import ctypes
import os
import sys
import zlib

import numpy as np

CINS = list(range(8, 129, 8)) + [192, 768]
COUTS = list(range(8, 137, 8)) + [192, 256]
KS, DILS, STRIDES = (1, 3, 4, 5, 7), (1, 2, 4, 8, 16, 32), (1, 2)
SWEEP_FIELDS = ("C1", "C2", "Cout", "k", "dil", "stride", "valid", "dtype")
SWEEP_B, SWEEP_HW = 2, (33, 61)

RELU_IN, IDS, OWNER, EXTENT = 1, 1024, 2048, 65536
FLAG_SETS = (0, RELU_IN, IDS, OWNER, OWNER | EXTENT, OWNER | RELU_IN)
# (C1, C2, Cout, k, dil, stride): the weight gradients of the plans of tools/plan_dump.py, and four more -- a generic shape, the
# 64 -> 8 kernel at one, two and twelve chunks
SHAPES = ((8, 0, 8, 3, 1, 1), (8, 0, 8, 4, 1, 1), (8, 0, 16, 3, 1, 2), (8, 0, 16, 3, 2, 1), (8, 8, 8, 1, 1, 1), (8, 8, 8, 3, 1, 1),
          (16, 0, 8, 3, 1, 1), (16, 0, 16, 3, 1, 1), (16, 0, 32, 3, 1, 2), (16, 0, 32, 3, 4, 1), (16, 16, 16, 1, 1, 1), (16, 16, 16, 3, 1, 1),
          (32, 0, 8, 3, 1, 1), (32, 0, 32, 3, 1, 1), (32, 0, 64, 3, 1, 2), (32, 0, 64, 3, 8, 1), (32, 32, 32, 1, 1, 1), (32, 32, 32, 3, 1, 1),
          (64, 0, 8, 1, 1, 1), (64, 0, 64, 1, 1, 1), (64, 0, 64, 3, 1, 1), (64, 64, 64, 1, 1, 1),
          (24, 0, 40, 3, 1, 1), (64, 0, 8, 3, 1, 1), (128, 0, 8, 3, 1, 1), (768, 0, 8, 3, 1, 1))
BATCHES, SIZES, NSLABS = (1, 2, 8), ((33, 61), (18, 30), (12, 20)), (1, 5)
SUB_FIELDS = ("shape", "dtype", "flags", "B", "H", "W", "nslabs")
SWITCHES = ("", "MSAU_PAIR_ROWS=0", "MSAU_WGRAD_ROWS=0", "MSAU_WGRAD_ROWS4=1", "MSAU_ROWS_MIN_TASKS=1")
# every switch rows_env() reads that can move a weight gradient's route: unset while a block is evaluated
ROWS_ENV = ("MSAU_PAIR_ROWS", "MSAU_WGRAD_ROWS", "MSAU_WGRAD_ROWS4", "MSAU_ROWS_MIN_TASKS")

COLS = ("route", "family", "CTN", "NKW", "compact", "slices", "cch", "nchunks", "kextc", "geometry", "g.cch", "g.nchunks", "g.kext",
        "g.max_slabs", "g.slab_bytes", "g.lean", "g.reserved", "groupable", "groupable, other nslabs", "owner_slabs", "error text")
ROUTE, FAMILY, SLICES, GEOM, ERR = 0, 1, 5, slice(9, 17), 20
OWNER_SLABS = 19


def sweep_rows(cins=CINS, couts=COUTS, ks=KS, dils=DILS, strides=STRIDES):
    """(Cout innermost, the dtype outermost: most answers do not move with Cout, and the file compresses to a third)"""
    splits = []
    for cin in cins:
        splits.append((cin, 0))
        if cin >= 16:
            splits.append((cin - 8, 8))
            if cin % 16 == 0:
                splits.append((cin // 2, cin // 2))
    rows = [(c1, c2, cout, k, dil, stride, valid, dtype) for dtype in (0, 1) for k in ks for dil in dils for stride in strides
            for valid in ((0, 1) if stride == 1 and k > 1 else (0,)) for c1, c2 in splits for cout in couts]
    return np.asarray(rows, dtype=np.int32)


def sub_rows(shapes=SHAPES, flag_sets=FLAG_SETS, batches=BATCHES, sizes=SIZES, nslabs=NSLABS):
    rows = [(s, dtype, f, B, H, W, n) for s in range(len(shapes)) for dtype in (0, 1) for f in flag_sets for B in batches
            for H, W in sizes for n in nslabs]
    return np.asarray(rows, dtype=np.int32)


def fill(d, C1, C2, Cout, k, dil, stride, valid, B, H, W, flags, nslabs):
    """'same': Hin = Hout with the centred pad (stride 2: Hin = 2 Hout, pad k // 2); 'valid': Hin = Hout + (k - 1) dil, no pad"""
    pad = 0 if valid else (k // 2 if stride == 2 else dil * (k - 1) // 2)
    grow = (k - 1) * dil if valid else 0
    d.B, d.Hout, d.Wout, d.Hin, d.Win = B, H, W, stride * H + grow, stride * W + grow
    d.C1, d.C2, d.Cout, d.KH, d.KW, d.dil, d.pad_t, d.pad_l, d.stride, d.flags, d.nslabs = C1, C2, Cout, k, k, dil, pad, pad, stride, flags, nslabs


def sweep_descriptor(L, row, d=None):
    d = d or L.WgradDesc()
    fill(d, *row[:7], SWEEP_B, *SWEEP_HW, 0, 1)
    return d, row[7]


def sub_descriptor(L, row, shapes=SHAPES, d=None):
    d = d or L.WgradDesc()
    s, dtype, flags, B, H, W, nslabs = row
    fill(d, *shapes[s], 0, B, H, W, flags, nslabs)
    return d, dtype


def each_block(lib, switches=SWITCHES):
    """yields the index of every block while the library runs under that block's switch and no other of ROWS_ENV"""
    saved = {k: os.environ.pop(k) for k in ROWS_ENV if k in os.environ}
    try:
        for b, sw in enumerate(switches):
            name, _, value = str(sw).partition("=")
            if name:
                os.environ[name] = value
            lib.msau_reload_env()
            yield b
            if name:
                del os.environ[name]
    finally:
        for k in ROWS_ENV:
            os.environ.pop(k, None)
        os.environ.update(saved)
        lib.msau_reload_env()


def error_hash(text):
    return zlib.crc32(bytes(text))


class Asker:
    """the answers of one descriptor, in COLS order"""

    def __init__(self, L):
        self.lib, self.info, self.geom, self.other = L.load(), (ctypes.c_int32 * 8)(), L.WgradGeom(), L.WgradDesc()

    def __call__(self, d, dtype):
        lib, r = self.lib, ctypes.byref(d)
        rc = lib.msau_wgrad_route(dtype, r, self.info)
        err = error_hash(lib.msau_last_error()) if rc else 0
        ctypes.memset(ctypes.byref(self.geom), 0, ctypes.sizeof(self.geom))
        grc, g = lib.msau_wgrad_geometry(dtype, r, ctypes.byref(self.geom)), self.geom
        ctypes.memmove(ctypes.byref(self.other), r, ctypes.sizeof(d))
        self.other.nslabs = d.nslabs + 1
        return (rc, *self.info, grc, g.cch, g.nchunks, g.kext, g.max_slabs, g.slab_bytes, g.lean, g.reserved,
                lib.msau_conv2d_wgrad_groupable(dtype, r, r), lib.msau_conv2d_wgrad_groupable(dtype, r, ctypes.byref(self.other)),
                lib.msau_owner_slabs(r), err)


def evaluate(L, sweep, sub, switches=SWITCHES, shapes=SHAPES):
    """(sweep answers [N, COLS], sub answers [len(switches), M, COLS]), int64"""
    ask, lib = Asker(L), L.load()
    out_sweep = np.zeros((len(sweep), len(COLS)), dtype=np.int64)
    out_sub = np.zeros((len(switches), len(sub), len(COLS)), dtype=np.int64)
    d, listed_sweep, listed_sub = L.WgradDesc(), sweep.tolist(), sub.tolist()
    for b in each_block(lib, switches):
        if str(switches[b]) == "":
            for i, row in enumerate(listed_sweep):
                out_sweep[i] = ask(*sweep_descriptor(L, row, d))
        for i, row in enumerate(listed_sub):
            out_sub[b, i] = ask(*sub_descriptor(L, row, shapes, d))
    return out_sweep, out_sub


def load(path):
    z = np.load(path)
    axes = {k: z[k].tolist() for k in ("cins", "couts", "ks", "dils", "strides", "flag_sets", "shapes", "batches", "sizes", "nslabs")}
    axes["switches"] = [str(s) for s in z["switches"]]
    return axes, z["sweep"].T, z["sub"].transpose(0, 2, 1)                 # (stored column by column)


def rows_of(axes):
    return (sweep_rows(axes["cins"], axes["couts"], axes["ks"], axes["dils"], axes["strides"]),
            sub_rows(axes["shapes"], axes["flag_sets"], axes["batches"], axes["sizes"], axes["nslabs"]))


def describe_sub(axes, row):
    return dict(zip(("C1", "C2", "Cout", "k", "dil", "stride"), axes["shapes"][row[0]]), **dict(zip(SUB_FIELDS[1:], row[1:])))


def diff(pa, pb):
    (axes, sa, ua), (axes_b, sb, ub) = load(pa), load(pb)
    if axes != axes_b:
        print("the two tables are over different grids")
        return 1
    sweep, sub = rows_of(axes)
    n = 0
    for i, c in np.argwhere(sa != sb):
        n += 1
        if n <= 40:
            print("sweep", dict(zip(SWEEP_FIELDS, sweep[i].tolist())), COLS[c], int(sa[i, c]), "against", int(sb[i, c]))
    for b, i, c in np.argwhere(ua != ub):
        n += 1
        if n <= 40:
            print(axes["switches"][b] or "default", describe_sub(axes, sub[i].tolist()), COLS[c], int(ua[b, i, c]), "against", int(ub[b, i, c]))
    rows = int((sa != sb).any(axis=1).sum()) + int((ua != ub).any(axis=2).sum())
    print(f"sweep of {len(sa)} descriptors and {ua.shape[0]} blocks of {ua.shape[1]} compared, {n} fields of {rows} rows differ")
    return 1 if n else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(*args.diff))
    sys.path.insert(0, os.path.abspath(args.pkg_root))
    from msau_amd import _lib as L
    sweep, sub = sweep_rows(), sub_rows()
    out_sweep, out_sub = evaluate(L, sweep, sub)
    i32 = dict(dtype=np.int32)
    np.savez_compressed(args.out, cins=np.asarray(CINS, **i32), couts=np.asarray(COUTS, **i32), ks=np.asarray(KS, **i32), dils=np.asarray(DILS, **i32),
                        strides=np.asarray(STRIDES, **i32), flag_sets=np.asarray(FLAG_SETS, **i32), shapes=np.asarray(SHAPES, **i32),
                        batches=np.asarray(BATCHES, **i32), sizes=np.asarray(SIZES, **i32), nslabs=np.asarray(NSLABS, **i32),
                        switches=np.asarray(SWITCHES), sweep=np.ascontiguousarray(out_sweep.T),
                        sub=np.ascontiguousarray(out_sub.transpose(0, 2, 1)))
    print(f"sweep of {len(sweep)} descriptors, {len(SWITCHES)} blocks of {len(sub)} -> {args.out}")


if __name__ == "__main__":
    main()
