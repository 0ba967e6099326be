"""The routing table of msau_conv_pair over a descriptor grid, or the comparison of two such tables.

    python tools/pair_route_table.py [--pkg-root DIR] OUT.npz
    python tools/pair_route_table.py --diff parent.npz branch.npz

For every descriptor of the grid the four query answers, all of which run without a device: `msau_conv_pair_applicable`,
`msau_conv_pair_instance`, `msau_conv_pair_bits_bytes` and `msau_conv_pair_wgrad_slabs`, as `out` [blocks, N, 4] int64.  Only these
entry points and `msau_reload_env` are called, so the same file runs against any revision of the library (--pkg-root: the directory
that holds the `msau_amd` package to import, with its built library).  tests/golden/pair_routes.npz is the table of the commit
before pair_route; tests/test_pair_route_cpu.py holds the built library to it.  The file holds the grid's axes and the answers, not
the descriptors: `grid_rows` rebuilds them.

The grid: both dtypes, C in {8, 16, 24, 32}, B in {1, 2, 16}, ten image sizes, the flag sets of FLAG_SETS (each with and without
MSAU_PAIR_TILES), the ReLU masks as planes or as tensors, the riders' operands present or NULL, `add` the input tensor or another one.
One block of that grid under the default environment and one per switch of SWITCHES: the switches of conv_rows.hip that the routing
reads, which the library reads again after msau_reload_env().  The switches conv_pair.hip reads once per process (MSAU_PAIR_MAXC,
MSAU_PAIR_TW, MSAU_PAIR_MIN_TILES, MSAU_PAIR_COUPLE32, MSAU_PAIR_DCOUPLE32) are NOT in the table: every block has their defaults.

--diff: every row of every block must be equal in all four answers.  Exit status 1 otherwise.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

FIELDS = ("dtype", "C", "B", "H", "W", "set", "tiles", "planes", "riders", "same_add")
SIZES = ((8, 8), (14, 14), (20, 18), (33, 26), (42, 32), (64, 61), (84, 64), (60, 129), (168, 128), (336, 256))
RELU_IN, RELU_MID, MASK_MID, TILES, LRN_BWD, WGRAD1, COUPLE, DCOUPLE = 1, 2, 4, 8, 16, 32, 64, 128          # flags1
RELU_OUT, ADD, ACCUM, MASK_A, POOL = 2, 4, 8, 16, 512                                                         # flags2
FWD1, FWD2, BWD1, BWD2 = RELU_IN | RELU_MID, ADD | RELU_OUT, MASK_MID, MASK_A | ADD
# (flags1, flags2, the coupling conv's pooled output asked for)
FLAG_SETS = ((FWD1, FWD2, 0), (FWD1, FWD2 | POOL, 0), (FWD1 | COUPLE, FWD2, 0), (FWD1 | COUPLE, FWD2, 1), (FWD1 | COUPLE, FWD2 | POOL, 0),
             (BWD1, BWD2, 0), (BWD1 | LRN_BWD, BWD2, 0), (BWD1 | WGRAD1, BWD2, 0), (BWD1 | LRN_BWD | WGRAD1, BWD2, 0), (BWD1 | DCOUPLE, BWD2, 0),
             (BWD1, BWD2 | ACCUM, 0), (0, 0, 0), (FWD1, BWD2, 0))
SWITCHES = ("", "MSAU_ROWS_MIN_TASKS=1", "MSAU_PAIR_ROWS=0", "MSAU_ROWS_MAXC=8", "MSAU_PAIR_WGRAD=0", "MSAU_LRN_BWD16=0", "MSAU_PAIR_COUPLE=0",
            "MSAU_ROWS_SH=10")
# every switch rows_env() reads that can move a pair's route or its task split: unset while a block is evaluated
ROWS_ENV = ("MSAU_PAIR_ROWS", "MSAU_ROWS_SH", "MSAU_ROWS_SH16", "MSAU_ROWS_WAVES", "MSAU_ROWS_MIN_TASKS", "MSAU_ROWS_MAXC", "MSAU_PAIR_WGRAD",
            "MSAU_LRN_BWD16", "MSAU_PAIR_COUPLE")
MANDATORY = ("x", "w1", "b1", "mid", "w2", "b2", "y")
RIDER_OPERANDS = ("pool_y", "pool_idx", "lrn_a", "lrn_da", "wg1_x", "wg1_slabs", "cpl_prev", "cpl_w", "cpl_b", "cpl_y", "dcp_dz", "dcp_w",
                  "dcp_mask", "dcp_dprev")


def grid_rows(flag_sets=FLAG_SETS):
    rows = [(dtype, C, B, H, W, s, tiles, planes, riders, same_add)
            for dtype in (0, 1) for C in (8, 16, 24, 32) for B in (1, 2, 16) for H, W in SIZES for s in range(len(flag_sets))
            for tiles in (0, 1) for planes in (0, 1) for riders in (0, 1) for same_add in (0, 1)]
    return np.asarray(rows, dtype=np.int32)


def descriptor(L, row, keep, flag_sets=FLAG_SETS, d=None):
    """the msau_conv_pair_desc of a grid row (`d`: one to fill again); every operand pointer is an address inside `keep` (no launch reads it)"""
    dtype, C, B, H, W, s, tiles, planes, riders, same_add = row
    f1, f2, cpl_pool = flag_sets[s]
    p = ctypes.addressof(keep)
    if d is None:
        d = L.ConvPairDesc()
        for name in MANDATORY:
            setattr(d, name, p)
        d.lrn_alpha_over_n, d.lrn_beta = 1e-4 / 8, 0.75
    d.B, d.H, d.W, d.C, d.flags1, d.flags2 = B, H, W, C, f1 | (TILES if tiles else 0), f2
    d.add = p if same_add else p + 16
    d.bits_mid = d.bits_a = p if planes else None
    d.mask_mid = d.mask_a = None if planes else p
    for name in RIDER_OPERANDS:
        setattr(d, name, p if riders else None)
    d.cpl_pool_y = d.cpl_pool_idx = p if riders and cpl_pool else None
    d.lrn_k = 1.0 if riders else 0.0
    d.wg1_nslabs = 0
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


def evaluate(L, rows, switches=SWITCHES, flag_sets=FLAG_SETS):
    """out [len(switches), N, 4] int64: applicable, instance, bits bytes, wgrad slabs of every row under every switch"""
    lib = L.load()
    keep = (ctypes.c_char * 64)()
    out = np.zeros((len(switches), len(rows), 4), dtype=np.int64)
    for b in each_block(lib, switches):
        d = None
        for i, row in enumerate(rows.tolist()):
            d, dtype = descriptor(L, row, keep, flag_sets, d)
            r = ctypes.byref(d)
            out[b, i] = (lib.msau_conv_pair_applicable(dtype, r), lib.msau_conv_pair_instance(dtype, r),
                         lib.msau_conv_pair_bits_bytes(dtype, r), lib.msau_conv_pair_wgrad_slabs(dtype, r))
    return out


def diff(pa, pb):
    A, B = np.load(pa), np.load(pb)
    if any(not np.array_equal(A[k], B[k]) for k in ("flag_sets", "switches", "sizes")):
        print("the two tables are over different grids")
        return 1
    rows, oa, ob = grid_rows(A["flag_sets"].tolist()).tolist(), A["out"], B["out"]
    bad = np.argwhere((oa != ob).any(axis=2))
    for b, i in bad[:40]:
        print(str(A["switches"][b]) or "default", dict(zip(FIELDS, rows[i])), oa[b, i].tolist(), "against", ob[b, i].tolist())
    print(f"{oa.shape[0]} blocks of {oa.shape[1]} descriptors compared, {len(bad)} differences")
    return 1 if len(bad) else 0


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
    rows = grid_rows()
    np.savez_compressed(args.out, flag_sets=np.asarray(FLAG_SETS, dtype=np.int32), switches=np.asarray(SWITCHES),
                        sizes=np.asarray(SIZES, dtype=np.int32), out=evaluate(L, rows))
    print(f"{len(SWITCHES)} blocks of {len(rows)} descriptors -> {args.out}")


if __name__ == "__main__":
    main()
