"""Writes tests/golden/kv/elastic_fields.npz: the elastic warp's fields (kv_warp.elastic_field: the generator's coarse random fields,
smoothed, `bytescale`d and resized with Pillow's bicubic filter) of the document shapes that tests/elastic_util.py uses, each from
`RandomState(SEED + index)`.  The fields do not depend on the elastic values, only the alphas do, so one pair per shape is stored;
the GPU tests read the file and need no Pillow, tests/test_kv_elastic_cpu.py regenerates it where Pillow is installed.

    python tools/elastic_fields.py [--check]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msau_amd.training import kv_warp as KW  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kv", "elastic_fields.npz")
SHAPES = [(37, 29), (44, 91), (52, 77)]             # a 1 x 1 grid (a zero field), 1 x 3, 2 x 3
SEED = 20


def fields():
    out = {"shapes": np.array(SHAPES, dtype=np.int64), "seed": np.array(SEED, dtype=np.int64)}
    for k, shape in enumerate(SHAPES):
        el = KW.elastic_field(shape, 0.0002, 0.0002, np.random.RandomState(SEED + k))
        out[f"fy{k}"], out[f"fx{k}"] = el.field_y, el.field_x
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="compare with the file instead of writing it")
    args = ap.parse_args()
    new = fields()
    if args.check:
        old = np.load(OUT)
        bad = [k for k in new if not np.array_equal(old[k], new[k])]
        print("equal" if not bad else f"different: {bad}")
        return 1 if bad else 0
    np.savez_compressed(OUT, **new)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
