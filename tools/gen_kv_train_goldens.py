#!/usr/bin/env python
"""Golden batches of the reference's text data generator for tests/test_kv_train_*.py -> tests/golden/kv_train/kv_train.npz.

Runs `DataGenerator._generate_masks_from_label` of the reference project (MSAU_REFERENCE: its checkout; cv2 is only used by its
drawing code and is stubbed) on the three golden layouts under `random.seed(seed)`, for five settings of the scale range and
the text error, and stores per case the argmax of the three one-hot maps it returns (int16: ids, labels, aux labels) and the next
`random.random()` after the call, which pins how many draws it consumed.  Only this data file is committed.

    MSAU_REFERENCE=/path/to/reference python tools/gen_kv_train_goldens.py"""
import contextlib
import io
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV = os.path.join(ROOT, "tests", "golden", "kv")
OUT = os.path.join(ROOT, "tests", "golden", "kv_train", "kv_train.npz")
N_CLASS = 17
SETTINGS = [(3.0, 3.0, 0.0, 100), (2.0, 4.0, 0.0, 101), (2.0, 4.0, 0.1, 102), (3.0, 3.0, 0.3, 103), (2.0, 2.5, 0.1, 104)]


def main():
    ref = os.environ.get("MSAU_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("set MSAU_REFERENCE to the reference project's checkout")
    sys.path.insert(0, ref)
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    with contextlib.redirect_stdout(io.StringIO()):
        from data_generator.data_generator_text import DataGenerator
        gen = DataGenerator(None, None, N_CLASS, path_charset=os.path.join(KV, "charset.txt"))
    out = {"settings": np.array(SETTINGS, dtype=np.float64), "n_class": np.array(N_CLASS), "n_token": np.array(gen.n_token)}
    for si, (smin, smax, err, seed) in enumerate(SETTINGS):
        for di in range(3):
            random.seed(seed)
            maps = gen._generate_masks_from_label(os.path.join(KV, f"layout{di}.json"), smin, smax, err)
            out[f"s{si}.d{di}.next"] = np.array(random.random(), dtype=np.float64)
            for name, m in zip(("ids", "labels", "aux"), maps):
                out[f"s{si}.d{di}.{name}"] = np.argmax(m, axis=-1).astype(np.int16)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
