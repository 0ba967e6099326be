"""Inputs shared by tests/test_regions_large_cpu.py and tests/test_regions_large_gpu.py: documents of more pixels than the LDS
form of the region kernel holds (documents as in tests/regions_util.py)."""
import numpy as np

from tests import regions_util as U


def overflow_test_map():
    """the 130 x 192 document of tests/test_regions_cpu.py's overflow test, drawn as it draws it"""
    rng = np.random.default_rng(5)
    rng.integers(0, 17, size=(70, 128))
    return U.with_lines(U.blocky_map(rng, 130, 192, 17), 3)


def runs_map(rng, h, w, n_class, run_len=40):
    """a thin document drawn in runs of `run_len` pixels of one class along its long side, so that a class has about
    long side / run_len / n_class regions (uniformly random pixels give more than a class may have: 1862 on 1 x 30 000)"""
    n = max(h, w)
    line = np.repeat(rng.integers(0, n_class, size=n // run_len + 1), run_len)[:n]
    return np.broadcast_to(line[None, :] if w >= h else line[:, None], (h, w)).copy()


def large_cases():
    """[(name, document, n_class)], every one over the LDS form's pixel limit"""
    out = [("overflow_test_map", overflow_test_map(), 17)]
    rng = np.random.default_rng(21)
    out.append(("257x191", U.with_lines(U.blocky_map(rng, 257, 191, 17, flip=0.01), 22, n_lines=60), 17))
    out.append(("300x256", U.with_lines(U.blocky_map(rng, 300, 256, 5, flip=0.005), 23, n_lines=60), 5))
    out.append(("spiral", U.with_lines(U.spiral(201, 401, 3), 24), 5))
    out.append(("comb", U.with_lines(U.comb(200, 400, 2), 25), 4))
    out.append(("full", U.with_lines(np.full((160, 160), 2), 26), 3))
    out.append(("empty", U.with_lines(np.zeros((160, 160), int), 27), 6))
    for k, (h, w) in enumerate([(1, 30000), (2, 15001), (30000, 1), (10001, 3)]):
        out.append((f"thin_{h}x{w}", U.with_lines(runs_map(rng, h, w, 5), 30 + k, n_lines=6), 5))
    return out
