"""Shared by tests/test_box_vote_cpu.py and tests/test_box_vote_gpu.py: the case table of `msau_box_vote` (canvas, box list, logits,
the zero_as / extent / owner settings), guarded output buffers, and a brute-force pixel-by-pixel statement of the vote.

Every comparison is integer equality: the device's per-pixel class is the first maximum of the stored values, the oracle
(`msau_amd.data.entities.box_vote_host`) takes the same argmax of the same stored values (a bf16 buffer converted to fp32: exact).

The kernel hands a box of at most 256 clipped pixels to one wave (trips of 64) and a larger one to the workgroup, so the list holds
areas on both edges: 63, 64, 65, 255, 256 and -- because 257, 258 and 259 are no rectangles of a 21 x 35 canvas (257 is prime,
258 = 6 x 43, 259 = 7 x 37) -- 260 = 13 x 20, the smallest box above the switch; a 1 x 3 box painted over it later leaves it exactly
257 voting pixels whenever the owner map is given."""
import itertools

import numpy as np

B, H, W = 3, 21, 35
COMBOS = ((2, 8), (5, 8), (13, 16), (64, 64))
DTYPES = ("f32", "bf16")
EXTENT = np.array([[21, 35], [7, 9], [0, 35]], np.int32)
SENTINEL = -777
GUARD = 64
KINDS = ("random", "ties", "nan")
TIE_BOX = (0, 15, 17, 27, 31)              # sample, y0, y1, x0, x1: the last box of the list, so it owns all its pixels


def boxes(C):
    """the box list of the table -> (int32 [n,6], index of the tie box, index of the 260-pixel box)"""
    bx = [
        (0, 0, H, 0, W, 1),                  # the whole canvas (first: later boxes take its pixels from it in the owner map)
        (1, 0, H, 0, W, 1 % C),              # ... of the sample with the small extent
        (2, 0, H, 0, W, 1 % C),              # ... of the sample with the empty extent
        (1, -3, H + 3, -3, W + 3, 1),        # the whole canvas, from outside
        (0, 3, 4, 5, 6, 1),                  # 1 x 1
        (0, 5, 6, 2, 30, 1),                 # one row
        (1, 1, 19, 33, 34, 1),               # one column
        (0, 0, 7, 0, 9, 1),                  # 63
        (1, 0, 7, 0, 9, 1),                  # 63: sample 1's whole extent
        (0, 8, 16, 0, 8, 1),                 # 64
        (1, 2, 7, 10, 23, 1),                # 65
        (2, 0, 15, 0, 17, 1),                # 255
        (2, 3, 19, 18, 34, 1),               # 256
    ]
    big = len(bx)
    bx += [
        (1, 8, 21, 0, 20, 1),                # 260: the smallest box of this canvas above the wave / workgroup switch
        (1, 9, 10, 4, 7, 1),                 # 1 x 3 inside it: 257 voting pixels are left to it in the owner map
        (0, -4, 3, -2, 6, 1),                # negative starts
        (0, 18, H + 5, 30, W + 9, 1),        # ends beyond H / W
        (0, H, H + 4, 0, 5, 1),              # wholly outside
        (0, 2, 6, -9, 0, 1),
        (0, 9, 4, 3, 8, 1),                  # inverted (y1 <= y0)
        (0, 4, 9, 8, 8, 1),                  # empty (x1 == x0)
        (-1, 0, 5, 0, 5, 1),                 # sample -1
        (B, 0, 5, 0, 5, 1),                  # sample B
        (2, 10, 14, 3, 12, 1),               # two overlapping boxes
        (2, 12, 17, 8, 15, 1),
        (0, 11, 14, 20, 26, 1),              # two identical boxes
        (0, 11, 14, 20, 26, 1),
        (0, 6, 9, 12, 18, 0),                # values that are predicted but not counted: 0, C, C + 3, -1
        (0, 6, 9, 19, 25, C),
        (1, 0, 4, 0, 5, C + 3),
        (2, 0, 3, 30, 35, -1),
    ]
    tie = len(bx)
    bx.append(TIE_BOX + (1,))
    out = np.asarray(bx, np.int32).reshape(-1, 6)
    v = 1 + np.arange(len(out)) % max(C - 1, 1)          # spread the counted values over [1, C) (C = 2: all 1)
    out[:, 5] = np.where(out[:, 5] == 1, v, out[:, 5])
    return out, tie, big


def many_boxes(C):
    """5000 one-pixel boxes: 1250 groups of four, more than the 1024 workgroups the launch is capped at, so the stride loop runs"""
    rng = np.random.default_rng(11)
    n = 5000
    b, y, x = rng.integers(0, B, n), rng.integers(0, H, n), rng.integers(0, W, n)
    return np.stack([b, y, y + 1, x, x + 1, rng.integers(0, C + 1, n)], 1).astype(np.int32)


def stored(x, dtype):
    """float32 values that `dtype` storage holds exactly"""
    if dtype == "bf16":
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000          # round to nearest even; NaNs of the table keep a mantissa bit
        return u.astype(np.uint32).view(np.float32)
    return np.ascontiguousarray(x, np.float32)


def to_storage(x, dtype):
    """the buffer the kernel reads: float32, or the uint16 bit patterns of bf16"""
    x = np.ascontiguousarray(x, np.float32)
    return x if dtype == "f32" else np.ascontiguousarray((x.view(np.uint32) >> 16).astype(np.uint16))


def logits(kind, C, Cs, dtype):
    """float32 [B,H,W,Cs] holding values `dtype` stores exactly.  The padded channels [C, Cs) hold 1000: a kernel that read them
    would predict a class >= C."""
    rng = np.random.default_rng({"random": 1, "ties": 2, "nan": 3}[kind] + 10 * C)
    if kind == "ties":
        x = rng.integers(0, 3, (B, H, W, Cs)).astype(np.float32)        # many pixels whose largest value stands in two channels
        b, y0, y1, x0, x1 = TIE_BOX
        c1 = C - 1                                                      # the tie box: classes 0 and c1 with four votes each
        x[b, y0:y1, x0:x1, :] = 0
        px = [(y, xx) for y in range(y0, y1) for xx in range(x0, x1)]
        for k, (y, xx) in enumerate(px):
            if k < 3:
                x[b, y, xx, 0] = 2
            elif k == 3:
                x[b, y, xx, 0] = x[b, y, xx, c1] = 2                    # both channels tie inside the pixel: the first wins
            else:
                x[b, y, xx, c1] = 2
    else:
        x = rng.standard_normal((B, H, W, Cs)).astype(np.float32)
        if kind == "nan":
            x[0, 12, 22, C - 1] = np.nan                                # inside the two identical boxes
            x[1, 3, 3, 0] = np.nan
    x = stored(x, dtype)
    x[..., C:] = 1000.0
    return x


def settings():
    """(zero_as, extent, owned) of the table"""
    return list(itertools.product((None, 1), (None, EXTENT), (False, True)))


def guarded(shape, dtype=np.int32):
    """a flat buffer for an output of `shape`: the sentinel everywhere, a guard band of GUARD elements on both sides of the payload"""
    return np.full(int(np.prod(shape)) + 2 * GUARD, SENTINEL, dtype)


def check_guarded(buf, shape, name):
    """the band is untouched and every payload element was written -> the payload"""
    size = int(np.prod(shape))
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + size:] == SENTINEL).all(), f"{name}: written outside [0, n)"
    pay = buf[GUARD:GUARD + size].reshape(shape)
    assert (pay != SENTINEL).all(), f"{name}: {int((pay == SENTINEL).sum())} elements not written"
    return pay


def first_max_classes(x, C, zero_as=None):
    """int [B,H,W] by an explicit loop over the channels: strictly greater wins, a NaN counts as the maximum"""
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape[:3], np.int64)
    for idx in np.ndindex(*x.shape[:3]):
        best, bv = 0, -np.inf
        for c in range(C):
            v = x[idx + (c,)]
            if v > bv or (v != v and bv == bv):
                best, bv = c, v
        out[idx] = zero_as if (best == 0 and zero_as is not None and zero_as >= 0) else best
    return out


def brute_vote(classes, bx, C, owner=None, extent=None):
    """the vote pixel by pixel from a class map [B,H,W] -> (pred, votes, hist, counts) as `box_vote_host` returns them"""
    n = len(bx)
    pred, votes = np.full(n, -1, np.int32), np.zeros((n, 2), np.int32)
    hist, counts = np.zeros((n, C), np.int32), np.zeros((C, C), np.int64)
    for i, (b, y0, y1, x0, x1, v) in enumerate(np.asarray(bx).tolist()):
        if b < 0 or b >= B:
            continue
        eh, ew = (H, W) if extent is None else (min(max(int(extent[b][0]), 0), H), min(max(int(extent[b][1]), 0), W))
        for y in range(y0, y1):
            for x in range(x0, x1):
                if y < 0 or y >= eh or x < 0 or x >= ew:
                    continue
                if owner is not None and owner[b, y, x] != i:
                    continue
                hist[i, classes[b, y, x]] += 1
        total = int(hist[i].sum())
        if total == 0:
            continue
        best = 0
        for c in range(C):
            if hist[i, c] > hist[i, best]:
                best = c
        pred[i], votes[i] = best, (hist[i, best], total)
        if 1 <= v < C:
            counts[v, best] += 1
    return pred, votes, hist, counts


def assert_same(got, want, what):
    for name, g, w in zip(("pred", "votes", "hist", "counts"), got, want):
        if g is None:
            continue
        assert np.array_equal(np.asarray(g), np.asarray(w)), f"{what}: {name} differs at {np.argwhere(np.asarray(g) != np.asarray(w))[:5].tolist()}"
