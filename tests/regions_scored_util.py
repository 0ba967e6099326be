"""Inputs shared by tests/test_regions_scored_cpu.py and tests/test_regions_scored_gpu.py: probabilities for the documents of
tests/regions_util.py (a document is (cls, line_mask, char_mask, boxes); its probabilities are fp32 [h, w, n_class])."""
import functools

import numpy as np

from tests import regions_util as U


def doc_probs(rng, cls, n_class):
    """the fp32 softmax of random logits whose first maximum is `cls`: normal logits, the class's own raised above the rest"""
    cls = np.asarray(cls)
    logits = rng.normal(size=cls.shape + (n_class,)).astype(np.float32)
    top = logits.max(-1) + rng.uniform(0.05, 3.0, size=cls.shape).astype(np.float32)
    np.put_along_axis(logits, cls[..., None], top[..., None], -1)
    e = np.exp(logits - logits.max(-1, keepdims=True), dtype=np.float32)
    p = (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    assert np.array_equal(np.argmax(p, -1), cls)
    return p


def pack_probs(probs, canvas_shape, n_class, outside=None, seed=0):
    """the documents' probabilities at the origin of a [B, H, W, n_class] canvas; outside the documents `outside` for every class,
    or random values"""
    B, H, W = canvas_shape
    if outside is None:
        out = np.random.default_rng(seed).random((B, H, W, n_class), dtype=np.float32)
    else:
        out = np.full((B, H, W, n_class), outside, np.float32)
    for b, p in enumerate(probs):
        out[b, :p.shape[0], :p.shape[1]] = p
    return out


def full_doc(h, w):
    """one class (2 of 3) with p = 1.0 everywhere -> (document, probabilities); its one region is h x (w - 2) pixels"""
    pr = np.zeros((h, w, 3), np.float32)
    pr[..., 2] = 1.0
    return U.with_lines(np.full((h, w), 2), 3), pr


def quarter_doc():
    """one region of class 3 (of 4) at p = 0.75 exactly, over one text line -> (document, probabilities, lines)"""
    h, w = 9, 30
    lines = [{"box": [2, 3, 24, 6], "text": "hello world", "type": 0, "value": 0}]
    cls, lm, cm = np.zeros((h, w), int), np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16)
    cls[3:6, 2:24] = 3
    lm[3:6, 2:24] = 1
    for k in range(11):
        cm[3:6, 2 + 2 * k:4 + 2 * k] = k + 1
    pr = np.zeros((h, w, 4), np.float32)
    pr[..., 0] = 1.0
    pr[3:6, 2:24] = (0.25, 0.0, 0.0, 0.75)
    return (cls, lm, cm, [l["box"] for l in lines]), pr, lines


def score_rows(header_doc, n_class):
    """the rows of a document's region list (and score list) that its classes reserved"""
    rows = [np.arange(header_doc[c, 0], header_doc[c, 0] + header_doc[c, 1]) for c in range(2, n_class)]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def scored_cases(max_pixels):
    """[(name, document, n_class, probabilities)]: the shapes of tests/regions_util.py, a blocky map, and a document whose
    probabilities are all ties of the quantisation (odd multiples of 2^-17; there the class map is not their maximum)"""
    rng = np.random.default_rng(50)
    out = [(name, doc, n_class, doc_probs(rng, doc[0], n_class)) for name, doc, n_class in U.shape_cases(max_pixels)]
    blocky = U.with_lines(U.blocky_map(rng, 64, 96, 6, flip=0.05), 51)
    out.append(("blocky", blocky, 6, doc_probs(rng, blocky[0], 6)))
    ties = U.with_lines(np.full((8, 12), 2), 52, n_lines=2)
    pr = np.zeros((8, 12, 3), np.float32)
    pr[..., 2] = (rng.integers(0, 32768, size=(8, 12)) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -17)
    pr[..., 0] = 1 - pr[..., 2]
    out.append(("ties", ties, 3, pr))
    return out
