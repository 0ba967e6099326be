"""Entity-level predictions by box vote, stated in numpy: what `msau_box_vote` (msau_amd/csrc/boxvote.hip) computes on the
device, written from its definition with slices, `argmax` and `bincount`.  The oracle of the box-vote tests, and the route a user
had before the kernel: export the logits of every batch and loop over the boxes on the host."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def owner_host(boxes, B: int, H: int, W: int, extent=None) -> np.ndarray:
    """the owner map `msau_raster_owner` / `msau_raster_owner_ext` write for a box list: int32 [B,H,W], per pixel the LAST box of
    the list that covers it (boxes clipped to the canvas, or with `extent` [B,2] to their own document), -1 = none"""
    owner = np.full((B, H, W), -1, np.int32)
    for i, (b, y0, y1, x0, x1) in enumerate(clip_boxes(boxes, B, H, W, extent)):
        if y1 > y0 and x1 > x0:
            owner[b, y0:y1, x0:x1] = i
    return owner


def clip_boxes(boxes, B: int, H: int, W: int, extent=None):
    """per box (sample, y0, y1, x0, x1) after the painters' clipping; an empty box comes back with y1 <= y0 or x1 <= x0"""
    out = []
    for b, y0, y1, x0, x1, _v in np.asarray(boxes, np.int64).reshape(-1, 6).tolist():
        if not 0 <= b < B:
            out.append((0, 0, 0, 0, 0))
            continue
        eh, ew = (H, W) if extent is None else (min(max(int(extent[b][0]), 0), H), min(max(int(extent[b][1]), 0), W))
        out.append((b, max(y0, 0), min(y1, eh), max(x0, 0), min(x1, ew)))
    return out


def pixel_classes(logits_nhwc, C: int, zero_as: Optional[int] = None) -> np.ndarray:
    """int64 [B,H,W]: the first maximum of the C stored values of every pixel, a NaN counting as the maximum (np.argmax, as
    torch.argmax); 0 -> zero_as when one is given"""
    cls = np.argmax(np.asarray(logits_nhwc, np.float32)[..., :C], axis=-1)
    if zero_as is not None and zero_as >= 0:
        cls = np.where(cls == 0, zero_as, cls)
    return cls


def box_vote_host(logits_nhwc, boxes, C: int, zero_as: Optional[int] = None, owner=None,
                  extent=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """logits_nhwc float [B,H,W,>=C] (a bf16 buffer converted to fp32: exact), boxes int [n,6] = sample, y0, y1, x0, x1, value,
    owner None or int [B,H,W], extent None or int [B,2] -> (pred int32 [n], votes int32 [n,2], hist int32 [n,C], counts int64 [C,C]).
    hist[i] = votes per class of box i's voting pixels (its clipped rectangle; with `owner`, the pixels of it with owner == i);
    votes[i] = (votes of the winner, voting pixels); pred[i] = the smallest class among the most voted, -1 without a voting pixel;
    counts[value, pred] += 1 for the boxes with 1 <= value < C and pred >= 0."""
    logits_nhwc = np.asarray(logits_nhwc)
    B, H, W = logits_nhwc.shape[:3]
    boxes = np.asarray(boxes, np.int64).reshape(-1, 6)
    n = len(boxes)
    cls = pixel_classes(logits_nhwc, C, zero_as)
    pred, votes = np.full(n, -1, np.int32), np.zeros((n, 2), np.int32)
    hist, counts = np.zeros((n, C), np.int32), np.zeros((C, C), np.int64)
    for i, (b, y0, y1, x0, x1) in enumerate(clip_boxes(boxes, B, H, W, extent)):
        if y1 <= y0 or x1 <= x0:
            continue
        c = cls[b, y0:y1, x0:x1]
        if owner is not None:
            c = c[np.asarray(owner)[b, y0:y1, x0:x1] == i]
        hist[i] = np.bincount(c.reshape(-1), minlength=C)
        total = int(hist[i].sum())
        if total == 0:
            continue
        pred[i] = int(np.argmax(hist[i]))                    # the first of the largest counts = the smallest such class
        votes[i] = (hist[i, pred[i]], total)
        v = int(boxes[i, 5])
        if 1 <= v < C:
            counts[v, pred[i]] += 1
    return pred, votes, hist, counts
