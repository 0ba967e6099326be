"""Ragged batches: documents of different chargrid sizes in one training step.

The reference trains with batch 1 and one H x W per document (train_chargrid_funsd_msau.py:45-59,
data_generator_funsd_bert.py:216-222).  `pack` places B documents at the origin of one zero canvas and returns their sizes;
`MSAUWrapper.forward(x, sizes)` / `TrainEngine.step(x, labels, sizes)` then compute, for every document, what it would compute
alone ("Ragged batches").  `unpack` crops the canvas outputs back, `batches` groups documents of similar size, `pack_ids` packs character-id masks for
`MSAUWrapper.predict_nhwc(ids=..., sizes=...)`, `pack_masks` the line-id / character-position masks of the region stage,
`pack_boxes` the box lists (and feature tables) of `msau_amd.data.raster` for `TrainEngine.step_boxes(..., sizes=)`: no canvas is built
on the host at all.

    for idx in batches(docs, 16):
        x, labels, sizes = pack([docs[i] for i in idx])
        loss = engine.step(x.cuda(), labels.cuda(), sizes)
"""
from __future__ import annotations

from typing import Iterator, List, Sequence, Tuple

import numpy as np
import torch


def _hw(doc) -> Tuple[int, int]:
    m = doc["mask"]
    return int(m.shape[-2]), int(m.shape[-1])


def pack(docs: Sequence[dict], round_to: int = 16) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`docs`: the {"mask": [1, C, h, w] (or [C, h, w]), "label": [1, h, w] (or [h, w])} items of the FUNSD loader.
    -> (x fp32 [B, C, H, W], labels int64 [B, H, W], sizes int64 CPU [B, 2] of (h, w)), every document at the canvas origin and
    zeros elsewhere.  The canvas is the batch's largest h and w, each rounded up to a multiple of `round_to`, so that few
    distinct canvases (= plans, = captured graphs) occur over an epoch."""
    if len(docs) == 0:
        raise ValueError("pack: no documents")
    if round_to < 1:
        raise ValueError(f"pack: round_to must be >= 1, got {round_to}")
    sizes = torch.tensor([_hw(d) for d in docs], dtype=torch.int64)
    C = int(docs[0]["mask"].shape[-3])
    H = -(-int(sizes[:, 0].max()) // round_to) * round_to
    W = -(-int(sizes[:, 1].max()) // round_to) * round_to
    x = torch.zeros((len(docs), C, H, W), dtype=torch.float32)
    labels = torch.zeros((len(docs), H, W), dtype=torch.int64)
    for b, d in enumerate(docs):
        h, w = int(sizes[b, 0]), int(sizes[b, 1])
        m = d["mask"].reshape(-1, h, w)
        if int(m.shape[0]) != C:
            raise ValueError(f"pack: document {b} has {int(m.shape[0])} channels, document 0 has {C}")
        x[b, :, :h, :w] = m
        labels[b, :h, :w] = d["label"].reshape(h, w).long()
    return x, labels, sizes


def pack_ids(masks: Sequence, round_to: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """`masks`: [h, w] character-id masks (numpy or torch, e.g. KVModel's uint16 `char_ids`).
    -> (ids int32 [B, H, W] with -1 (= empty pixel) outside every document, sizes int64 CPU [B, 2] of (h, w)), the canvas rounded
    as in `pack`.  Feed them to `MSAUWrapper.predict_nhwc(ids=ids.cuda(), sizes=sizes)`."""
    if len(masks) == 0:
        raise ValueError("pack_ids: no documents")
    if round_to < 1:
        raise ValueError(f"pack_ids: round_to must be >= 1, got {round_to}")
    ts = [torch.from_numpy(np.asarray(m).astype(np.int64)) if isinstance(m, np.ndarray) else torch.as_tensor(m) for m in masks]
    for b, t in enumerate(ts):
        if t.dim() != 2 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"pack_ids: mask {b} must be an integer [h, w] array, got {t.dtype} {tuple(t.shape)}")
    sizes = torch.tensor([tuple(t.shape) for t in ts], dtype=torch.int64)
    H = -(-int(sizes[:, 0].max()) // round_to) * round_to
    W = -(-int(sizes[:, 1].max()) // round_to) * round_to
    ids = torch.full((len(ts), H, W), -1, dtype=torch.int32)
    for b, t in enumerate(ts):
        ids[b, :t.shape[0], :t.shape[1]] = t.to(torch.int32)
    return ids, sizes


def pack_boxes(docs: Sequence, round_to: int = 16):
    """`docs`: per document `(feat_boxes [n, 6], label_boxes [m, 6], h, w)` or `(feat_boxes, label_boxes, h, w, feats [n_vec, C])`, as
    `raster.document_boxes` / `raster.document_line_boxes` return them (plus the document's feature table); every document in its
    own coordinates.
    -> (grid_boxes int32 [sum n, 6], label_boxes int32 [sum m, 6], feats fp32 [sum n_vec, C] or None, sizes int64 CPU [B, 2] of
    (h, w), (H, W)): the lists concatenated in document order with the sample column rewritten to the document's place in the batch,
    with feature tables the value column (= row of the table) offset by the rows of the documents before and the tables stacked; the
    canvas rounded as in `pack`.  Boxes are NOT clipped here: `TrainEngine.step_boxes(grid_boxes, label_boxes, B, H, W, feats=feats,
    sizes=sizes)` clips every box to its own document on the device, as the reference's painter does on the document's own array."""
    if len(docs) == 0:
        raise ValueError("pack_boxes: no documents")
    if round_to < 1:
        raise ValueError(f"pack_boxes: round_to must be >= 1, got {round_to}")
    with_feats = [len(d) >= 5 and d[4] is not None for d in docs]
    if any(with_feats) and not all(with_feats):
        raise ValueError("pack_boxes: either every document brings a feature table or none does")
    gbs, lbs, tabs, sizes = [], [], [], []
    base, C = 0, None
    for b, d in enumerate(docs):
        if len(d) not in (4, 5):
            raise ValueError(f"pack_boxes: document {b} must be (feat_boxes, label_boxes, h, w[, feats]), got {len(d)} items")
        h, w = int(d[2]), int(d[3])
        if h < 1 or w < 1:
            raise ValueError(f"pack_boxes: document {b} has size ({h}, {w})")
        lists = []
        for nm, bx in (("feature", d[0]), ("label", d[1])):
            a = np.asarray(bx)
            if a.size and (a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 6):
                raise ValueError(f"pack_boxes: the {nm} boxes of document {b} must be an integer [n, 6] array, got {a.dtype} {a.shape}")
            a = a.astype(np.int32).reshape(-1, 6).copy()
            a[:, 0] = b
            lists.append(a)
        gb, lb = lists
        if with_feats[b]:
            t = np.ascontiguousarray(np.asarray(d[4]), dtype=np.float32)
            if t.ndim != 2:
                raise ValueError(f"pack_boxes: the feature table of document {b} must be [n_vec, C], got {t.shape}")
            if C is None:
                C = int(t.shape[1])
            elif int(t.shape[1]) != C:
                raise ValueError(f"pack_boxes: document {b} has {int(t.shape[1])} channels, document 0 has {C}")
            if len(gb) and int(gb[:, 5].max()) >= len(t):
                raise ValueError(f"pack_boxes: a box of document {b} names feature row {int(gb[:, 5].max())}, its table has {len(t)}")
            gb[:, 5] = np.where(gb[:, 5] >= 0, gb[:, 5] + base, gb[:, 5])
            base += len(t)
            tabs.append(t)
        gbs.append(gb)
        lbs.append(lb)
        sizes.append((h, w))
    sizes = torch.tensor(sizes, dtype=torch.int64)
    H = -(-int(sizes[:, 0].max()) // round_to) * round_to
    W = -(-int(sizes[:, 1].max()) // round_to) * round_to
    feats = np.concatenate(tabs, axis=0) if tabs else None
    return np.concatenate(gbs, axis=0), np.concatenate(lbs, axis=0), feats, sizes, (H, W)


def pack_masks(masks: Sequence, round_to: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """`masks`: [h, w] uint16 masks (KVModel's `line_ids` / `char_pos`), the documents in the order given to `pack_ids`.
    -> (int16 [B, H, W] holding the uint16 bits, zero outside every document; sizes int64 CPU [B, 2]) on the canvas of `pack_ids`,
    for the region stage behind the forward (`MSAUWrapper.predict_regions`)."""
    if len(masks) == 0:
        raise ValueError("pack_masks: no documents")
    if round_to < 1:
        raise ValueError(f"pack_masks: round_to must be >= 1, got {round_to}")
    arrs = [np.asarray(m) for m in masks]
    for b, a in enumerate(arrs):
        if a.ndim != 2 or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 65535)):
            raise ValueError(f"pack_masks: mask {b} must be an integer [h, w] array of values in [0, 65535], got {a.dtype} {a.shape}")
    sizes = torch.tensor([a.shape for a in arrs], dtype=torch.int64)
    H = -(-int(sizes[:, 0].max()) // round_to) * round_to
    W = -(-int(sizes[:, 1].max()) // round_to) * round_to
    canvas = np.zeros((len(arrs), H, W), dtype=np.uint16)
    for b, a in enumerate(arrs):
        canvas[b, :a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(canvas.view(np.int16)), sizes


def unpack(t: torch.Tensor, sizes: torch.Tensor) -> List[torch.Tensor]:
    """crop a canvas tensor [B, ..., H, W] back to the per-document tensors [..., h_b, w_b] (views)"""
    sizes = torch.as_tensor(sizes)
    if tuple(sizes.shape) != (int(t.shape[0]), 2):
        raise ValueError(f"unpack: sizes must have shape ({int(t.shape[0])}, 2), got {tuple(sizes.shape)}")
    H, W = int(t.shape[-2]), int(t.shape[-1])
    out = []
    for b in range(int(t.shape[0])):
        h, w = int(sizes[b, 0]), int(sizes[b, 1])
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"unpack: size ({h}, {w}) of sample {b} is outside the {H} x {W} canvas")
        out.append(t[b, ..., :h, :w])
    return out


def batches(docs: Sequence[dict], batch_size: int, round_to: int = 16) -> Iterator[List[int]]:
    """Indices of `docs` in groups of at most `batch_size`, documents of similar size together (sorted by area, then by the
    rounded canvas they need) to limit the padding a canvas adds.  Every index appears exactly once."""
    if batch_size < 1:
        raise ValueError(f"batches: batch_size must be >= 1, got {batch_size}")

    def key(i):
        h, w = _hw(docs[i])
        return (-(-h // round_to), -(-w // round_to), h * w)

    order = sorted(range(len(docs)), key=lambda i: (_hw(docs[i])[0] * _hw(docs[i])[1], key(i)))
    for k in range(0, len(order), batch_size):
        yield order[k:k + batch_size]


def padded_fraction(sizes: torch.Tensor, H: int, W: int) -> float:
    """share of the canvas pixels that belong to no document"""
    sizes = torch.as_tensor(sizes)
    used = int((sizes[:, 0] * sizes[:, 1]).sum())
    return 1.0 - used / float(int(sizes.shape[0]) * H * W)
