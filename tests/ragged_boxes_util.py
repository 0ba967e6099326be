"""Shared by tests/test_ragged_boxes_cpu.py and tests/test_ragged_boxes_gpu.py: a numpy restatement of what the device painters do
with a ragged batch of box lists -- every box clipped to its OWN document (h_b, w_b) at the origin of the H x W canvas, boxes applied
in order, the last one wins (data_generator_funsd_bert.py:64-93,149-186: numpy slicing on the document's own h x w array) -- and the
golden FUNSD documents as box lists."""
import json
import os
import pickle

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "funsd")


def owner_ragged(boxes, sizes, H, W):
    """int32 [B, H, W]: index of the last box covering the pixel after clipping to the box's own document, -1 = none"""
    B = len(sizes)
    owner = np.full((B, H, W), -1, np.int32)
    for i, (b, y0, y1, x0, x1, _v) in enumerate(np.asarray(boxes, np.int64).reshape(-1, 6).tolist()):
        if not 0 <= b < B:
            continue
        h, w = int(sizes[b][0]), int(sizes[b][1])
        ya, yb, xa, xb = max(y0, 0), min(y1, h), max(x0, 0), min(x1, w)
        if yb > ya and xb > xa:
            owner[b, ya:yb, xa:xb] = i
    return owner


def labels_ragged(label_boxes, sizes, H, W):
    lb = np.asarray(label_boxes, np.int64).reshape(-1, 6)
    o = owner_ragged(lb, sizes, H, W)
    return np.where(o >= 0, lb[np.maximum(o, 0), 5] if len(lb) else 0, 0).astype(np.int64)


def onehot_ragged(char_boxes, sizes, H, W, C):
    """float32 [B, H, W, C]: one-hot of the owning box's value, zeros where none, where the value is -1 and outside the documents"""
    cb = np.asarray(char_boxes, np.int64).reshape(-1, 6)
    o = owner_ragged(cb, sizes, H, W)
    v = np.where(o >= 0, cb[np.maximum(o, 0), 5] if len(cb) else -1, -1)
    return (v[..., None] == np.arange(C)[None, None, None, :]).astype(np.float32)


def dense_ragged(feat_boxes, feats, sizes, H, W):
    """float32 [B, H, W, C]: the owning box's feature row, zeros elsewhere"""
    fb = np.asarray(feat_boxes, np.int64).reshape(-1, 6)
    o = owner_ragged(fb, sizes, H, W)
    rows = np.concatenate([np.asarray(feats, np.float32), np.zeros((1, feats.shape[1]), np.float32)])
    v = np.where(o >= 0, fb[np.maximum(o, 0), 5] if len(fb) else -1, -1)
    return rows[np.where(v >= 0, v, len(rows) - 1)]


def golden_documents(tmp_path):
    """the committed FUNSD-format documents through the product's loaders ->
    [(dense dataset, chargrid dataset, index)]: `ds[i]` is the document painted alone by the existing CPU painters"""
    from msau_amd.data import funsd as F
    g = np.load(os.path.join(GOLDEN, "bertgrid.npz"), allow_pickle=True)
    labels = json.loads(str(g["labels_json"]))
    train, inv = F.get_preprocessed_list_word_msau(os.path.join(GOLDEN, "train"))
    test, _ = F.get_preprocessed_list_word_msau(os.path.join(GOLDEN, "test"), inv_dict_charset=inv)
    out = []
    for name, docs in (("train", train), ("test", test)):
        docs.sort(key=lambda d: d["file_path"])
        for di, d in enumerate(docs):
            d["transformer_feature"] = g[f"{name}{di}.feats"]
        with open(tmp_path / f"{name}.pkl", "wb") as fh:
            pickle.dump(docs, fh)
        dense = F.FUNSDBertDataLoaderBoxMaskBoxLabel(str(tmp_path / f"{name}.pkl"), labels, write_labels_file=False)
        chars = F.FUNSDCharGridDataLoaderBoxMaskBoxLabel(str(tmp_path / f"{name}.pkl"), labels, write_labels_file=False)
        out += [(dense, chars, i) for i in range(len(dense))]
    return out, len(inv)
