"""Training tables for the key-value model: the geometry and labels of `DataGenerator._generate_masks_from_label`
(data_generator/data_generator_text.py:160-250) without the painting, and the painter of a training batch on the device
(csrc/paint.hip, `msau_kv_paint_train`).

A document crosses the bus as its table -- the line and glyph records of msau_amd/inference/glyphs.py plus 8 bytes of labels per
line -- and one launch paints the three canvases that `TrainEngine.step_unet` reads:

    label record  int32 [2] = (label, aux_label)    label = value + 1 if value > 0 else 0            (the last stage's field map)
                                                    aux_label = value + 1 if type == 1 else (1 if type == 2 else 0)   (key / type map)

The random text scale, the aspect jitter, the random pad and the OCR errors are drawn on the host from a `random.Random`, with the
generator's expressions in the generator's order, so a table under `random.Random(s)` is the generator's batch under
`random.seed(s)`.  `paint_train_host` is the statement of what the kernel computes (a gather), `paint_train_painter` the plain
loop of the generator: the fallback for a document whose table is not `ok` (STATS counts them) and what the gather is tested
against.  The generator's affine and rotation warps are a table's optional `warp` (msau_amd/training/kv_warp.py): `KVTrainBatches`
draws them when `kwargs_dat` asks for them and `TrainEngine.step_kv` resamples the painted canvases on the device
(csrc/warp.hip, `msau_kv_warp_train`).  The generator's elastic warp is a `kv_warp.Elastic` in the same slot, drawn
when `KVTrainBatches(..., imresize="pillow")` names the restatement of its removed resize, and resampled by `msau_kv_elastic_train`."""
from __future__ import annotations

import json
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from ..inference import glyphs as G
from .kv_warp import ELASTIC_GRID, Elastic, Warp, affine_warp, elastic_field, mod90_angle, rotate_warp

LABEL_INTS = 2

# what the device painter was given (tools/kv_train_loop.py reads and resets these)
# "host_warped": documents of a warped group that the warp kernel flagged and `kv_warp.warp_host` warped instead
STATS = {"calls": 0, "documents": 0, "host_painted": 0, "h2d_bytes": 0, "host_warped": 0}


@dataclass
class TrainTable:
    shape: Tuple[int, int]              # (h, w) of the document's grid
    scale: float                        # text scale / median line height, before the aspect jitter
    v_scale: float
    h_scale: float
    pad: float                          # page units around the text (an int when jittered, the float 3 * median otherwise)
    lines: list                         # the document's lines, boxes rewritten to grid coordinates
    tokens: np.ndarray                  # int64 [n_glyphs]: the token of every character in text order, OCR errors applied
    label_rec: np.ndarray               # int32 [n_lines, 2] = (label, aux_label)
    line_rec: Optional[np.ndarray]      # int32 [n_lines, 8] as glyphs.GlyphTable; None when the table cannot represent the document
    glyph_rec: Optional[np.ndarray]     # int16 [n_glyphs, 4]
    reason: str = ""                    # why not, when it cannot
    warp: Optional[Union[Warp, Elastic]] = None     # the generator's affine, rotation or elastic augmentation of the painted document, if any

    @property
    def ok(self) -> bool:
        return self.line_rec is not None

    def glyph_table(self) -> G.GlyphTable:
        """the inference view of the table: what `glyphs.paint_host` takes"""
        return G.GlyphTable(self.shape, self.scale, int(self.pad), (), self.lines, self.line_rec, self.glyph_rec, self.reason)


def train_table(doc_or_path, tok_to_id: dict, blank_idx: int, n_token: int, n_class: int, scale_min: float = 3.0,
                scale_max: float = 3.0, text_err: float = 0.0, rng: Optional[random.Random] = None) -> TrainTable:
    """The layout + OCR JSON of a document (its path, or the loaded dict, which is left as it is) -> its training table.

    `rng` (a `random.Random`; None: a fresh one) is drawn from exactly as the generator draws from the module `random`: with
    scale_min != scale_max the vertical and the horizontal jitter and the pad; always the scale (also when the two bounds are
    equal); per character of a line with text one `random()` for the OCR error -- at text_err 0 too -- and on a hit one
    `choice(range(n_token))`.  The generator then looks that INTEGER up in its dictionary of characters, where it never is: a
    replaced character is always `blank_idx`, and so it is here.  Digits are not folded to '0' (the training painter has that
    line commented out).  A label or aux label outside [0, n_class) raises ValueError (the generator's `to_categorical`: IndexError)."""
    rng = random.Random() if rng is None else rng
    if isinstance(doc_or_path, dict):
        lines = [dict(l) for l in doc_or_path["lines"]]
    else:
        with open(doc_or_path, "r") as fh:
            lines = json.load(fh)["lines"]
    min_x, min_y = min(l["box"][0] for l in lines), min(l["box"][1] for l in lines)
    max_x, max_y = max(l["box"][2] for l in lines), max(l["box"][3] for l in lines)
    median_h = np.median([l["box"][3] - l["box"][1] for l in lines])
    if scale_min != scale_max:
        v_scale = rng.uniform(0.8, 1.2)
        h_scale = rng.uniform(0.8, 1.2)
        pad = int(rng.uniform(median_h, median_h * 5))
    else:
        v_scale = h_scale = 1.0
        pad = median_h * 3
    min_x, min_y, max_x, max_y = min_x - pad, min_y - pad, max_x + pad, max_y + pad
    scale = rng.uniform(scale_min, scale_max) / median_h
    w, h = max_x - min_x, max_y - min_y
    shape = (int(h * scale * v_scale), int(w * scale * h_scale))
    L = len(lines)
    # int((c - min) * scale * h_scale) for every box at once: the same float64 products in the same order, truncated the same way
    page = np.array([l["box"] for l in lines], dtype=np.float64).reshape(L, 4)
    jitter = np.array([h_scale, v_scale, h_scale, v_scale], dtype=np.float64)
    boxes = ((page - np.array([min_x, min_y, min_x, min_y], dtype=np.float64)) * scale * jitter).astype(np.int64)
    label_rec = np.zeros((L, LABEL_INTS), dtype=np.int32)
    toks: List[int] = []
    for li, (line, box) in enumerate(zip(lines, boxes.tolist())):
        text, type_idx, value_idx = line["text"], line["type"], line["value"]
        line["box"] = box
        if len(text) == 0:
            continue
        label_rec[li, 0] = value_idx + 1 if value_idx > 0 else 0
        label_rec[li, 1] = value_idx + 1 if type_idx == 1 else (1 if type_idx == 2 else 0)
        err = 2 * text_err if type_idx == 2 else text_err
        for ch in text:
            if rng.random() < err:
                rng.choice(range(n_token))
                toks.append(blank_idx)
            else:
                toks.append(tok_to_id.get(ch, blank_idx))
    bad = (label_rec < 0) | (label_rec >= n_class)
    if bad.any():
        li = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"line {li}: label {label_rec[li].tolist()} is outside the n_class = {n_class} classes")
    tokens = np.array(toks, dtype=np.int64)
    count = np.array([len(l["text"]) for l in lines], dtype=np.int64)
    line_rec, glyph_rec, why = G.span_records(boxes, count, shape, lambda: tokens)
    return TrainTable(shape, scale, v_scale, h_scale, pad, lines, tokens, label_rec, line_rec, glyph_rec, why)


def paint_train_host(table: TrainTable) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (ids uint16, labels int64, aux int64) [h, w]: what the kernel computes, as the kernel computes it.  The ids are
    `glyphs.paint_host`'s.  labels / aux at a pixel are the record of the last line with text whose box [y1:y2, x1:x2] holds it, 0
    if none: the lines are visited from last to first and a pixel keeps the first answer it gets.  The glyph spans play no part,
    and a later line with label 0 hides an earlier label."""
    if not table.ok:
        raise ValueError(f"the table does not represent the document ({table.reason}): paint it with paint_train_painter")
    h, w = table.shape
    ids = G.paint_host(table.glyph_table())[0]
    labels, aux = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    owned = np.zeros((h, w), dtype=bool)
    for li in range(len(table.line_rec) - 1, -1, -1):
        x1, y1, x2, y2, _g0, n = (int(v) for v in table.line_rec[li, :6])
        if n == 0:
            continue
        box = (slice(min(y1, h), min(y2, h)), slice(min(x1, w), min(x2, w)))
        free = ~owned[box]
        labels[box] = np.where(free, int(table.label_rec[li, 0]), labels[box])
        aux[box] = np.where(free, int(table.label_rec[li, 1]), aux[box])
        owned[box] = True
    return ids, labels, aux


def paint_train_painter(table: TrainTable) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (ids, labels, aux) uint16 [h, w] by the generator's plain loop (data_generator_text.py:208-244) over the table's grid
    boxes, tokens and labels: every line paints over what is there.  Needs no records, so it also paints a document whose
    table is not `ok`."""
    ids, labels, aux = (np.zeros(list(table.shape), dtype="uint16") for _ in range(3))
    g = 0
    for li, line in enumerate(table.lines):
        x1, y1, x2, y2 = line["box"]
        text = line["text"]
        if len(text) > 0:
            labels[y1:y2, x1:x2] = table.label_rec[li, 0]
            aux[y1:y2, x1:x2] = table.label_rec[li, 1]
            char_full_w = max(1.0 * (x2 - x1) / len(text), 1.0)
            char_w = max(0.9 * char_full_w, 1.0)
            char_w = min(char_w, int((y2 - y1) * 1.2))
            for idx in range(len(text)):
                offset = x1 + idx * char_full_w
                ids[y1:y2, int(offset):int(offset + char_w)] = table.tokens[g + idx]
            g += len(text)
    return ids, labels, aux


def pack_train_tables(tables: Sequence[TrainTable], round_to: int = 16):
    """The tables of a group of documents as ONE upload, as `glyphs.pack_tables`.  -> (records, offsets, sizes, canvas): records
    int32 [n] = line offsets [B + 1] | glyph offsets [B + 1] | sizes [B][2] | line records | label records | glyph records.  A
    table that does not represent its document takes part as a document without lines (`paint_train_device` paints it on the host)."""
    records, off, sizes, canvas = G.pack_tables([t if t.ok else _no_lines(t) for t in tables], round_to=round_to)
    n_lines = (off["glyphs"] - off["lines"]) // G.LINE_INTS
    labs = [t.label_rec.reshape(-1) for t in tables if t.ok and len(t.label_rec)]
    labs = np.concatenate(labs) if labs else np.zeros(0, dtype=np.int32)
    assert len(labs) == LABEL_INTS * n_lines
    offsets = dict(off, labels=off["glyphs"], glyphs=off["glyphs"] + LABEL_INTS * n_lines)      # still an even number of int32
    return np.concatenate([records[:off["glyphs"]], labs, records[off["glyphs"]:]]), offsets, sizes, canvas


def _no_lines(t: TrainTable) -> G.GlyphTable:
    return G.GlyphTable(t.shape, t.scale, 0, (), t.lines, None, None, t.reason)


def paint_train_device(tables: Sequence[TrainTable], round_to: int = 16, device=None):
    """-> (ids int32, labels int64, aux int64) [B, H, W] on the device and sizes (CPU int64 [B, 2]): one upload of the packed
    tables, one launch of `msau_kv_paint_train` on the current stream.  Inside a document the ids are 0 for the background;
    outside every document ids and both label canvases are -1.  Nothing is cleared first and nothing comes back.  A document whose
    table is not `ok` is painted by `paint_train_painter` and uploaded into its slice (STATS["host_painted"])."""
    import torch
    from .. import _lib as L
    if not torch.cuda.is_available():
        raise RuntimeError("paint_train_device paints through libmsau_hip.so on an MI355X; no GPU is visible (paint_train_host is "
                           "the statement it is tested against, not a fallback)")
    records, off, sizes, (H, W) = pack_train_tables(tables, round_to=round_to)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    B = len(tables)
    rec_d = torch.from_numpy(records).to(dev)
    ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    aux = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    base = rec_d.data_ptr()
    L.call("msau_kv_paint_train", torch.cuda.current_stream(dev).cuda_stream, base + 4 * off["lines"], base + 4 * off["glyphs"],
           base + 4 * off["labels"], base + 4 * off["line_off"], base + 4 * off["glyph_off"], base + 4 * off["sizes"], B, H, W,
           ids.data_ptr(), labels.data_ptr(), aux.data_ptr())
    STATS["calls"] += 1
    STATS["documents"] += B
    STATS["h2d_bytes"] += records.nbytes
    for b, t in enumerate(tables):
        if not t.ok:
            h, w = t.shape
            for dst, src, dt in zip((ids, labels, aux), paint_train_painter(t), (np.int32, np.int64, np.int64)):
                dst[b, :h, :w].copy_(torch.from_numpy(src.astype(dt)))
            STATS["host_painted"] += 1
            STATS["h2d_bytes"] += 20 * h * w
    return ids, labels, aux, torch.from_numpy(sizes)


def canvases_host(tables: Sequence[TrainTable], round_to: int = 16):
    """what `paint_train_device` leaves on the device, built on the host: (ids int32, labels int64, aux int64) [B, H, W] numpy and
    sizes int64 [B, 2] -- `paint_train_host` (the painter for a table that is not `ok`) inside every document, -1 outside"""
    sizes = np.array([t.shape for t in tables], dtype=np.int64).reshape(len(tables), 2)
    H, W = (int(-(-int(sizes[:, d].max()) // round_to) * round_to) for d in (0, 1))
    ids = np.full((len(tables), H, W), -1, dtype=np.int32)
    labels, aux = np.full(ids.shape, -1, dtype=np.int64), np.full(ids.shape, -1, dtype=np.int64)
    for b, t in enumerate(tables):
        h, w = t.shape
        ids[b, :h, :w], labels[b, :h, :w], aux[b, :h, :w] = paint_train_host(t) if t.ok else paint_train_painter(t)
    return ids, labels, aux, sizes


def load_charset(charset_path: str):
    """-> (tok_to_id, blank_idx, n_token) as the generator builds them: ' ' and '$' in front of the file's characters, '$' the blank"""
    with open(charset_path, "r") as fh:
        charset = " " + "$" + fh.read()
    tok_to_id = {tok: idx for idx, tok in enumerate(charset)}
    return tok_to_id, 1, len(tok_to_id)


class KVTrainBatches:
    """Iterator of table groups (lists of `batch_size` TrainTables) over epochs, without end: the generator's `_fillQueue` without its
    threads.  ONE `random.Random(seed)` gives the order (a shuffle per epoch) and the jitter of every table.  The defaults are the
    generator's `scale_min`, `scale_max` and `text_err_train`.

    `kwargs_dat` takes the generator's augmentation keys: `affine_tr` with `affine_value` (default 0.025), `rotate_tr` and
    `rotateMod90_tr`.  A table then carries a `warp` (kv_warp.py), drawn AFTER the table's own draws: for the affine map one
    `getrandbits(32)` that seeds the `RandomState` of its six draws (the generator's own `RandomState(None)` cannot be seeded), for a
    rotation the generator's `uniform(-20, 20)`.  `rotateMod90_tr` maps that angle as the generator does, which -- as written there
    -- always yields -45 degrees (kv_warp.mod90_angle); the oddity is kept.  With every flag off not one extra draw is taken.
    Refused with NotImplementedError: `affine_tr` together with a rotation (the generator re-interpolates the grey-level planes of the
    first warp, which the id canvases cannot express) and the `*_val` flags (validation is not augmented here).

    `elastic_tr` (with the generator's keys `elastic_val_x` and `elastic_value_y`, both 0.0002 by default; `elastic_val` is the
    validation flag) needs `scipy.misc.imresize`, which no current scipy has.  `imresize="pillow"` names its restatement
    (kv_warp.imresize_bicubic: `bytescale` + Pillow's bicubic resize) and turns the flag on; without it `elastic_tr` is refused with
    NotImplementedError, any other value is a ValueError.  A table then carries a `kv_warp.Elastic`: one `getrandbits(32)` per
    document, after the table's own draws, seeds the `RandomState` of its two fields.  A document under 25 pixels on a side -- on
    which the generator itself fails -- still takes its draw and keeps `warp is None`.  `elastic_tr` together with `affine_tr`,
    `rotate_tr` or `rotateMod90_tr` is refused (the generator re-interpolates grey-level planes there)."""

    def __init__(self, paths: Sequence[str], charset_path: str, n_class: int, batch_size: int, scale_min: float = 2.0,
                 scale_max: float = 4.0, text_err: float = 0.1, shuffle: bool = True, seed: int = 0, kwargs_dat: Optional[dict] = None,
                 imresize: Optional[str] = None):
        if len(paths) == 0 or batch_size < 1:
            raise ValueError("KVTrainBatches: needs at least one document and batch_size >= 1")
        kw = dict(kwargs_dat or {})
        self.affine, self.affine_value = bool(kw.get("affine_tr", False)), float(kw.get("affine_value", 0.025))
        self.rotate, self.rotate_mod90 = bool(kw.get("rotate_tr", False)), bool(kw.get("rotateMod90_tr", False))
        if self.affine and (self.rotate or self.rotate_mod90):
            raise NotImplementedError("KVTrainBatches: affine_tr together with rotate_tr / rotateMod90_tr -- the generator rotates the "
                                      "grey-level planes the affine warp interpolated, which cannot be computed from the id canvases")
        if imresize not in (None, "pillow"):
            raise ValueError(f"KVTrainBatches: imresize = {imresize!r}; the one restatement of scipy.misc.imresize is \"pillow\"")
        self.elastic = bool(kw.get("elastic_tr", False))
        self.elastic_value_x, self.elastic_value_y = float(kw.get("elastic_val_x", 0.0002)), float(kw.get("elastic_value_y", 0.0002))
        if self.elastic and imresize is None:
            raise NotImplementedError("KVTrainBatches: elastic_tr -- the generator's elastic_transform needs scipy.misc.imresize, which "
                                      "no current scipy has; pass imresize=\"pillow\" to take its restatement with Pillow "
                                      "(kv_warp.imresize_bicubic)")
        if self.elastic and (self.affine or self.rotate or self.rotate_mod90):
            raise NotImplementedError("KVTrainBatches: elastic_tr together with affine_tr / rotate_tr / rotateMod90_tr -- the generator "
                                      "re-interpolates the grey-level planes of the first warp, which cannot be computed from the id "
                                      "canvases")
        on = [k for k in ("affine_val", "elastic_val", "rotate_val", "rotateMod90_val") if kw.get(k, False)]
        if on:
            raise NotImplementedError(f"KVTrainBatches: {', '.join(on)} -- validation tables are not augmented")
        self.paths, self.n_class, self.batch_size = list(paths), int(n_class), int(batch_size)
        self.scale_min, self.scale_max, self.text_err, self.shuffle = scale_min, scale_max, text_err, shuffle
        self.tok_to_id, self.blank_idx, self.n_token = load_charset(charset_path)
        self.rng = random.Random(seed)
        self._order: List[str] = []

    def table(self, path, scale_min=None, scale_max=None, text_err=None, rng=None) -> TrainTable:
        return train_table(path, self.tok_to_id, self.blank_idx, self.n_token, self.n_class,
                           self.scale_min if scale_min is None else scale_min, self.scale_max if scale_max is None else scale_max,
                           self.text_err if text_err is None else text_err, self.rng if rng is None else rng)

    def __iter__(self):
        return self

    def __next__(self) -> List[TrainTable]:
        group = []
        while len(group) < self.batch_size:
            if not self._order:
                self._order = list(self.paths)
                if self.shuffle:
                    self.rng.shuffle(self._order)
                self._order.reverse()                     # (popped from the end: the shuffled order, first to last)
            group.append(self._augment(self.table(self._order.pop())))
        return group

    def _augment(self, t: TrainTable) -> TrainTable:
        """the table with the warp `kwargs_dat` asks for, drawn from the iterator's generator; no flag on: the table, no draw"""
        if self.affine:
            t.warp = affine_warp(t.shape, self.affine_value, np.random.RandomState(self.rng.getrandbits(32)))
        elif self.rotate or self.rotate_mod90:
            angle = self.rng.uniform(-20, 20)
            t.warp = rotate_warp(t.shape, mod90_angle(angle) if self.rotate_mod90 else angle)
        elif self.elastic:
            rs = np.random.RandomState(self.rng.getrandbits(32))            # (drawn whatever the size: the stream does not depend on it)
            if min(t.shape) >= ELASTIC_GRID:
                t.warp = elastic_field(t.shape, self.elastic_value_x, self.elastic_value_y, rs)
        return t

    def validation(self, scale: float = 3.0) -> List[List[TrainTable]]:
        """the deterministic tables of all documents in groups of `batch_size` (the last may be smaller): scale_min == scale_max ==
        `scale`, no OCR errors; the iterator's generator is left alone"""
        rng = random.Random(0)
        ts = [self.table(p, scale, scale, 0.0, rng) for p in self.paths]
        return [ts[i:i + self.batch_size] for i in range(0, len(ts), self.batch_size)]
