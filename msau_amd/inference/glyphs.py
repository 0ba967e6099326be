"""Glyph tables: the geometry of `KVModel._generate_masks_from_label` without the painting, and the painter of the three masks
on the device (csrc/paint.hip).

A document crosses the bus as its table -- 32 bytes per text line, 8 bytes per character -- and one launch paints the
character-id, line-id and character-position canvases where the forward and the region kernel read them:

    line record   int32 [8] = (x1, y1, x2, y2, first glyph, glyphs, xl, xr)   the box in grid coordinates, the line's glyphs (counted
                                                                             from the document's first), the columns [xl, xr) that
                                                                             box and glyphs reach; glyphs = 0: no text, paints nothing
    glyph record  int16 [4] = (a, b, token, 0)                               character k of its line covers columns [a, b); the
                                                                             token is the uint16 character id

The spans are computed here, in float64 with the painter's expressions in the painter's order, for all characters of the document
at once; the device sees integers only.  `paint_host` is the statement of what the kernel computes (a gather: every pixel takes
the last line that covers it), tested against the painter's loop.  A document the table cannot represent (`GlyphTable.ok` False)
is painted by the host painter and its masks are uploaded, as without the table; STATS counts them.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

LINE_INTS = 8
LINE_BYTES, GLYPH_BYTES = 4 * LINE_INTS, 8
COORD_MAX = 32767                       # glyph spans travel as int16
COUNT_MAX = 65535                       # the masks are uint16: line ids and character positions beyond it would wrap

# what the device painter was given (tools/infer_bench.py reads and resets these)
STATS = {"calls": 0, "documents": 0, "host_painted": 0, "h2d_bytes": 0}


@dataclass
class GlyphTable:
    shape: Tuple[int, int]              # (h, w) of the document's grid
    scale: float
    bg_pad: int
    text_bbox: tuple
    lines: list                         # the document's lines, boxes rewritten to grid coordinates
    line_rec: Optional[np.ndarray]      # int32 [n_lines, 8]; None when the table cannot represent the document
    glyph_rec: Optional[np.ndarray]     # int16 [n_glyphs, 4]
    reason: str = ""                    # why not, when it cannot

    @property
    def ok(self) -> bool:
        return self.line_rec is not None


def _tokens(text: str, tok_to_id: dict, blank_idx: int) -> np.ndarray:
    """token of every character of `text`: digits folded to '0', characters outside the charset to `blank_idx`; one dictionary
    look-up per DISTINCT character"""
    cps = np.frombuffer(text.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    uniq, inv = np.unique(cps, return_inverse=True)
    toks = np.empty(len(uniq), dtype=np.int64)
    for i, cp in enumerate(uniq.tolist()):
        ch = chr(cp)
        toks[i] = tok_to_id.get("0" if ch.isdigit() else ch, blank_idx)
    return toks[inv]


def glyph_table(doc_or_path, tok_to_id: dict, blank_idx: int) -> GlyphTable:
    """The layout + OCR JSON of a document (its path, or the loaded dict, which is left as it is) -> its glyph table.  Grid, scale,
    pad, text box and the lines' grid boxes are `_generate_masks_from_label`'s (same expressions, same order)."""
    if isinstance(doc_or_path, dict):
        lines = [dict(l) for l in doc_or_path["lines"]]
    else:
        with open(doc_or_path, "r") as fh:
            lines = json.load(fh)["lines"]
    left, top = min(l["box"][0] for l in lines), min(l["box"][1] for l in lines)
    right, bottom = max(l["box"][2] for l in lines), max(l["box"][3] for l in lines)
    text_bbox = (left, top, right, bottom)
    median_h = np.median([l["box"][3] - l["box"][1] for l in lines])
    bg_pad = int(median_h * 3)
    left, top, right, bottom = left - bg_pad, top - bg_pad, right + bg_pad, bottom + bg_pad
    scale = 3.0 / median_h
    shape = (int((bottom - top) * scale), int((right - left) * scale))
    L = len(lines)
    for line in lines:
        _type, _value = line["type"], line["value"]                     # required keys, as in the painter
    # int((bx - left) * scale) for every box at once: the same float64 products, truncated the same way
    page = np.array([l["box"] for l in lines], dtype=np.float64).reshape(L, 4)
    boxes = ((page - np.array([left, top, left, top], dtype=np.float64)) * scale).astype(np.int64)
    for line, box in zip(lines, boxes.tolist()):
        line["box"] = box
    count = np.array([len(l["text"]) for l in lines], dtype=np.int64)
    text = "".join(l["text"] for l in lines)
    line_rec, glyph_rec, why = span_records(boxes, count, shape, lambda: _tokens(text, tok_to_id, blank_idx))
    return GlyphTable(shape, scale, bg_pad, text_bbox, lines, line_rec, glyph_rec, why)


def span_records(boxes: np.ndarray, count: np.ndarray, shape: Tuple[int, int], tokens):
    """The grid boxes int64 [L, 4] and character counts [L] of a document's lines on a grid of `shape` -> (line_rec, glyph_rec, "") or
    (None, None, why the table cannot represent the document).  `tokens()` gives the token of every character of the document, in
    text order; it is asked only when everything else fits.  (Shared with the training tables, msau_amd/training/kv_data.py.)"""
    L = len(boxes)
    why = ""
    reversed_ = (count > 0) & ((boxes[:, 2] < boxes[:, 0]) | (boxes[:, 3] < boxes[:, 1]))
    if reversed_.any():
        li = int(np.flatnonzero(reversed_)[0])
        why = f"line {li}: reversed box {boxes[li].tolist()}"
    # pitch = max(1.0 * (x2 - x1) / n, 1.0), glyph_w = min(max(0.9 * pitch, 1.0), int((y2 - y1) * 1.2))
    pitch = np.maximum((boxes[:, 2] - boxes[:, 0]).astype(np.float64) / np.maximum(count, 1), 1.0)
    glyph_w = np.minimum(np.maximum(0.9 * pitch, 1.0), ((boxes[:, 3] - boxes[:, 1]) * 1.2).astype(np.int64))
    if not why and (shape[0] < 1 or shape[1] < 1):
        why = f"empty grid {shape}"
    if not why and (L > COUNT_MAX or int(count.max(initial=0)) > COUNT_MAX):
        why = f"{L} lines, {int(count.max(initial=0))} characters in a line: more than {COUNT_MAX}"
    if not why and (boxes.min(initial=0) < 0 or max(int(boxes.max(initial=0)), *shape) > COORD_MAX):
        why = "a coordinate outside [0, %d]" % COORD_MAX
    if why:
        return None, None, why
    # every character of the document at once: its line, its index in the line, its span
    first = np.cumsum(count) - count
    G = int(count.sum())
    of_line = np.repeat(np.arange(L), count)
    k = np.arange(G) - np.repeat(first, count)
    xs = boxes[of_line, 0] + k * pitch[of_line]                         # x1 + k * pitch
    a = xs.astype(np.int64)                                             # int(xs)
    b = (xs + glyph_w[of_line]).astype(np.int64)                        # int(xs + glyph_w)
    if G and (int(a.min()) < 0 or int(b.min()) < 0 or int(b.max()) > COORD_MAX):
        return None, None, "a glyph span outside [0, %d]" % COORD_MAX
    same_line = of_line[1:] == of_line[:-1]
    if G and ((a > b).any() or ((b[:-1] > a[1:]) | (a[:-1] >= a[1:]))[same_line].any()):
        return None, None, "glyph spans of a line are not disjoint with increasing starts"
    tok = np.asarray(tokens(), dtype=np.int64)
    if G and (int(tok.min()) < 0 or int(tok.max()) > COUNT_MAX):
        return None, None, "a token outside uint16"
    line_rec = np.zeros((L, LINE_INTS), dtype=np.int32)
    line_rec[:, :4] = boxes
    line_rec[:, 4], line_rec[:, 5] = first, count
    has = count > 0
    line_rec[has, 6] = np.minimum(boxes[has, 0], a[first[has]])
    line_rec[has, 7] = np.maximum(boxes[has, 2], b[first[has] + count[has] - 1])
    glyph_rec = np.zeros((G, 4), dtype=np.int16)
    glyph_rec[:, 0], glyph_rec[:, 1] = a, b
    glyph_rec[:, 2] = tok.astype(np.uint16).view(np.int16)
    return line_rec, glyph_rec, ""


def paint_host(table: GlyphTable) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (char_ids, line_ids, char_pos) uint16 [h, w]: what the kernel computes, as the kernel computes it.  Every pixel takes
    its line id from the last line with text whose rows hold it and whose box or glyph spans hold its column, and its character
    from the last line whose rows hold it and that has a glyph span over its column: the lines are visited from last to first
    and a pixel keeps the first answer it gets."""
    if not table.ok:
        raise ValueError(f"the table does not represent the document ({table.reason}): paint it with the host painter")
    h, w = table.shape
    char_ids, line_ids, char_pos = (np.zeros((h, w), dtype=np.uint16) for _ in range(3))
    xs = np.arange(w)
    for li in range(len(table.line_rec) - 1, -1, -1):
        x1, y1, x2, y2, g0, n = (int(v) for v in table.line_rec[li, :6])
        if n == 0:
            continue
        rows = slice(min(max(y1, 0), h), min(max(y2, 0), h))
        g = table.glyph_rec[g0:g0 + n]
        ga, gb, tok = g[:, 0].astype(np.int64), g[:, 1].astype(np.int64), g[:, 2].view(np.uint16)
        k = np.searchsorted(ga, xs, side="right") - 1                    # the last span that starts at or before x
        hit = (k >= 0) & (xs < gb[np.maximum(k, 0)])
        covered = hit | ((xs >= x1) & (xs < x2))
        free = line_ids[rows] == 0
        line_ids[rows] = np.where(free & covered[None, :], li + 1, line_ids[rows])
        free = (char_pos[rows] == 0) & hit[None, :]
        char_ids[rows] = np.where(free, tok[np.maximum(k, 0)][None, :], char_ids[rows])
        char_pos[rows] = np.where(free, (k + 1)[None, :], char_pos[rows])
    return char_ids, line_ids, char_pos


def pack_tables(tables: Sequence[GlyphTable], round_to: int = 16):
    """The tables of a group of documents as ONE upload.  -> (records, offsets, sizes, canvas): records int32 [n] = line offsets
    [B + 1] | glyph offsets [B + 1] | sizes [B][2] | line records | glyph records; offsets: where each part starts in it (in
    int32); sizes int64 [B, 2] of (h, w); canvas (H, W) rounded up to `round_to` as `ragged.pack_ids` rounds (1: a single
    document on its own shape).  A table that does not represent its document takes part as a document without lines: paint
    it on the host and `upload_host_masks`."""
    if len(tables) == 0:
        raise ValueError("pack_tables: no documents")
    if round_to < 1:
        raise ValueError(f"pack_tables: round_to must be >= 1, got {round_to}")
    B = len(tables)
    sizes = np.array([t.shape for t in tables], dtype=np.int64).reshape(B, 2)
    if (sizes < 1).any():
        raise ValueError(f"pack_tables: empty document, sizes {sizes.tolist()}")
    canvas = tuple(int(-(-int(sizes[:, d].max()) // round_to) * round_to) for d in (0, 1))
    n_lines = [len(t.line_rec) if t.ok else 0 for t in tables]
    n_glyphs = [len(t.glyph_rec) if t.ok else 0 for t in tables]
    offsets = {"line_off": 0, "glyph_off": B + 1, "sizes": 2 * B + 2, "lines": 4 * B + 2}
    offsets["glyphs"] = offsets["lines"] + LINE_INTS * sum(n_lines)       # an even number of int32: 8-byte aligned
    records = np.zeros(offsets["glyphs"] + 2 * sum(n_glyphs), dtype=np.int32)
    records[1:B + 1] = np.cumsum(n_lines)
    records[B + 2:2 * B + 2] = np.cumsum(n_glyphs)
    records[offsets["sizes"]:offsets["lines"]] = sizes.reshape(-1)
    lr = [t.line_rec.reshape(-1) for t in tables if t.ok and len(t.line_rec)]
    if lr:
        records[offsets["lines"]:offsets["glyphs"]] = np.concatenate(lr)
    gr = [t.glyph_rec.reshape(-1) for t in tables if t.ok and len(t.glyph_rec)]
    if gr:
        records[offsets["glyphs"]:] = np.concatenate(gr).view(np.int32)
    return records, offsets, sizes, canvas


def paint_device(records: np.ndarray, offsets: dict, sizes: np.ndarray, canvas: Tuple[int, int], device=None):
    """`pack_tables`' result -> (ids int32, line_ids int16, char_pos int16) [B, H, W] on the device, painted by one launch of
    csrc/paint.hip on the current stream: ids 0 for the background of a document and -1 outside every document, the two masks
    (uint16 bits) 0 outside.  Nothing is cleared first and nothing comes back: the kernel writes every pixel of the canvases."""
    import torch
    from .. import _lib as L
    if not torch.cuda.is_available():
        raise RuntimeError("paint_device paints through libmsau_hip.so on an MI355X; no GPU is visible (paint_host is the "
                           "statement it is tested against, not a fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    B, (H, W) = len(sizes), canvas
    rec_d = torch.from_numpy(records).to(dev)
    ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    line_ids = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    char_pos = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    base = rec_d.data_ptr()
    L.call("msau_kv_paint", torch.cuda.current_stream(dev).cuda_stream, base + 4 * offsets["lines"], base + 4 * offsets["glyphs"],
           base + 4 * offsets["line_off"], base + 4 * offsets["glyph_off"], base + 4 * offsets["sizes"], B, H, W,
           ids.data_ptr(), line_ids.data_ptr(), char_pos.data_ptr())
    STATS["calls"] += 1
    STATS["documents"] += B
    STATS["h2d_bytes"] += records.nbytes
    return ids, line_ids, char_pos


def upload_host_masks(canvases, b: int, masks) -> None:
    """document b of the painted canvases from the host painter's (char_ids, line_ids, char_pos): the way of a document whose
    table does not represent it"""
    import torch
    ids, line_ids, char_pos = canvases
    h, w = masks[0].shape
    ids[b, :h, :w].copy_(torch.from_numpy(masks[0].astype(np.int32)))
    line_ids[b, :h, :w].copy_(torch.from_numpy(np.ascontiguousarray(masks[1]).view(np.int16)))
    char_pos[b, :h, :w].copy_(torch.from_numpy(np.ascontiguousarray(masks[2]).view(np.int16)))
    STATS["host_painted"] += 1
    STATS["h2d_bytes"] += 8 * h * w
