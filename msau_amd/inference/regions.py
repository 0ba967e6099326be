"""Region tables: the per-pixel part of `KVModel._extract_value`, on the device (csrc/regions.hip) or with scipy, and the host
remainder that turns a table into field values.

The table of one document, for every class c in [2, n_class):

    regions[c] = (comps, pairs)
    comps = [(first_y, first_x, y0, y1, x0, x1, pixels)]   the 4-connected components of r_closing(class_map == c, (1, 3)), in
                                                           scipy.ndimage.label's order; the box is find_objects' (half-open)
    pairs = {(k, v): (n_under, cp_min, cp_max)}            component k and text line v >= 1: pixels of k whose line id is v;
                                                           smallest / largest non-zero character position over the pixels of k
                                                           inside line v's box (65535 / 0 when there is none)

`fields_from_regions` applies the selection of `_extract_value` to it (main region, extra regions of the multi-line fields,
claims, text assembly) with the same `np.argsort` calls on the same lists, so ties fall as they do there.  It is O(regions +
text lines); everything per pixel is in the table.

With probabilities (`regions_host(..., probs=)`, `regions_device(..., probs=)`) every region also gets a score, the integer sum of
its class's quantised probability over its pixels; `field_confidences` turns the scores of a field's kept regions into the mean
probability the network gave that field.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
from scipy import ndimage as ndi

from .generic_util import sort_box_reading_order
from .morph_util import area, intersect_boxes, r_closing, union_boxes, ycenter

OVF_PIXELS, OVF_LABEL, OVF_REGIONS, OVF_PAIRS, OVF_LINES = 1, 2, 4, 8, 16

# per-document capacities of the device lists when the caller names none: what a random-weight network's class map produces
# at KVModel's scale with room to spare (929 regions, 118 pairs on a 44 x 91 document); 320 KiB per document on the device
DEFAULT_CAP_REGIONS = 8192
DEFAULT_CAP_PAIRS = 4096

# what the device path has copied and how often the host had to step in (tools/infer_bench.py reads and resets these)
# "large_documents": documents whose table the large form of the kernel wrote (`regions_device(large=True)`)
STATS = {"calls": 0, "documents": 0, "d2h_bytes": 0, "fallbacks": 0, "large_documents": 0}

# multi-line fields: KVModel.multiple_lines_fields (kv_model.py:155)
MULTIPLE_LINES_FIELDS = (5, 11)

# a region's score is the sum over its pixels of rint(p * SCORE_ONE), p the probability of the region's class (csrc/regions.hip)
SCORE_ONE = 65536


def closing_1x3(mask: np.ndarray) -> np.ndarray:
    """`r_closing(mask, (1, 3))` written out: dilate then erode along x, zero outside the array.  Columns 0 and w - 1 are
    always False (the erosion sees the outside there)."""
    m = np.asarray(mask, dtype=bool)
    d = m.copy()
    d[:, 1:] |= m[:, :-1]
    d[:, :-1] |= m[:, 1:]
    e = d.copy()
    e[:, 1:] &= d[:, :-1]
    e[:, :-1] &= d[:, 1:]
    e[:, 0] = False
    e[:, -1] = False
    return e


def quantise(p) -> np.ndarray:
    """q(p) = rint(p * 65536) as int64, to nearest even: what the scored kernel adds per pixel (p fp32; the product by 2^16 is
    exact in fp32 and in float64, so both give the same integer)"""
    return np.rint(np.asarray(p).astype(np.float64) * SCORE_ONE).astype(np.int64)


def regions_host(cls, line_mask, char_mask, boxes, n_class: int, probs=None):
    """The region table of one document on the CPU (scipy): `cls` int [h, w] class map, `line_mask` / `char_mask` uint16 [h, w],
    `boxes` the lines' [x1, y1, x2, y2] in grid coordinates (line id v = boxes[v - 1]; boxes are clipped to the document, so a
    negative coordinate counts as 0).  The statement the kernel is tested against, and the fallback of the device path.
    With `probs` (fp32 [h, w, n_class], the head's probabilities) -> (table, scores): scores[c] = per component of class c, in
    `comps` order, the int sum of `quantise(probs[y, x, c])` over its pixels (those of the closed mask: a gap pixel the closing
    added counts with the probability of c it has)."""
    cls = np.asarray(cls)
    line_mask, char_mask = np.asarray(line_mask), np.asarray(char_mask)
    h, w = cls.shape
    if probs is not None:
        probs = np.asarray(probs)
        if probs.shape != (h, w, n_class) or probs.dtype != np.float32:
            raise ValueError(f"probs must be float32 [h, w, n_class] = {(h, w, n_class)}, got {probs.dtype} {probs.shape}")
    out, scores = {}, {}
    for c in range(2, n_class):
        lab, n = ndi.label(r_closing(cls == c, (1, 3)))
        comps, pairs = [], {}
        scores[c] = []
        if n:
            ys, xs = np.nonzero(lab)                                    # raster order
            ks = lab[ys, xs].astype(np.int64) - 1
            if probs is not None:
                total = np.zeros(n, dtype=np.int64)
                np.add.at(total, ks, quantise(probs[ys, xs, c]))
                scores[c] = total.tolist()
            _, first = np.unique(ks, return_index=True)
            count = np.bincount(ks, minlength=n)
            for k, (sy, sx) in enumerate(ndi.find_objects(lab)):
                comps.append((int(ys[first[k]]), int(xs[first[k]]), sy.start, sy.stop, sx.start, sx.stop, int(count[k])))
            lv = line_mask[ys, xs].astype(np.int64)
            keys, cnt = np.unique((ks[lv > 0] << 16) | lv[lv > 0], return_counts=True)
            for key, m in zip(keys.tolist(), cnt.tolist()):
                pairs[(key >> 16, key & 0xFFFF)] = (m, 65535, 0)
            cp = char_mask[ys, xs].astype(np.int64)
            for li, (x1, y1, x2, y2) in enumerate(boxes):
                sel = (ys >= y1) & (ys < y2) & (xs >= x1) & (xs < x2) & (cp > 0)
                if not sel.any():
                    continue
                ksel, cpsel = ks[sel], cp[sel]
                for k in np.unique(ksel).tolist():
                    v = cpsel[ksel == k]
                    old = pairs.get((k, li + 1), (0, 65535, 0))
                    pairs[(k, li + 1)] = (old[0], int(v.min()), int(v.max()))
        out[c] = (comps, pairs)
    return out if probs is None else (out, scores)


def fields_from_regions(regions, label_lines, n_class: int, selection=None):
    """Region table of one document -> the `values` list of `KVModel._extract_value`: per class (text, [main region box],
    intersection box, union box), ("", None, None, None) for a class without a field.  Sets line["id"] as `_extract_value` does.
    `selection`: what `select_regions` returned for the same arguments, when the caller has it already."""
    multi = MULTIPLE_LINES_FIELDS
    values = [("", None, None, None)] * n_class
    kept, field_lines, field_boxes, claims = selection or select_regions(regions, label_lines, n_class)
    for c in range(2, n_class):
        if len(field_lines[c]) == 0:
            continue
        _comps, pairs = regions[c]
        ordered = sort_box_reading_order([label_lines[i - 1] for i in field_lines[c] if i > 0])
        text, rects = "", []
        for line in ordered:
            rects.append(line["box"])
            if claims[line["id"]] <= 1:
                text += line["text"]
            else:
                spans = [pairs[(k, line["id"])] for k in kept[c] if (k, line["id"]) in pairs]
                spans = [p for p in spans if p[2] > 0]
                if len(spans) == 0:
                    continue                                            # (also skips the line break below)
                first, last = min(p[1] for p in spans), max(p[2] for p in spans)
                if last > len(line["text"]) - 3:
                    last = len(line["text"]) + 1
                text += line["text"][first - 2 if first >= 2 else 0: last - 1]
            if c in multi:
                text += "\n"
        if len(text) > 0 and text[-1] == "\n":
            text = text[:-1]
        merged = union_boxes(rects)
        values[c] = (text, [field_boxes[c][-1]], intersect_boxes(field_boxes[c] + [merged]),
                     union_boxes(field_boxes[c] + [merged]))
    return values


def field_confidences(regions, scores, label_lines, n_class: int, selection=None) -> List[Optional[float]]:
    """The confidence of every field `fields_from_regions` yields from this table: per class None (no field) or the mean
    probability of the class over the pixels of its kept regions (the main region and, for a multi-line field, its extra
    regions), sum(score_k) / (SCORE_ONE * sum(pixels_k)) in float64.  `scores`: per class the regions' integer sums in `comps`
    order (`regions_host(..., probs=)`, `regions_device(..., probs=)`).  Integers in, one division: the same float on every
    path that produced the same table.  `selection` as in `fields_from_regions`."""
    kept, field_lines, _boxes, _claims = selection or select_regions(regions, label_lines, n_class)
    out: List[Optional[float]] = [None] * n_class
    for c in range(2, n_class):
        if len(field_lines[c]) == 0:
            continue
        comps = regions[c][0]
        total = sum(int(scores[c][k]) for k in kept[c])
        pixels = sum(int(comps[k][6]) for k in kept[c])
        out[c] = float(np.float64(total) / np.float64(SCORE_ONE * pixels))
    return out


def select_regions(regions, label_lines, n_class: int):
    """The selection of `_extract_value`, shared by `fields_from_regions` and `field_confidences`: -> (kept, field_lines,
    field_boxes, claims): per class with a main region its kept regions [main] + extra (indices into `comps`); per class the ids
    of the lines under them (empty: no field) and the regions' boxes, the main one last; per line id how many fields claim it.
    Sets line["id"] as `_extract_value` does."""
    multi = MULTIPLE_LINES_FIELDS
    claims = [0] * (len(label_lines) + 1)
    field_lines = [[] for _ in range(n_class + 1)]
    field_boxes = [[] for _ in range(n_class + 1)]
    kept = {}
    for i, line in enumerate(label_lines):
        line["id"] = i + 1
    for c in range(2, n_class):
        comps, pairs = regions[c]
        if len(comps) == 0:
            continue
        objects = [(slice(y0, y1), slice(x0, x1)) for _, _, y0, y1, x0, x1, _ in comps]
        under = {}
        for (k, v), p in pairs.items():
            if p[0] > 0:
                under.setdefault(k, []).append(v)
        if c in multi:
            order = np.argsort([-ycenter(o) for o in objects])           # last = top-most
        else:
            order = np.argsort([area(o) for o in objects])               # last = largest box
        main = int(order[-1])
        if area(objects[main]) < 5:
            continue
        extra = []

        def box_of(o):
            return [o[1].start, o[0].start, o[1].stop, o[0].stop]

        if c in multi:
            for comp in order[:-1]:
                if area(objects[comp]) > 5:
                    extra.append(int(comp))
                    field_boxes[c].append(box_of(objects[comp]))
        field_boxes[c].append(box_of(objects[main]))
        ids = sorted(under.get(main, []))
        for comp in extra:
            ids += sorted(under.get(comp, []))
        field_lines[c] = list(set(ids))
        for v in ids:
            claims[v] += 1
        kept[c] = [main] + extra
    return kept, field_lines, field_boxes, claims


# ---- the device path ------------------------------------------------------------------------------------------------
_limits = None


def device_limits() -> dict:
    """what csrc/regions.hip holds per document / per (document, class): asked from the library, not restated here"""
    global _limits
    if _limits is None:
        from .. import _lib as L
        out = (C.c_int32 * 6)()
        L.call("msau_kv_regions_limits", out)
        _limits = dict(zip(("max_pixels", "max_regions_per_class", "max_pairs_per_class", "region_ints", "pair_ints", "max_lines"),
                           (int(v) for v in out)))
    return _limits


def table_from_records(header_doc: np.ndarray, regions_doc: np.ndarray, pairs_doc: np.ndarray, n_class: int) -> Dict[int, tuple]:
    """one document's rows of the kernel's output (header [n_class][4], regions [r][8], pairs [p][4]) -> the table"""
    out = {}
    hd = header_doc.tolist()
    for c in range(2, n_class):
        roff, nr, poff, npair = hd[c]
        comps = [tuple(r[:7]) for r in regions_doc[roff:roff + nr].tolist()]
        pairs = {((key >> 16) & 0xFFFF, key & 0xFFFF): (n, lo, hi) for key, n, lo, hi in pairs_doc[poff:poff + npair].tolist()}
        out[c] = (comps, pairs)
    return out


_buffers: dict = {}
_workspaces: dict = {}


def _workspace(dev, n_ints: int):
    """the large form's labels: int32 on `dev`, kept and grown; it holds nothing between calls"""
    import torch
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < n_ints:
        _workspaces.pop(dev, None)
        ws = _workspaces[dev] = torch.empty(max(n_ints, 1), dtype=torch.int32, device=dev)
    return ws


def regions_device(argmax, line_ids, char_pos, boxes: Sequence, n_class: int, sizes=None,
                   cap_regions: Optional[int] = None, cap_pairs: Optional[int] = None,
                   large: bool = False, probs=None):
    """The region tables of a batch, by the kernel, on the current stream (so: behind the forward that wrote `argmax`).

    argmax uint8 [B, H, W] on the device (the plan's `head_argmax`, not copied); line_ids / char_pos [B, H, W] on the device,
    uint16 values in int16 (or uint16) storage, zero outside the documents (msau_amd.data.ragged.pack_masks); boxes: per document
    the [x1, y1, x2, y2] of its lines; sizes: CPU integer [B, 2] of (h, w) for a ragged batch, None for a dense one.
    cap_regions / cap_pairs: how many records a document may produce (defaults DEFAULT_CAP_*).
    large=True: the documents of more than `device_limits()["max_pixels"]` pixels (known here from their sizes, nothing is read
    back for it) get their tables from a second launch behind the first, the large form of the kernel, which keeps their labels
    in a workspace in device memory; without it such a document is flagged OVF_PIXELS.  The per-class limits and the capacities
    hold for them as for the others.
    -> ([table or None per document], [overflow flags per document]); a document with a non-zero flag (OVF_*) has no table:
    run `regions_host` on its class map.  Reads back the header (16 bytes per class) and the used prefix of the two lists.
    probs: fp32 [B, H, W, n_class] on the device (the plan's `head_probs`, not copied): the scored entry points write, beside
    every region record, the integer sum of its class's quantised probability over its pixels (`regions_host(..., probs=)` is the
    statement); the used prefix of those sums (8 bytes per region row) comes back with the regions.
    -> (tables, flags, scores): scores[b] = {class: [int per region, in `comps` order]}, None for a document with a flag."""
    import torch
    from .. import _lib as L
    if argmax.dim() != 3 or argmax.dtype != torch.uint8 or not argmax.is_cuda:
        raise ValueError("argmax must be a uint8 [B, H, W] tensor on the device")
    B, H, W = (int(v) for v in argmax.shape)
    if not (1 <= n_class <= 255):
        raise ValueError(f"n_class must be in [1, 255], got {n_class}")
    for name, t in (("line_ids", line_ids), ("char_pos", char_pos)):
        if tuple(t.shape) != (B, H, W) or t.element_size() != 2 or t.dtype.is_floating_point or t.device != argmax.device:
            raise ValueError(f"{name} must be a 16-bit integer [B, H, W] = {(B, H, W)} tensor on {argmax.device}")
    if len(boxes) != B:
        raise ValueError(f"boxes must hold one list per document ({B}), got {len(boxes)}")
    if probs is not None and (tuple(probs.shape) != (B, H, W, n_class) or probs.dtype != torch.float32 or probs.device != argmax.device
                              or not probs.is_contiguous()):
        raise ValueError(f"probs must be a contiguous float32 [B, H, W, n_class] = {(B, H, W, n_class)} tensor on {argmax.device}")
    scored = probs is not None
    lim = device_limits()
    cap_regions = DEFAULT_CAP_REGIONS if cap_regions is None else int(cap_regions)
    cap_pairs = DEFAULT_CAP_PAIRS if cap_pairs is None else int(cap_pairs)
    if cap_regions < 1 or cap_pairs < 1:
        raise ValueError("capacities must be >= 1")
    argmax, line_ids, char_pos = argmax.contiguous(), line_ids.contiguous(), char_pos.contiguous()
    # one small upload: box offsets, extents, boxes
    counts = [len(b) for b in boxes]
    n_box = sum(counts)
    small = np.zeros(B + 1 + 2 * B + 4 * max(n_box, 1), dtype=np.int32)
    small[1:B + 1] = np.cumsum(counts)
    if sizes is not None:
        sz = np.asarray(sizes, dtype=np.int64).reshape(B, 2)
        if (sz[:, 0] < 1).any() or (sz[:, 1] < 1).any() or (sz[:, 0] > H).any() or (sz[:, 1] > W).any():
            raise ValueError(f"sizes must satisfy 1 <= h <= {H} and 1 <= w <= {W}, got {sz.tolist()}")
        small[B + 1:3 * B + 1] = sz.reshape(-1)
    if n_box:
        small[3 * B + 1:] = np.concatenate([np.asarray(b, dtype=np.int64).reshape(-1, 4) for b in boxes if len(b)]).reshape(-1)
    dev = argmax.device
    small_d = torch.from_numpy(small).to(dev, non_blocking=False)
    key = (dev, B, n_class, cap_regions, cap_pairs) + (("scored",) if scored else ())
    if key not in _buffers:
        if len(_buffers) >= 8:
            _buffers.clear()
        _buffers[key] = (torch.zeros(B * n_class * 4 + B, dtype=torch.int32, device=dev),
                         torch.zeros((B, cap_regions, lim["region_ints"]), dtype=torch.int32, device=dev),
                         torch.zeros((B, cap_pairs, lim["pair_ints"]), dtype=torch.int32, device=dev)) + \
                        ((torch.zeros((B, cap_regions), dtype=torch.int64, device=dev),) if scored else ())
    head_d, reg_d, pair_d = _buffers[key][:3]
    score_d = _buffers[key][3] if scored else None
    base = small_d.data_ptr()
    inputs = (argmax.data_ptr(),) + ((probs.data_ptr(),) if scored else ()) + (line_ids.data_ptr(), char_pos.data_ptr())
    outputs = (head_d.data_ptr(), reg_d.data_ptr(), cap_regions, pair_d.data_ptr(), cap_pairs) + \
              ((score_d.data_ptr(),) if scored else ()) + (head_d.data_ptr() + 16 * B * n_class,)
    L.call("msau_kv_regions_scored" if scored else "msau_kv_regions", torch.cuda.current_stream().cuda_stream, *inputs,
           base + 4 * (3 * B + 1), base, base + 4 * (B + 1) if sizes is not None else None, B, H, W, n_class, *outputs)
    if large and n_class > 2:
        pixels = [int(h) * int(w) for h, w in sz] if sizes is not None else [H * W] * B
        big = [b for b in range(B) if pixels[b] > lim["max_pixels"]]
        if big:
            share = [(n_class - 2) * pixels[b] for b in big]
            ws = _workspace(dev, sum(share))
            docs_a = (C.c_int32 * len(big))(*big)
            off_a = (C.c_int64 * len(big))(*np.concatenate([[0], np.cumsum(share)[:-1]]).tolist())
            L.call("msau_kv_regions_large_scored" if scored else "msau_kv_regions_large", torch.cuda.current_stream().cuda_stream,
                   *inputs, base + 4 * (3 * B + 1), base, base + 4 * (B + 1) if sizes is not None else None, B, H, W,
                   n_class, docs_a, len(big), off_a, ws.data_ptr(), sum(share), *outputs)
            STATS["large_documents"] += len(big)
    head = head_d.cpu().numpy()
    header, flags = head[:B * n_class * 4].reshape(B, n_class, 4), head[B * n_class * 4:].tolist()
    ok = [b for b in range(B) if flags[b] == 0]
    used_r = max([int(header[b, 0, 0]) for b in ok], default=0)
    used_p = max([int(header[b, 0, 1]) for b in ok], default=0)
    nbytes = head.nbytes
    reg = pair = score = None
    if used_r:
        reg = reg_d[:, :used_r].cpu().numpy()
        nbytes += reg.nbytes
        if scored:
            score = score_d[:, :used_r].cpu().numpy()
            nbytes += score.nbytes
    if used_p:
        pair = pair_d[:, :used_p].cpu().numpy()
        nbytes += pair.nbytes
    empty_r, empty_p = np.zeros((0, lim["region_ints"]), np.int32), np.zeros((0, lim["pair_ints"]), np.int32)
    docs = [table_from_records(header[b], reg[b] if reg is not None else empty_r, pair[b] if pair is not None else empty_p, n_class)
            if flags[b] == 0 else None for b in range(B)]
    STATS["calls"] += 1
    STATS["documents"] += B
    STATS["d2h_bytes"] += nbytes
    if not scored:
        return docs, flags
    scores = [{c: (score[b, header[b, c, 0]:header[b, c, 0] + header[b, c, 1]].tolist() if score is not None else [])
               for c in range(2, n_class)} if flags[b] == 0 else None for b in range(B)]
    return docs, flags, scores
