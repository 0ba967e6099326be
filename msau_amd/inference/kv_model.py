"""Key-value inference model (reference: inference/kv_model.py `KVModel`).

Host side as in the reference -- character-id / line-id / character-position masks from the layout+OCR JSON, the
connected-component post-processing that turns the class map into field texts -- with the network between them run
by the forward-only HIP plan:

    reference (kv_model.py:274-279, 305-309)              here
    to_categorical(mask) -> float [1,C,H,W] -> .cuda()    int32 id mask [1,H,W] -> device, one-hot painted by a kernel
    net(batch_x) (autograd-free forward)                  MSAUWrapper.predict_nhwc: buffers reused, nothing saved
    softmax, transpose to NHWC, .cpu()                    softmax + argmax in the end conv's epilogue, NHWC output

There is no CPU network path: without the HIP library / a GPU `predict` raises (msau_amd.model).

`device_post=True` (predict, predict_batch, run_test) keeps the class map on the device as well: the line-id and
character-position masks and the line boxes go up with the ids, a kernel behind the forward extracts the field regions
(csrc/regions.hip, msau_amd.inference.regions), and the host selects the fields from that table.  Same results; the default
(False) is the path above, unchanged.

`device_masks=True` (with `device_post=True`) paints the three masks on the device as well: a document goes up as its glyph
table (msau_amd.inference.glyphs: 32 bytes per line, 8 per character), one launch (csrc/paint.hip) writes the canvases the
forward and the region kernel read, and the host builds a per-pixel array only for a document that falls back.  Same results.

`large_documents=True` (with `device_post=True`, with or without `device_masks`) sends a page of more pixels than the region
kernel holds in LDS through that kernel's large form (labels in device memory) and not through the host fallback.  Same results.

`confidence=True` (predict, predict_batch, run_test; on every path above) gives each field a score beside its text: the mean
probability of the field's class over the pixels of its kept regions (msau_amd.inference.regions.field_confidences).  On the
device paths the scored form of the region kernel sums the probabilities where the head left them; on the host path
`regions_host(..., probs=)` sums the copy that path already has.  Integer sums and one division: the same float on every path.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .generic_util import read_json_gt, sort_box_reading_order, to_categorical  # noqa: F401  (API parity)
from .morph_util import IoU, area, connected_components, intersect_boxes, r_closing, union_boxes, ycenter
from .postprocess import CLASS_NAMES, post_process_kv, post_process_kv_scored  # noqa: F401


def _obj_box(o):
    return [o[1].start, o[0].start, o[1].stop, o[0].stop]


class KVModel:
    """Inference key-value model; attribute and method names follow kv_model.py:15-387."""

    default_config = {"scale": 3.0, "charset": "", "model_kv": "", "n_class": 0}

    # fields whose value may span several text lines (kv_model.py:155)
    multiple_lines_fields = (5, 11)

    def __init__(self, net=None):
        self.net = net                      # the reference expects the caller to set this before load()
        self.scale = None
        self.tok_to_id, self.id_to_tok = None, None
        self.blank_idx = 1
        self.n_token = 1
        self.charset = ""
        self.n_class = 1

    # ---- configuration (kv_model.py:36-59) ---------------------------------------------------------------------
    def load(self, **config):
        """config: model_weight (state_dict file), charset (text file or None), n_class; optional `model_kwargs`
        and `dtype` build the network here when the caller did not supply one."""
        self.set_charset(config["charset"])
        self.n_class = config["n_class"]
        self.scale = self.default_config["scale"]
        if self.net is None:
            from ..model import MSAUWrapper
            kw = dict(config.get("model_kwargs", {}))
            if "dtype" in config:
                kw["dtype"] = config["dtype"]
            self.net = MSAUWrapper(channels=self.n_token, n_class=self.n_class, model_kwargs=kw)
        if torch.cuda.is_available():
            self.net = self.net.cuda()
        self.net.load_weights(config["model_weight"])
        self.net.eval()

    def set_charset(self, path_charset):
        """token 0 is ' ' (also the background id), token 1 is '$' (unknown / blank), then the file's characters"""
        if path_charset is None:
            self.charset = None
            return
        with open(path_charset, "r") as fh:
            self.charset = " " + "$" + fh.read()
        self.blank_idx = 1
        self.tok_to_id = {tok: i for i, tok in enumerate(self.charset)}      # later duplicates win, as in the reference
        self.id_to_tok = {i: tok for tok, i in self.tok_to_id.items()}
        self.n_token = len(self.tok_to_id)

    @staticmethod
    def _read_json_layout_ocr(json_path):
        with open(json_path, "r") as fh:
            return json.load(fh)

    # ---- input masks (kv_model.py:83-148) ------------------------------------------------------------------------
    def _generate_masks_from_label(self, label_path):
        """-> (char-id mask, line-id mask, char-position mask  [uint16, H x W], lines (boxes rewritten to grid
        coordinates), scale, background pad, (min_x, min_y, max_x, max_y) of the text in page coordinates).
        The grid is the text bounding box grown by 3 median line heights, scaled so that a median line is 3 px high.
        Digits are folded to '0'; character k of a line occupies [x1 + k*cw, x1 + k*cw + 0.9*cw) (at least 1 px,
        at most 1.2 line heights); later lines / characters overwrite earlier ones."""
        doc = self._read_json_layout_ocr(label_path)
        lines = doc["lines"]
        left, top = min(l["box"][0] for l in lines), min(l["box"][1] for l in lines)
        right, bottom = max(l["box"][2] for l in lines), max(l["box"][3] for l in lines)
        text_bbox = (left, top, right, bottom)
        median_h = np.median([l["box"][3] - l["box"][1] for l in lines])
        bg_pad = int(median_h * 3)
        left, top, right, bottom = left - bg_pad, top - bg_pad, right + bg_pad, bottom + bg_pad
        scale = 3.0 / median_h
        shape = [int((bottom - top) * scale), int((right - left) * scale)]
        char_ids = np.zeros(shape, dtype="uint16")
        line_ids = np.zeros(shape, dtype="uint16")
        char_pos = np.zeros(shape, dtype="uint16")
        for li, line in enumerate(lines):
            _type, _value = line["type"], line["value"]                 # required keys (kv_model.py:115)
            bx1, by1, bx2, by2 = line["box"]
            x1, y1 = int((bx1 - left) * scale), int((by1 - top) * scale)
            x2, y2 = int((bx2 - left) * scale), int((by2 - top) * scale)
            line["box"] = [x1, y1, x2, y2]
            text = "".join("0" if ch.isdigit() else ch for ch in line["text"])
            if not text:
                continue
            pitch = max(1.0 * (x2 - x1) / len(text), 1.0)
            glyph_w = min(max(0.9 * pitch, 1.0), int((y2 - y1) * 1.2))
            line_ids[y1:y2, x1:x2] = li + 1
            for k, ch in enumerate(text):
                xs = x1 + k * pitch
                a, b = int(xs), int(xs + glyph_w)
                char_ids[y1:y2, a:b] = self.tok_to_id.get(ch, self.blank_idx)
                line_ids[y1:y2, a:b] = li + 1
                char_pos[y1:y2, a:b] = k + 1
        return char_ids, line_ids, char_pos, lines, scale, bg_pad, text_bbox

    # ---- post-processing (kv_model.py:150-261) ------------------------------------------------------------------
    @staticmethod
    def _extract_value(line_mask, char_mask, label_lines, pred_mask, num_classes, pred_class=None):
        """Class map -> per-class (text, [region box], intersection box, union box) and the cleaned class mask.

        For every class c >= 2: close the argmax region with a 1x3 element, take its connected components and keep
        the one with the largest bounding box (multi-line fields: the top-most one as the main region plus every
        other component with a box area > 5); a main box of area < 5 drops the class.  The text lines under the kept
        regions belong to the field.  A line claimed by one field contributes its whole text; a line shared between
        fields contributes the character span its kept pixels cover (start widened by one character, end snapped to
        the line end when within 3 characters of it).  `pred_class` may carry a precomputed argmax (the device head's)."""
        n_class = pred_mask.shape[2]
        multi = KVModel.multiple_lines_fields
        values = [("", None, None, None)] * n_class
        if pred_class is None:
            pred_class = np.argmax(pred_mask, axis=-1)
        kept = np.zeros(pred_mask.shape)
        kept[:, :, 0] = pred_mask[:, :, 0]
        claims = [0] * (len(label_lines) + 1)
        field_lines = [[] for _ in range(num_classes + 1)]
        field_boxes = [[] for _ in range(num_classes + 1)]
        for i, line in enumerate(label_lines):
            line["id"] = i + 1

        def lines_under(labels, comp):
            return [v for v in np.unique(line_mask[labels == comp + 1]) if v > 0]

        for c in range(2, n_class):
            labels, objects = connected_components(r_closing(pred_class == c, (1, 3)))
            if len(objects) == 0:
                continue
            if c in multi:
                order = np.argsort([-ycenter(o) for o in objects])       # last = top-most
            else:
                order = np.argsort([area(o) for o in objects])           # last = largest box
            main = order[-1]
            if area(objects[main]) < 5:
                continue
            extra = []
            if c in multi:
                for comp in order[:-1]:
                    if area(objects[comp]) > 5:
                        extra.append(comp)
                        field_boxes[c].append(_obj_box(objects[comp]))
            field_boxes[c].append(_obj_box(objects[main]))
            ids = lines_under(labels, main)
            for comp in extra:
                ids += lines_under(labels, comp)
                kept[:, :, c][labels == comp + 1] = 1
            field_lines[c] = list(set(ids))
            for v in ids:
                claims[v] += 1
            kept[:, :, c][labels == main + 1] = 1

        for c in range(2, n_class):
            if len(field_lines[c]) == 0:
                continue
            ordered = sort_box_reading_order([label_lines[i - 1] for i in field_lines[c] if i > 0])
            text, rects = "", []
            for line in ordered:
                rects.append(line["box"])
                if claims[line["id"]] <= 1:
                    text += line["text"]
                else:
                    x1, y1, x2, y2 = line["box"]
                    covered = set(np.unique(char_mask[y1:y2, x1:x2][kept[:, :, c][y1:y2, x1:x2] > 0]))
                    covered.discard(0)
                    if len(covered) == 0:
                        continue                                        # (also skips the line break below)
                    first, last = min(covered), max(covered)
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
        return values, kept

    # ---- evaluation bookkeeping the reference does inside its drawing routine (generic_util.py:166-189) ----------
    @staticmethod
    def _count_predictions(values, n_class, eval_results, correct_answers):
        for value_id in range(1, n_class):
            if values[value_id][1] is None:
                continue
            for box in values[value_id][1]:
                eval_results[value_id]["num_pred"] += 1
                if correct_answers is not None:
                    gt = correct_answers[value_id][0][:1] if value_id in correct_answers else []
                    if any(IoU(box, g) > 0.7 for g in gt):
                        eval_results[value_id]["num_correct"] += 1

    # ---- the network (kv_model.py:274-309) ------------------------------------------------------------------------
    def _run_net(self, input_mask):
        """char-id mask [H,W] -> (pred fp32 [H,W,n_class] numpy, argmax uint8 [H,W] numpy) through the HIP plan"""
        if not torch.cuda.is_available():
            raise RuntimeError("KVModel.predict runs the network through libmsau_hip.so on an MI355X; no GPU is "
                               "visible and there is no CPU fallback")
        ids = torch.from_numpy(input_mask.astype(np.int32))[None]
        pred, amax = self.net.predict_nhwc(ids=ids.cuda())
        return pred[0].cpu().numpy(), amax[0].cpu().numpy()

    def _run_net_batch(self, input_masks):
        """char-id masks [h_b, w_b] -> per document (pred fp32 [h_b, w_b, n_class], argmax uint8 [h_b, w_b]) numpy: ONE ragged
        forward over the group (msau_amd.data.ragged.pack_ids, MSAUWrapper.predict_nhwc(ids=..., sizes=...)) and one copy of
        the canvas outputs to the host, then a crop per document"""
        if not torch.cuda.is_available():
            raise RuntimeError("KVModel.predict runs the network through libmsau_hip.so on an MI355X; no GPU is "
                               "visible and there is no CPU fallback")
        from ..data.ragged import pack_ids
        ids, sizes = pack_ids(input_masks)
        pred, amax = self.net.predict_nhwc(ids=ids.cuda(), sizes=sizes)
        pred, amax = pred.cpu().numpy(), amax.cpu().numpy()
        return [(np.ascontiguousarray(pred[b, :h, :w]), np.ascontiguousarray(amax[b, :h, :w]))
                for b, (h, w) in enumerate(sizes.tolist())]

    def _read_answers(self, label_path, scale, offset, eval_results, notes=None):
        """the ground-truth boxes of a document (None without `label_path`), counted into `eval_results`.  A file that cannot
        be read is reported at once, or appended to `notes` (the arguments of the print) for the caller to report later."""
        correct_answers = None
        if label_path is not None:
            try:
                correct_answers = read_json_gt(label_path, scale=scale, offset=offset)
            except IOError as e:
                if notes is None:
                    print("Error reading CA", e)
                else:
                    notes.append(("Error reading CA", e))
        if correct_answers is not None:
            for value_id in correct_answers:
                eval_results[value_id]["num_label"] += 1
        return correct_answers

    def _fallback_table(self, amax, b, host_masks, boxes, confidence):
        """the table of document `b`, whose overflow flag is set, from `regions_host` on its crop of the class map (and, with
        `confidence`, of the probabilities), copied back for that document alone -> (table, scores or None)"""
        from . import regions as R
        h, w = host_masks[0].shape
        cls = amax[b, :h, :w].cpu().numpy()
        R.STATS["fallbacks"] += 1
        R.STATS["d2h_bytes"] += cls.nbytes
        if not confidence:
            return R.regions_host(cls, host_masks[1], host_masks[2], boxes, self.n_class), None
        probs = np.ascontiguousarray(self.net.last_head_probs[b, :h, :w].cpu().numpy())
        R.STATS["d2h_bytes"] += probs.nbytes
        return R.regions_host(cls, host_masks[1], host_masks[2], boxes, self.n_class, probs=probs)

    def _run_regions(self, docs_masks, large=False, confidence=False):
        """`device_post`: the masks of a group of documents -> per document its region table.  One forward (dense at one
        document, ragged otherwise) with the region kernel behind it; a document whose overflow flag is set (more pixels, regions
        or pairs than the kernel's tables hold) gets its table from `regions_host` on its crop of the class map, copied back for
        that document alone -- the same table, never an approximation.  `large`: more pixels are no overflow (`regions_device`).
        -> (tables, scores): scores is None without `confidence`, else per document its regions' sums (scored form of the kernel)."""
        if not torch.cuda.is_available():
            raise RuntimeError("KVModel.predict runs the network through libmsau_hip.so on an MI355X; no GPU is "
                               "visible and there is no CPU fallback")
        from ..data.ragged import pack_ids, pack_masks
        boxes = [[l["box"] for l in m[3]] for m in docs_masks]
        if len(docs_masks) == 1:
            m = docs_masks[0]
            ids, sizes = torch.from_numpy(m[0].astype(np.int32))[None], None
            line_ids = torch.from_numpy(np.ascontiguousarray(m[1]).view(np.int16))[None]
            char_pos = torch.from_numpy(np.ascontiguousarray(m[2]).view(np.int16))[None]
        else:
            ids, sizes = pack_ids([m[0] for m in docs_masks])
            line_ids, _ = pack_masks([m[1] for m in docs_masks])
            char_pos, _ = pack_masks([m[2] for m in docs_masks])
        tables, flags, amax, *scores = self.net.predict_regions(ids=ids.cuda(), sizes=sizes, line_ids=line_ids, char_pos=char_pos,
                                                                boxes=boxes, large=large, **({"scores": True} if confidence else {}))
        scores = scores[0] if confidence else [None] * len(docs_masks)
        for b, m in enumerate(docs_masks):
            if flags[b] != 0:
                tables[b], scores[b] = self._fallback_table(amax, b, m[:3], boxes[b], confidence)
        return tables, scores if confidence else None

    def _doc_for_paint(self, json_path):
        """`device_masks`: -> (masks, glyph table) of a document; `masks` is the tuple of `_generate_masks_from_label` with None
        for the three planes, or the host painter's own when the table cannot represent the document"""
        from .glyphs import glyph_table
        table = glyph_table(json_path, self.tok_to_id, self.blank_idx)
        if not table.ok:
            return self._generate_masks_from_label(json_path), table
        return (None, None, None, table.lines, table.scale, table.bg_pad, table.text_bbox), table

    def _run_regions_painted(self, docs, json_paths, large=False, confidence=False):
        """`_run_regions` with the masks painted on the device: docs = [(masks, glyph table)] of `_doc_for_paint`.  One upload of
        the group's tables and one launch paint the canvases; a document without a table has its host masks copied into them.  A
        document whose overflow flag is set has its masks painted on the host then, for `regions_host`.  -> (tables, scores) as
        `_run_regions`."""
        if not torch.cuda.is_available():
            raise RuntimeError("KVModel.predict runs the network through libmsau_hip.so on an MI355X; no GPU is "
                               "visible and there is no CPU fallback")
        from . import glyphs as G
        boxes = [[l["box"] for l in m[3]] for m, _ in docs]
        single = len(docs) == 1
        records, offsets, sizes, canvas = G.pack_tables([t for _, t in docs], round_to=1 if single else 16)
        ids, line_ids, char_pos = G.paint_device(records, offsets, sizes, canvas)
        for b, (m, t) in enumerate(docs):
            if not t.ok:
                G.upload_host_masks((ids, line_ids, char_pos), b, m[:3])
        tables, flags, amax, *scores = self.net.predict_regions(ids=ids, sizes=None if single else torch.from_numpy(sizes),
                                                                line_ids=line_ids, char_pos=char_pos, boxes=boxes, large=large,
                                                                **({"scores": True} if confidence else {}))
        scores = scores[0] if confidence else [None] * len(docs)
        for b, (m, t) in enumerate(docs):
            if flags[b] != 0:
                host = m[:3] if m[0] is not None else self._generate_masks_from_label(json_paths[b])[:3]
                tables[b], scores[b] = self._fallback_table(amax, b, host, boxes[b], confidence)
        return tables, scores if confidence else None

    def _finish_regions(self, masks, table, correct_answers, eval_results, scores=None):
        """`_finish` from a region table (and, for `confidence`, its regions' sums)"""
        from .regions import field_confidences, fields_from_regions, select_regions
        if scores is None:
            values = fields_from_regions(table, masks[3], self.n_class)
            kv_results = post_process_kv(values)
        else:
            selection = select_regions(table, masks[3], self.n_class)   # once for both
            values = fields_from_regions(table, masks[3], self.n_class, selection)
            kv_results = post_process_kv_scored(values, field_confidences(table, scores, masks[3], self.n_class, selection))
        if eval_results is not None:
            self._count_predictions(values, self.n_class, eval_results, correct_answers)
        return kv_results

    def _finish(self, masks, a_pred, a_cls, correct_answers, eval_results, confidence=False):
        """post-processing of one document's prediction -> kv_results; `confidence`: the fields' scores from `regions_host` on
        the same prediction (its table selects the regions `_extract_value` keeps)"""
        _input_im, line_mask, char_mask, label_lines = masks[:4]
        values, _pred_mask = self._extract_value(line_mask, char_mask, label_lines, a_pred, self.n_class,
                                                 pred_class=a_cls.astype(np.int64))
        if not confidence:
            kv_results = post_process_kv(values)
        else:
            from .regions import field_confidences, regions_host
            table, scores = regions_host(a_cls, line_mask, char_mask, [l["box"] for l in label_lines], self.n_class,
                                         probs=np.ascontiguousarray(a_pred, dtype=np.float32))
            kv_results = post_process_kv_scored(values, field_confidences(table, scores, label_lines, self.n_class))
        if eval_results is not None:
            self._count_predictions(values, self.n_class, eval_results, correct_answers)
        return kv_results

    @staticmethod
    def _check_flags(device_post, device_masks, large_documents=False):
        if device_masks and not device_post:
            raise ValueError("device_masks=True needs device_post=True: the host post-processing reads the masks on the host")
        if large_documents and not device_post:
            raise ValueError("large_documents=True needs device_post=True: it chooses the form of the region kernel")

    def predict(self, data, debug_info=None, label_path=None, eval_results=None, device_post=False, device_masks=False,
                large_documents=False, confidence=False):
        """data = (layout JSON path, page image or None) -> ({field: text}, debug image).
        The debug rendering of the reference (OpenCV + PIL drawing) is not part of this build: the second result is
        always None; everything that feeds `kv_results` and `eval_results` is computed as in kv_model.py:264-347.
        device_post=True: the field regions are extracted on the device (module docstring); the results are the same.
        device_masks=True (needs device_post): the masks are painted on the device from the glyph table; the results are the same.
        large_documents=True (needs device_post): a page beyond the region kernel's LDS form stays on the device; the same results.
        confidence=True (any path): -> ({field: {"text": text, "confidence": float or None}}, None), the texts as without it; the
        confidence is the mean probability of the field's class over its kept regions (module docstring), None without a field."""
        self._check_flags(device_post, device_masks, large_documents)
        json_path, _debug_im = data
        masks, table = self._doc_for_paint(json_path) if device_masks else (self._generate_masks_from_label(json_path), None)
        input_im, _line_mask, _char_mask, _label_lines, scale, bg_pad, (min_x, min_y, _max_x, _max_y) = masks
        correct_answers = self._read_answers(label_path, scale, (min_x - bg_pad, min_y - bg_pad), eval_results)
        if device_post:
            tables, scores = (self._run_regions_painted([(masks, table)], [json_path], large_documents, confidence) if device_masks
                              else self._run_regions([masks], large_documents, confidence))
            return self._finish_regions(masks, tables[0], correct_answers, eval_results, scores[0] if confidence else None), None
        a_pred, a_cls = self._run_net(input_im)
        return self._finish(masks, a_pred, a_cls, correct_answers, eval_results, confidence), None

    def predict_batch(self, json_paths, label_paths=None, eval_results=None, device_post=False, device_masks=False,
                      large_documents=False, confidence=False):
        """`predict` for a group of layout JSONs with one network forward: the documents' id masks share a ragged canvas
        (each is computed as it would be alone).  -> [kv_results] in the order of `json_paths`.  The ground truth of the whole
        group is read before the forward, so a label file that cannot be read is reported before any result is returned
        (`run_test` prints each such message next to its own document, as at batch 1).  device_post=True, device_masks=True: as
        in `predict`; the group's glyph tables go up in one copy and one launch paints its canvases.  large_documents=True: as in
        `predict`, for the pages of the group that need it.  confidence=True: as in `predict`."""
        results, notes = self._predict_group(json_paths, label_paths, eval_results, device_post, device_masks, large_documents,
                                             confidence)
        for doc_notes in notes:
            for n in doc_notes:
                print(*n)
        return results

    def _predict_group(self, json_paths, label_paths, eval_results, device_post=False, device_masks=False, large_documents=False,
                       confidence=False):
        """predict_batch -> ([kv_results], per document the list of its unprinted messages)"""
        self._check_flags(device_post, device_masks, large_documents)
        docs, notes, painted = [], [], []
        for k, json_path in enumerate(json_paths):
            if device_masks:
                masks, table = self._doc_for_paint(json_path)
                painted.append((masks, table))
            else:
                masks = self._generate_masks_from_label(json_path)
            scale, bg_pad, (min_x, min_y, _max_x, _max_y) = masks[4:]
            label_path = label_paths[k] if label_paths is not None else None
            notes.append([])
            docs.append((masks, self._read_answers(label_path, scale, (min_x - bg_pad, min_y - bg_pad), eval_results,
                                                   notes[-1])))
        if device_post:
            tables, scores = (self._run_regions_painted(painted, json_paths, large_documents, confidence) if device_masks
                              else self._run_regions([masks for masks, _ in docs], large_documents, confidence))
            return [self._finish_regions(masks, table, correct_answers, eval_results, scores[b] if confidence else None)
                    for b, ((masks, correct_answers), table) in enumerate(zip(docs, tables))], notes
        outs = self._run_net_batch([masks[0] for masks, _ in docs])
        return [self._finish(masks, a_pred, a_cls, correct_answers, eval_results, confidence)
                for (masks, correct_answers), (a_pred, a_cls) in zip(docs, outs)], notes

    def run_test(self, list_inf, out_dir, label_dir=None, img_dir=None, batch_size=1, device_post=False, device_masks=False,
                 large_documents=False, confidence=False):
        """predict every layout JSON of `list_inf`; with `label_dir`, print per-class counts and precision / recall /
        F1 over region boxes (kv_model.py:350-387).  Unlike the reference a missing page image does not skip the
        document, because no debug image is drawn.  batch_size > 1: consecutive groups of `batch_size` documents go through
        the network as one ragged forward (as in `predict_batch`); results, printing and `eval_results` keep the order of
        `list_inf`, and the last group may be shorter.  The counts are kept as `self.eval_results`.  device_post=True: the
        field regions of every document are extracted on the device (module docstring); results and printing are the same.
        device_masks=True (needs device_post): the masks are painted on the device as well; results and printing are the same.
        large_documents=True (needs device_post): pages beyond the region kernel's LDS form stay on the device; the same again.
        confidence=True: every result is {field: {"text", "confidence"}} (as in `predict`); `eval_results` and the printed counts
        are what they are without it."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        self._check_flags(device_post, device_masks, large_documents)
        eval_results = [{"num_pred": 0, "num_correct": 0, "num_label": 0} for _ in range(self.n_class)]
        self.eval_results = eval_results
        kv_results = []
        for k in range(0, len(list_inf), batch_size):
            group = list_inf[k:k + batch_size]
            names = [os.path.basename(p).split(".")[0] for p in group]
            label_paths = [os.path.join(label_dir, n + ".json") for n in names] if label_dir is not None else None
            if batch_size == 1:
                results = [self.predict((group[0], None), debug_info=("", None),
                                        label_path=label_paths[0] if label_paths is not None else None,
                                        eval_results=eval_results, device_post=device_post, device_masks=device_masks,
                                        large_documents=large_documents, confidence=confidence)[0]]
                notes = [[]]                                     # (printed by predict)
            else:
                results, notes = self._predict_group(group, label_paths, eval_results, device_post, device_masks, large_documents,
                                                     confidence)
            for basename, result, doc_notes in zip(names, results, notes):
                for n in doc_notes:
                    print(*n)
                print(basename)
                print(result)
                kv_results.append(result)
        if label_dir is not None:
            for c, count in enumerate(eval_results):
                if count["num_pred"] > 0 or count["num_label"] > 0:
                    print(c, count)
            n_correct = np.sum([c["num_correct"] for c in eval_results])
            recall = 1.0 * n_correct / np.sum([c["num_label"] for c in eval_results])
            precision = 1.0 * n_correct / np.sum([c["num_pred"] for c in eval_results])
            f1 = 2 * recall * precision / (recall + precision)
            print("Precision : {}   Recall : {}    F1-score : {}".format(precision, recall, f1))
        return kv_results
