#!/usr/bin/env python3
"""Forward-only throughput of the inference path: MSAUWrapper.predict_nhwc at the bench size and at
the size KVModel really runs at (text lines scaled to 3 px), dense input vs the device-painted id mask.
With --ragged B: ms per document of predict_nhwc(ids) one document at a time against ragged batches of B (pack_ids +
predict_nhwc(ids=..., sizes=...)) on id masks of varied sizes around KVModel's 70 x 128 scale (60 tokens, 17 classes).
With --post B: ms per document of KVModel's post-processing on the host against device_post=True (the region kernel of
csrc/regions.hip) and against device_post=True, device_masks=True (the masks painted on the device as well, csrc/paint.hip),
interleaved in one process: (a) predict_batch end to end on the golden layouts with the golden (seeded, random-weight) net,
(b) the region stage alone on the reference's clean class maps, both arms starting from class maps on the
device.  With --post B --large: pages of more pixels than the region kernel holds in LDS (generated here, 260 x 190 at the
model's scale, 57 824 pixels with the painter's margin) through device_post=True without and with large_documents=True (host fallback against the large form of the
kernel), interleaved, with the fallback counts of each arm.  With --post B --confidence (with or without --large): one arm more,
device_post=True with confidence=True (the scored form of the region kernel), and the bytes copied back per document with and
without the scores.  Reads tests/golden/kv only.
Not the headline metric (bench.py is); numbers are quoted in DESIGN.md."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from msau_amd.model import MSAUWrapper


def run(B, C, H, W, n_class, dtype, use_ids, iters, warmup, graph=False):
    m = MSAUWrapper(C, n_class, dict(featRoot=8, scale_space_num=4, res_depth=2, filter_size=3, pool_size=2,
                                     final_act="softmax", dtype=dtype, seed=0)).cuda().eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int32)
    if use_ids:
        arg = dict(ids=ids.cuda())
    else:
        arg = dict(inp=torch.nn.functional.one_hot(ids.long(), C).permute(0, 3, 1, 2).float().cuda())
    for _ in range(warmup):
        m.predict_nhwc(graph=graph, **arg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        m.predict_nhwc(graph=graph, **arg)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    plan = next(iter(m._plans.values()))
    return {"B": B, "C": C, "H": H, "W": W, "n_class": n_class, "dtype": dtype, "input": "ids" if use_ids else "dense",
            "ms_per_call": round(dt * 1e3, 3), "tiles_per_s": round(B / dt, 1), "head_fused": plan.head_fused,
            "activation_MB": round(sum(b.numel() * b.element_size() for b in plan.buffers) / 1e6, 1),
            "launches": plan._fwd_seq[1], "graph": graph}


def run_ragged(B, n_docs, dtype, iters, warmup, C=60, n_class=17):
    from msau_amd.data.ragged import pack_ids
    m = MSAUWrapper(C, n_class, dict(featRoot=8, scale_space_num=4, res_depth=2, filter_size=3, pool_size=2,
                                     final_act="softmax", dtype=dtype, seed=0)).cuda().eval()
    g = torch.Generator().manual_seed(2)
    masks = []
    for _ in range(n_docs):
        h, w = int(torch.randint(50, 91, (1,), generator=g)), int(torch.randint(96, 161, (1,), generator=g))
        masks.append(torch.randint(0, C, (h, w), generator=g, dtype=torch.int32))
    m.max_cached_plans = 2 * n_docs + 4
    singles = [mk[None].cuda() for mk in masks]
    groups = []
    for k in range(0, n_docs, B):
        ids, sizes = pack_ids(masks[k:k + B])
        groups.append((ids.cuda(), sizes))
    out = {"n_docs": n_docs, "batch": B, "dtype": dtype, "C": C, "n_class": n_class}
    for name, calls in (("batch1", [dict(ids=s) for s in singles]), ("ragged", [dict(ids=i, sizes=s) for i, s in groups])):
        for _ in range(warmup):
            for kw in calls:
                m.predict_nhwc(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            for kw in calls:
                m.predict_nhwc(**kw)
        torch.cuda.synchronize()
        out[name + "_ms_per_doc"] = round((time.perf_counter() - t0) / iters / n_docs * 1e3, 4)
    pr = m._plan_for_shape(*groups[0][0].shape, torch.device("cuda", 0), False, ragged=True)
    out["ragged_launches"] = pr._fwd_seq[1] + 2                            # + the painter and the head
    out["speedup"] = round(out["batch1_ms_per_doc"] / out["ragged_ms_per_doc"], 3)
    return out


def run_post(B, dtype, repeats, n_docs=48, confidence=False):
    import copy
    import numpy as np
    from msau_amd.data.ragged import pack_masks
    from msau_amd.inference import KVModel
    from msau_amd.inference import glyphs as G
    from msau_amd.inference import regions as R
    from oracle import msau_oracle as O
    import tempfile
    KV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "kv")
    g, meta = np.load(os.path.join(KV, "kv.npz")), json.load(open(os.path.join(KV, "kv.json")))
    n_class, cfg = meta["n_class"], meta["net"]["cfg"]
    km = KVModel()
    with tempfile.TemporaryDirectory() as tmp:
        wpath = os.path.join(tmp, "w.pt")
        torch.save(O.init_params(cfg, meta["net"]["seed"]), wpath)
        km.load(model_weight=wpath, charset=os.path.join(KV, "charset.txt"), n_class=n_class, dtype=dtype,
                model_kwargs=dict(featRoot=cfg["featRoot"], scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                                  filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax"))
    files = [os.path.join(KV, f"layout{i % 3}.json") for i in range(n_docs)]
    groups = [files[k:k + B] for k in range(0, n_docs, B)]
    out = {"batch": B, "dtype": dtype, "n_docs": n_docs, "repeats": repeats, "n_class": n_class}

    def reset():
        for stats in (R.STATS, G.STATS):
            for k in stats:
                stats[k] = 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / n_docs * 1e3, 4)

    # (a) end to end, layout JSON -> kv_results
    arms = {"host": lambda: [km.predict_batch(gr) for gr in groups],
            "device": lambda: [km.predict_batch(gr, device_post=True) for gr in groups],
            "device_masks": lambda: [km.predict_batch(gr, device_post=True, device_masks=True) for gr in groups]}
    same = arms["host"]() == arms["device"]() == arms["device_masks"]()    # (the warm-up)
    if confidence:
        arms["device_scored"] = lambda: [km.predict_batch(gr, device_post=True, confidence=True) for gr in groups]
        texts = [[{k: v["text"] for k, v in r.items()} for r in grp] for grp in arms["device_scored"]()]
        same = same and texts == arms["device"]()
    reset()
    ms = {name: [] for name in arms}
    scored_stats = {"documents": 0, "d2h_bytes": 0}
    for _ in range(repeats):
        for name in arms:
            before = dict(R.STATS)
            ms[name].append(timed(arms[name]))
            if name == "device_scored":                                   # kept apart: the figures below are the unscored arms'
                for k in scored_stats:
                    scored_stats[k] += R.STATS[k] - before[k]
                for k in R.STATS:
                    R.STATS[k] = before[k]
    sizes = [g[f"d{i}.line_mask"].shape for i in range(3)]
    canvas = (-(-max(h for h, _ in sizes) // 16) * 16) * (-(-max(w for _, w in sizes) // 16) * 16) if B > 1 else None
    pixels = canvas if B > 1 else int(np.mean([h * w for h, w in sizes]))
    out["a_end_to_end"] = {"host_ms_per_doc": ms["host"], "device_ms_per_doc": ms["device"],
                           "device_masks_ms_per_doc": ms["device_masks"], "same_results": same,
                           "device_h2d_bytes_per_doc": 8 * pixels,          # int32 ids + two 16-bit masks per canvas pixel
                           "device_masks_h2d_bytes_per_doc": round(G.STATS["h2d_bytes"] / max(G.STATS["documents"], 1)),
                           "device_masks_host_painted": G.STATS["host_painted"],
                           "host_d2h_bytes_per_doc": pixels * (4 * n_class + 1),
                           "device_d2h_bytes_per_doc": round(R.STATS["d2h_bytes"] / max(R.STATS["documents"], 1)),
                           "fallbacks": R.STATS["fallbacks"]}
    if confidence:
        out["a_end_to_end"]["device_scored_ms_per_doc"] = ms["device_scored"]
        out["a_end_to_end"]["device_scored_d2h_bytes_per_doc"] = round(scored_stats["d2h_bytes"] / max(scored_stats["documents"], 1))
    t0 = time.perf_counter()
    for f in files:
        km._generate_masks_from_label(f)
    out["a_end_to_end"]["masks_from_label_ms_per_doc"] = round((time.perf_counter() - t0) / n_docs * 1e3, 4)
    t0 = time.perf_counter()
    for f in files:
        G.glyph_table(f, km.tok_to_id, km.blank_idx)
    out["a_end_to_end"]["glyph_table_ms_per_doc"] = round((time.perf_counter() - t0) / n_docs * 1e3, 4)

    # (b) the region stage on the reference's clean class maps, already on the device
    docs = []
    for i in range(n_docs):
        di = i % 3
        docs.append((np.argmax(g[f"d{di}.pred"].astype(np.float32), -1).astype(np.uint8), g[f"d{di}.line_mask"], g[f"d{di}.char_mask"],
                     meta[f"d{di}"]["lines"]))
    batches = []
    for k in range(0, n_docs, B):
        grp = docs[k:k + B]
        am, szs = pack_masks([d[0] for d in grp], round_to=16 if B > 1 else 1)
        am = torch.from_numpy(am.numpy().view(np.uint16).astype(np.uint8)).cuda()
        batches.append((grp, am, szs, [np.zeros(d[0].shape + (n_class,), np.float32) for d in grp]))

    def host_arm(keep=None):
        for grp, am, szs, preds in batches:
            a = am.cpu().numpy()
            for b, (d, pred) in enumerate(zip(grp, preds)):
                h, w = d[0].shape
                v, _ = KVModel._extract_value(d[1], d[2], copy.deepcopy(d[3]), pred, n_class, pred_class=a[b, :h, :w].astype(np.int64))
                if keep is not None:
                    keep.append(v)

    def device_arm(keep=None):
        for grp, am, szs, _preds in batches:
            lm, _ = pack_masks([d[1] for d in grp], round_to=16 if B > 1 else 1)
            cm, _ = pack_masks([d[2] for d in grp], round_to=16 if B > 1 else 1)
            tables, flags = R.regions_device(am, lm.cuda(), cm.cuda(), [[l["box"] for l in d[3]] for d in grp], n_class,
                                             sizes=szs if B > 1 else None)
            for d, t, f in zip(grp, tables, flags):
                if f:
                    R.STATS["fallbacks"] += 1
                    t = R.regions_host(d[0], d[1], d[2], [l["box"] for l in d[3]], n_class)
                v = R.fields_from_regions(t, copy.deepcopy(d[3]), n_class)
                if keep is not None:
                    keep.append(v)

    hv, dv = [], []
    host_arm(hv)
    device_arm(dv)
    norm = lambda o: json.loads(json.dumps(o, default=lambda v: v.item() if hasattr(v, "item") else list(v)))
    same = norm(hv) == norm(dv)
    reset()
    ms = {"host": [], "device": []}
    for _ in range(repeats):
        ms["host"].append(timed(host_arm))
        ms["device"].append(timed(device_arm))
    out["b_region_stage"] = {"host_ms_per_doc": ms["host"], "device_ms_per_doc": ms["device"], "same_results": same,
                             "device_faster_in_every_repeat": all(d < h for d, h in zip(ms["device"], ms["host"])),
                             "host_d2h_bytes_per_doc": round(sum(int(b[1].numel()) for b in batches) / n_docs),
                             "device_d2h_bytes_per_doc": round(R.STATS["d2h_bytes"] / max(R.STATS["documents"], 1)),
                             "fallbacks": R.STATS["fallbacks"]}
    tables = [R.regions_host(d[0], d[1], d[2], [l["box"] for l in d[3]], n_class) for d in docs]
    t0 = time.perf_counter()
    for d, t in zip(docs, tables):
        R.fields_from_regions(t, copy.deepcopy(d[3]), n_class)
    out["b_region_stage"]["fields_from_regions_ms_per_doc"] = round((time.perf_counter() - t0) / n_docs * 1e3, 4)
    return out


def large_layout(seed, height=260, width=190):
    """a page of text lines 3 units high (so the grid scale is 1): an A4 scan with 40 px lines at KVModel's scale, 278 x 208 =
    57 824 pixels with the painter's margin; a line every 5 rows, one to three fields of 4 to 30 characters on each"""
    import numpy as np
    rng = np.random.default_rng(seed)
    alphabet = "abcXYZ :-./#0123456789"
    lines = [{"box": [0, 0, 12, 3], "text": "abc", "type": 0, "value": 0},
             {"box": [width - 12, height - 3, width, height], "text": "xyz", "type": 0, "value": 0}]     # the page's corners
    for y in range(5, height - 8, 5):
        x = int(rng.integers(0, 30))
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(4, 31))
            x2 = x + 2 * n + int(rng.integers(0, 3))
            if x2 > width:
                break
            lines.append({"box": [x, y, x2, y + 3], "text": "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n)),
                          "type": 0, "value": 0})
            x = x2 + int(rng.integers(3, 20))
    return {"lines": lines}


def run_large(B, dtype, repeats, n_docs=16, bias_class=3, bias=6.0, confidence=False):
    """The seeded golden net with the end conv's bias of one field class raised: as it is, its class map has thousands of regions
    per class on such a page and every document overflows the per-class tables in both arms."""
    import tempfile
    import numpy as np
    from msau_amd.inference import KVModel
    from msau_amd.inference import glyphs as G
    from msau_amd.inference import regions as R
    from oracle import msau_oracle as O
    KV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "kv")
    meta = json.load(open(os.path.join(KV, "kv.json")))
    n_class, cfg = meta["n_class"], meta["net"]["cfg"]
    km = KVModel()
    with tempfile.TemporaryDirectory() as tmp:
        sd = O.init_params(cfg, meta["net"]["seed"])
        sd[f"msau_net.end_convs.{cfg.get('num_blocks', 3) - 1}.custom_conv.bias"][bias_class] += bias
        wpath = os.path.join(tmp, "w.pt")
        torch.save(sd, wpath)
        km.load(model_weight=wpath, charset=os.path.join(KV, "charset.txt"), n_class=n_class, dtype=dtype,
                model_kwargs=dict(featRoot=cfg["featRoot"], scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                                  filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax"))
        files = []
        for i in range(n_docs):
            files.append(os.path.join(tmp, f"page{i}.json"))
            with open(files[-1], "w") as fh:
                json.dump(large_layout(100 + i), fh)
        groups = [files[k:k + B] for k in range(0, n_docs, B)]
        pixels = [int(km._generate_masks_from_label(f)[0].size) for f in files]
        out = {"batch": B, "dtype": dtype, "n_docs": n_docs, "repeats": repeats, "n_class": n_class,
               "pixels_per_doc": [min(pixels), max(pixels)], "max_pixels_lds_form": R.device_limits()["max_pixels"]}
        arms = {}
        for masks in (False, True):
            for large in (False, True):
                arms[("masks_" if masks else "") + ("large" if large else "fallback")] = \
                    (lambda masks=masks, large=large: [km.predict_batch(gr, device_post=True, device_masks=masks, large_documents=large)
                                                       for gr in groups])
        first = {name: fn() for name, fn in arms.items()}                   # (the warm-up)
        out["same_results"] = all(r == first["fallback"] for r in first.values())
        if confidence:
            arms["large_scored"] = lambda: [km.predict_batch(gr, device_post=True, large_documents=True, confidence=True) for gr in groups]
            texts = [[{k: v["text"] for k, v in r.items()} for r in grp] for grp in arms["large_scored"]()]
            out["same_results"] = out["same_results"] and texts == first["fallback"]
        out["fields_found"] = sum(1 for grp in first["fallback"] for r in grp for v in r.values() if v)
        ms = {name: [] for name in arms}
        stats = {name: {k: 0 for k in R.STATS} for name in arms}
        for _ in range(repeats):
            for name, fn in arms.items():
                before = dict(R.STATS)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append(round((time.perf_counter() - t0) / n_docs * 1e3, 4))
                for k in R.STATS:
                    stats[name][k] += R.STATS[k] - before[k]
        for name in arms:
            docs = max(stats[name]["documents"], 1)
            out[name] = {"ms_per_doc": ms[name], "fallbacks": stats[name]["fallbacks"], "large_documents": stats[name]["large_documents"],
                         "documents": stats[name]["documents"], "d2h_bytes_per_doc": round(stats[name]["d2h_bytes"] / docs)}
        out["large_faster_in_every_repeat"] = all(a < b for a, b in zip(ms["large"], ms["fallback"]))
        out["masks_large_faster_in_every_repeat"] = all(a < b for a, b in zip(ms["masks_large"], ms["masks_fallback"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ragged", type=int, default=0, help="only the ragged comparison, in batches of this size")
    ap.add_argument("--docs", type=int, default=48, help="documents of the ragged comparison")
    ap.add_argument("--post", type=int, default=0, help="only the post-processing comparison (host against device_post=True and device_masks=True), "
                                                        "in batches of this size")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved repeats per arm of --post")
    ap.add_argument("--large", action="store_true", help="with --post: pages beyond the region kernel's LDS form, host fallback against "
                                                         "large_documents=True")
    ap.add_argument("--confidence", action="store_true", help="with --post: add the scored device path (confidence=True) to the comparison")
    ap.add_argument("--dtypes", default="bf16,fp32", help="with --post --large: the dtypes to run")
    a = ap.parse_args()
    if a.post and a.large:
        for dtype in a.dtypes.split(","):
            print(json.dumps(run_large(a.post, dtype, a.repeats, min(a.docs, 16), confidence=a.confidence)), flush=True)
        return
    if a.post:
        for dtype in ("bf16", "fp32"):
            print(json.dumps(run_post(a.post, dtype, a.repeats, a.docs, confidence=a.confidence)), flush=True)
        return
    if a.ragged:
        for dtype in ("bf16", "fp32"):
            print(json.dumps(run_ragged(a.ragged, a.docs, dtype, max(1, a.iters // 10), 1)), flush=True)
        return
    for cfg in ((16, 64, 336, 256, 5, "bf16"), (1, 64, 336, 256, 5, "bf16"), (1, 60, 70, 128, 17, "bf16"), (1, 60, 70, 128, 17, "fp32")):
        for use_ids, graph in ((False, False), (True, False), (True, True)):
            print(json.dumps(run(*cfg, use_ids, a.iters, a.warmup, graph)), flush=True)


if __name__ == "__main__":
    main()
