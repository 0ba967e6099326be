#!/usr/bin/env python3
"""The reference's own operating point: batch 1, a different H x W per document (train_chargrid_funsd_msau.py:45-59,
data_generator_funsd_bert.py:216-222).  N synthetic documents with FUNSD-like chargrid sizes, the engine loop, every
document's plan cached; reports, as one JSON object:

  first_epoch_ms_per_doc   epoch 0: every step builds its plan (buffers, descriptors, launch lists)
  docs_per_s / ms_per_doc  epochs >= 1: plans cached, steps back to back, one host sync at the end of the epoch
  host_ms_per_doc          host time to ENQUEUE a step (the loop is launch-bound when this is close to ms_per_doc)
  launches_per_step        native launch records of the median-size plan
  graph                    the same with TrainEngine(use_graph=True): one HIP-graph replay per cached plan

  ragged                   with --ragged B: the same documents in ragged batches of B (msau_amd.data.ragged: documents of
                           similar area together, canvases rounded up to 16), TrainEngine.step(x, labels, sizes) --
                           docs/s, launches per step, the canvases used and the padded fraction of the canvases

  eval                     with --eval B: evaluation of the same documents (train_chargrid_funsd_msau.evaluate) two ways --
                           the per-document loop (forward, NCHW fp32 logit export, torch argmax, .cpu() per document) and
                           MSAUWrapper.confusion_matrix on ragged batches of B (counts on the device, one host read) --
                           docs/s of each and launches per forward

  ragged_boxes             with --ragged B --boxes: documents made of text-line boxes with a feature row each (the BERT grid of
                           data_generator_funsd_bert.py:64-93), in ragged batches of B, three ways, interleaved, --repeats times:
                           "dense"       pack() on the host, upload of the fp32 NCHW canvas, TrainEngine.step(x, labels, sizes)
                           "boxes"       pack_boxes(), upload of the lists and the table, step_boxes(..., feats=, sizes=sizes)
                           "boxes_dense" the same lists through the DENSE step_boxes on the same canvas (no sizes): what the
                                         extent flag costs on the generic kernels
                           ms per step and bytes uploaded per step of each arm, every repeat; only this comparison runs

  entities                 with --eval B --entities: entity-level predictions of the same documents (one text-line-like entity box
                           per ~150 pixels) in ragged batches of B, two ways on identical batches, interleaved, --repeats times:
                           "device"  MSAUWrapper.box_predictions: forward-only plan + msau_box_vote, the int64 matrix read once per
                                     epoch; timed with device events around the epoch (the read included)
                           "host"    forward, copy of the exported logits to the host, msau_amd.data.entities.box_vote_host; timed
                                     with the wall clock around the epoch (it ends in host work)
                           docs/s of every repeat, bytes copied to the host per document, and whether both routes gave the same
                           predictions for every box; a timed window is --epochs passes over the documents; only this comparison runs

    python tools/funsd_loop.py [--docs 120] [--epochs 3] [--channels 64] [--dtype bf16] [--graph] [--ragged 16] [--eval 16]
    python tools/funsd_loop.py --ragged 16 --boxes --channels 768 --dtype bf16 [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def doc_shapes(n, seed=0):
    """FUNSD forms are A4 scans; the chargrid cell is the smallest word box (data_generator_funsd_bert.py:153-155): grids of
    roughly 60-170 rows x 40-130 columns.  Distinct shapes, as in a real epoch (almost every document has its own)."""
    import random
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add((rng.randint(60, 170), rng.randint(40, 130)))
    return sorted(out, key=lambda s: rng.random())


def make_docs(args):
    """the synthetic documents (CPU): {"mask": [1, C, h, w], "label": [1, h, w]} as the FUNSD loader yields them"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(1)
    docs = []
    for (H, W) in doc_shapes(args.docs):
        occ = torch.rand((1, H, W), generator=g) < 0.1
        ids = torch.randint(0, args.channels, (1, H, W), generator=g)
        x = torch.zeros((1, args.channels, H, W))
        x.scatter_(1, ids.unsqueeze(1), occ.unsqueeze(1).float())
        lab = (occ * torch.randint(1, 5, (1, H, W), generator=g)).long()
        docs.append({"mask": x, "label": lab})
    return docs


def make_model(args):
    import torch
    from msau_amd import MSAUWrapper
    kw = dict(scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, final_act="softmax", num_blocks=3,
              dtype=args.dtype, seed=0)
    return MSAUWrapper(args.channels, 5, kw).to(torch.device("cuda", 0))


def _cost(args):
    """--cost NAME as TrainEngine takes it (the cost's default parameter); cross_entropy: None, the default path"""
    name = getattr(args, "cost", "cross_entropy")
    return None if name == "cross_entropy" else {"cost_name": name}


def run(args, use_graph):
    import torch
    from msau_amd import TrainEngine
    dev = torch.device("cuda", 0)
    m = make_model(args)
    shapes = doc_shapes(args.docs)
    m.max_cached_plans = 2 * len(shapes) + 2
    eng = TrainEngine(m, lr=1e-4, use_graph=use_graph, cost=_cost(args))
    docs = [(d["mask"].to(dev), d["label"].to(dev)) for d in make_docs(args)]
    torch.cuda.synchronize()
    res = {}
    t0 = time.perf_counter()
    for x, lab in docs:
        eng.step(x, lab)
    torch.cuda.synchronize()
    res["first_epoch_ms_per_doc"] = round(1e3 * (time.perf_counter() - t0) / len(docs), 3)
    times, host = [], []
    for ep in range(args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th = 0.0
        for x, lab in docs:
            h0 = time.perf_counter()
            loss = eng.step(x, lab)
            th += time.perf_counter() - h0
        he = time.perf_counter()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        times.append((t1 - t0) / len(docs))
        host.append(th / len(docs))
    best = min(times)
    res.update(docs=len(docs), epochs=args.epochs, docs_per_s=round(1.0 / best, 1), ms_per_doc=round(1e3 * best, 3),
               host_ms_per_doc=round(1e3 * min(host), 3), loss=round(float(loss), 4),
               plan_MB=round(sum(p.activation_bytes() for p in m._plans.values()) / 1e6, 1))
    med = sorted(shapes, key=lambda s: s[0] * s[1])[len(shapes) // 2]
    plan = m._plan_for_shape(1, med[0], med[1], dev, True)
    res["median_shape"] = list(med)
    res["launches_per_step"] = sum(seq[1] for seq in (plan._fwd_seq, plan._bwd_seq) if seq is not None) + 6   # + pack, convert, counts, CE, clip+Adam
    return res


def run_ragged(args, B, use_graph=False):
    """the same documents in ragged batches of B: one step per batch, loss = mean of the per-document losses"""
    import torch
    from msau_amd import TrainEngine
    from msau_amd.data.ragged import batches, pack, padded_fraction
    dev = torch.device("cuda", 0)
    m = make_model(args)
    docs = make_docs(args)
    steps = []
    for idx in batches(docs, B, round_to=16):
        x, lab, sizes = pack([docs[i] for i in idx], round_to=16)
        steps.append((x.to(dev), lab.to(dev), sizes))
    canvases = sorted({(int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) for x, _, _ in steps})
    m.max_cached_plans = 2 * len(canvases) + 2
    eng = TrainEngine(m, lr=1e-4, use_graph=use_graph, cost=_cost(args))
    torch.cuda.synchronize()
    res = {}
    t0 = time.perf_counter()
    for x, lab, sizes in steps:
        eng.step(x, lab, sizes)
    torch.cuda.synchronize()
    res["first_epoch_ms_per_doc"] = round(1e3 * (time.perf_counter() - t0) / len(docs), 3)
    times, host = [], []
    for ep in range(args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th = 0.0
        for x, lab, sizes in steps:
            h0 = time.perf_counter()
            loss = eng.step(x, lab, sizes)
            th += time.perf_counter() - h0
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / len(docs))
        host.append(th / len(steps))
    best = min(times)
    pad = sum(padded_fraction(s, int(x.shape[2]), int(x.shape[3])) * x.shape[0] * x.shape[2] * x.shape[3] for x, _, s in steps) / \
        sum(x.shape[0] * x.shape[2] * x.shape[3] for x, _, _ in steps)
    x, _, _ = steps[len(steps) // 2]
    plan = m._plan_for_shape(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), dev, True, ragged=True)
    res.update(batch=B, docs=len(docs), steps_per_epoch=len(steps), epochs=args.epochs, docs_per_s=round(1.0 / best, 1),
               ms_per_doc=round(1e3 * best, 3), ms_per_step=round(1e3 * best * len(docs) / len(steps), 3),
               host_ms_per_step=round(1e3 * min(host), 3), loss=round(float(loss), 4), canvases=[list(c) for c in canvases],
               padded_fraction=round(pad, 4), median_canvas=[int(x.shape[0]), int(x.shape[2]), int(x.shape[3])],
               # + pack, convert, zero the input outside the documents, label canvas, counts, CE, clip+Adam
               launches_per_step=sum(seq[1] for seq in (plan._fwd_seq, plan._bwd_seq) if seq is not None) + 7)
    return res


def make_box_docs(args):
    """the synthetic documents as box lists (CPU): (feature boxes, label boxes, h, w, feats [n, C]) with one text-line-like box per
    ~150 pixels, some overlapping, some over the document's edge"""
    import numpy as np
    rng = np.random.default_rng(1)
    docs = []
    for (h, w) in doc_shapes(args.docs):
        n = max(4, h * w // 150)
        fb, lb = [], []
        for i in range(n):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(-2, w - 4))
            y1, x1 = y0 + int(rng.integers(1, 4)), x0 + int(rng.integers(6, 40))
            fb.append((0, y0, y1, x0, x1, i))
            lb.append((0, y0, y1, x0, x1, int(rng.integers(1, 5))))
        docs.append((np.asarray(fb, np.int32), np.asarray(lb, np.int32), h, w, rng.standard_normal((n, args.channels)).astype(np.float32)))
    return docs


def paint_host(doc):
    """one document painted on the host as the reference's loader does (numpy slicing on its own array) -> the FUNSD loader's item"""
    import numpy as np
    import torch
    fb, lb, h, w, feats = doc
    grid, lab = np.zeros((feats.shape[1], h, w), np.float32), np.zeros((h, w), np.int64)
    for (_, y0, y1, x0, x1, v), (_, _, _, _, _, lv) in zip(fb.tolist(), lb.tolist()):
        grid[:, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = feats[v][:, None, None]
        lab[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = lv
    return {"mask": torch.from_numpy(grid)[None], "label": torch.from_numpy(lab)[None]}


def run_ragged_boxes(args, B):
    """ragged batches of the same box documents: host-painted canvas + step(x, labels, sizes) against step_boxes(..., sizes=)"""
    import torch
    from msau_amd import TrainEngine
    from msau_amd.data.ragged import batches, pack, pack_boxes
    dev = torch.device("cuda", 0)
    bdocs = make_box_docs(args)
    ddocs = [paint_host(d) for d in bdocs]
    groups = list(batches(ddocs, B, round_to=16))
    arms = ("dense", "boxes", "boxes_dense")
    models = {a: make_model(args) for a in arms}                   # an engine of its own per arm: same seed, same documents
    engs = {a: TrainEngine(models[a], lr=1e-4) for a in arms}
    for m in models.values():
        m.max_cached_plans = 2 * len(groups) + 2
    up = {a: 0 for a in arms}

    def epoch(arm, count=False):
        eng = engs[arm]
        for idx in groups:
            if arm == "dense":
                x, lab, sizes = pack([ddocs[i] for i in idx], round_to=16)
                if count:
                    up[arm] += x.numel() * 4 + lab.numel() * 8
                loss = eng.step(x.to(dev), lab.to(dev), sizes)
            else:
                gb, lb, feats, sizes, (H, W) = pack_boxes([bdocs[i] for i in idx], round_to=16)
                if count:
                    up[arm] += gb.nbytes + lb.nbytes + feats.nbytes
                loss = eng.step_boxes(gb, lb, len(idx), H, W, feats=feats, sizes=sizes if arm == "boxes" else None)
            if count and arm != "boxes_dense":
                plan = models[arm]._plan_for_shape(len(idx), *((int(x.shape[2]), int(x.shape[3])) if arm == "dense" else (H, W)), dev, True, ragged=True)
                up[arm] += plan.extents.numel() * 4
        torch.cuda.synchronize()
        return loss

    for a in arms:                                                 # plans built, first launches done; the uploads counted once
        loss = epoch(a, count=True)
    res = {a: {"ms_per_step": [], "bytes_uploaded_per_step": up[a] // len(groups), "loss": round(float(loss), 4)} for a in arms}
    for _ in range(max(args.repeats, 5)):
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(a)
            res[a]["ms_per_step"].append(round(1e3 * (time.perf_counter() - t0) / len(groups), 3))
    plan = next(p for (b, h, w, tr, rg), p in models["boxes"]._plans.items() if rg)
    res.update(batch=B, docs=len(bdocs), steps_per_epoch=len(groups), channels=args.channels, dtype=args.dtype,
               box_fed_first_conv=getattr(plan, "_owner_keep", None) is not None,
               boxes_faster_in_every_repeat=all(b < d for b, d in zip(res["boxes"]["ms_per_step"], res["dense"]["ms_per_step"])))
    return res


def run_eval(args, B):
    """evaluation of the documents: today's per-document loop against ragged confusion counts (same model, same documents)"""
    import numpy as np
    import torch
    from msau_amd.data.ragged import batches, pack
    dev = torch.device("cuda", 0)
    m = make_model(args).eval()
    docs = make_docs(args)
    C = m.n_class
    steps = []
    for idx in batches(docs, B, round_to=16):
        x, lab, sizes = pack([docs[i] for i in idx], round_to=16)
        steps.append((x.to(dev), lab, sizes))
    m.max_cached_plans = len(docs) + len({tuple(x.shape) for x, _, _ in steps}) + 2
    single = [(d["mask"].to(dev), d["label"]) for d in docs]

    def loop():
        labels, preds = [], []
        with torch.no_grad():
            for x, lab in single:
                lab = np.squeeze(lab.numpy())
                _, ypred, _ = m(x)
                idx = ypred.squeeze(0).argmax(0).cpu().numpy()
                labels.append(lab[lab != 0])
                preds.append(idx[lab != 0])
        cm = np.zeros((C, C), np.int64)
        np.add.at(cm, (np.hstack(labels), np.hstack(preds)), 1)
        return cm

    def ragged():
        cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
        for x, lab, sizes in steps:
            m.confusion_matrix(x, lab, sizes=sizes, out=cm)
        return cm.cpu().numpy()

    res = {}
    for name, fn in (("loop", loop), ("ragged", ragged)):
        fn()                                                 # plans built, first launches done
        torch.cuda.synchronize()
        times = []
        for _ in range(args.epochs):
            t0 = time.perf_counter()
            cm = fn()
            times.append(time.perf_counter() - t0)
        best = min(times)
        res[name] = {"docs_per_s": round(len(docs) / best, 1), "ms_per_doc": round(1e3 * best / len(docs), 3),
                     "acc": round(float(np.trace(cm)) / max(int(cm.sum()), 1), 6)}
    shapes = doc_shapes(args.docs)
    med = sorted(shapes, key=lambda s: s[0] * s[1])[len(shapes) // 2]
    p1 = m._plan_for_shape(1, med[0], med[1], dev, False)
    # + convert the input, export the logits, argmax, copy to the host
    res["loop"]["launches_per_forward"] = p1._fwd_seq[1] + 4
    x, _, _ = steps[len(steps) // 2]
    pr = m._plan_for_shape(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), dev, False, ragged=True)
    # + convert the input, zero it outside the documents, the counts
    res["ragged"].update(batch=B, forwards=len(steps), launches_per_forward=pr._fwd_seq[1] + 3,
                         median_canvas=[int(x.shape[0]), int(x.shape[2]), int(x.shape[3])])
    res["speedup"] = round(res["ragged"]["docs_per_s"] / res["loop"]["docs_per_s"], 3)
    return res


def run_entities(args, B):
    """entity-level predictions: the device route (forward-only plan + vote) against the host route (forward, export, numpy)"""
    import numpy as np
    import torch
    from msau_amd.data.entities import box_vote_host
    from msau_amd.data.ragged import batches, pack
    dev = torch.device("cuda", 0)
    m = make_model(args).eval()
    docs = make_docs(args)
    C = m.n_class
    rng = np.random.default_rng(1)
    steps = []
    for idx in batches(docs, B, round_to=16):
        x, _lab, sizes = pack([docs[i] for i in idx], round_to=16)
        boxes = []
        for b, (h, w) in enumerate(sizes.tolist()):
            for _ in range(max(4, h * w // 150)):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(-2, w - 4))
                boxes.append((b, y0, y0 + int(rng.integers(1, 4)), x0, x0 + int(rng.integers(6, 40)), int(rng.integers(1, C))))
        steps.append((x.to(dev), np.asarray(boxes, np.int32), sizes))
    m.max_cached_plans = len(steps) + 2
    n_boxes = sum(len(bx) for _, bx, _ in steps)

    def device(keep=None):
        em = torch.zeros((C, C), dtype=torch.int64, device=dev)
        for x, bx, sizes in steps:
            pred, _votes, _hist = m.box_predictions(x, bx, sizes=sizes, out=em)
            if keep is not None:
                keep.append(pred)
        return em.cpu().numpy()

    def host(keep=None):
        em = np.zeros((C, C), np.int64)
        with torch.no_grad():
            for x, bx, sizes in steps:
                _, logits, _ = m(x, sizes)
                pred, _votes, _hist, counts = box_vote_host(logits.permute(0, 2, 3, 1).cpu().numpy(), bx, C, extent=sizes.numpy())
                em += counts
                if keep is not None:
                    keep.append(pred)
        return em

    kd, kh = [], []
    em_d, em_h = device(kd), host(kh)                          # plans built, first launches done; the comparison of the routes
    torch.cuda.synchronize()
    same = bool(np.array_equal(em_d, em_h)) and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(kd, kh))
    res = {"device": {"docs_per_s": []}, "host": {"docs_per_s": []}}
    passes = max(args.epochs, 1)                               # epochs per timed window (--epochs 20: windows of 0.2 s and more)
    for _ in range(max(args.repeats, 5)):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            device()
        e1.record()
        torch.cuda.synchronize()
        res["device"]["docs_per_s"].append(round(passes * len(docs) / (1e-3 * e0.elapsed_time(e1)), 1))
        t0 = time.perf_counter()
        for _ in range(passes):
            host()
        res["host"]["docs_per_s"].append(round(passes * len(docs) / (time.perf_counter() - t0), 1))
    res["device"].update(clock="device events", bytes_to_host_per_doc=round(C * C * 8 / len(docs), 1))
    res["host"].update(clock="wall clock", bytes_to_host_per_doc=round(sum(x.shape[0] * C * x.shape[2] * x.shape[3] * 4 for x, _, _ in steps) / len(docs), 1))
    med = lambda v: sorted(v)[len(v) // 2]
    res.update(batch=B, docs=len(docs), forwards=len(steps), boxes=n_boxes, epochs_per_window=passes, dtype=args.dtype, channels=args.channels, same_predictions=same,
               entity_acc=round(float(np.trace(em_d)) / max(int(em_d.sum()), 1), 6),
               speedup_median=round(med(res["device"]["docs_per_s"]) / med(res["host"]["docs_per_s"]), 3),
               device_faster_in_every_repeat=all(d > h for d, h in zip(res["device"]["docs_per_s"], res["host"]["docs_per_s"])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=120)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--graph", action="store_true", help="also run with one HIP-graph replay per cached plan")
    ap.add_argument("--ragged", type=int, default=0, help="also run the documents in ragged batches of this size")
    ap.add_argument("--ragged-only", action="store_true", help="skip the batch-1 loop (e.g. under rocprofv3)")
    ap.add_argument("--eval", type=int, default=0, help="also compare the per-document evaluation loop with ragged batches of this size")
    ap.add_argument("--eval-only", action="store_true", help="only the evaluation comparison (e.g. under rocprofv3)")
    ap.add_argument("--boxes", action="store_true", help="with --ragged: ragged batches from box lists against the host-painted canvas (only this runs)")
    ap.add_argument("--repeats", type=int, default=5, help="--boxes / --entities: interleaved repeats (at least 5)")
    ap.add_argument("--entities", action="store_true", help="with --eval: entity-level predictions, device route against host route (only this runs)")
    ap.add_argument("--cost", choices=["cross_entropy", "focal", "dice"], default="cross_entropy",
                    help="the cost of the masked loss in the batch-1 and the ragged training loops (TrainEngine(cost=...))")
    args = ap.parse_args()
    if args.entities:
        if not args.eval:
            ap.error("--entities compares evaluation routes: give --eval B")
        print(json.dumps({"entities": run_entities(args, args.eval)}))
        return
    if args.boxes:
        if not args.ragged:
            ap.error("--boxes compares ragged batches: give --ragged B")
        print(json.dumps({"ragged_boxes": run_ragged_boxes(args, args.ragged)}))
        return
    if args.eval_only:
        print(json.dumps({"eval": run_eval(args, args.eval or 16)}))
        return
    if args.ragged_only:
        print(json.dumps({"ragged": run_ragged(args, args.ragged or 16)}))
        return
    out = {"eager": run(args, False)}
    if args.graph:
        out["graph"] = run(args, True)
        out["graph_speedup"] = round(out["graph"]["docs_per_s"] / out["eager"]["docs_per_s"], 3)
    if args.ragged:
        out["ragged"] = run_ragged(args, args.ragged)
        out["ragged_speedup"] = round(out["ragged"]["docs_per_s"] / out["eager"]["docs_per_s"], 3)
        if args.graph:
            out["ragged_graph"] = run_ragged(args, args.ragged, use_graph=True)
    if args.eval:
        out["eval"] = run_eval(args, args.eval)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
