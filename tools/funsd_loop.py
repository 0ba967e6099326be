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

    python tools/funsd_loop.py [--docs 120] [--epochs 3] [--channels 64] [--dtype bf16] [--graph] [--ragged 16] [--eval 16]
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


def run(args, use_graph):
    import torch
    from msau_amd import TrainEngine
    dev = torch.device("cuda", 0)
    m = make_model(args)
    shapes = doc_shapes(args.docs)
    m.max_cached_plans = 2 * len(shapes) + 2
    eng = TrainEngine(m, lr=1e-4, use_graph=use_graph)
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
    eng = TrainEngine(m, lr=1e-4, use_graph=use_graph)
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
    args = ap.parse_args()
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
