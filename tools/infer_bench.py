#!/usr/bin/env python3
"""Forward-only throughput of the inference path: MSAUWrapper.predict_nhwc at the bench size and at
the size KVModel really runs at (text lines scaled to 3 px), dense input vs the device-painted id mask.
With --ragged B: ms per document of predict_nhwc(ids) one document at a time against ragged batches of B (pack_ids +
predict_nhwc(ids=..., sizes=...)) on id masks of varied sizes around KVModel's 70 x 128 scale (60 tokens, 17 classes).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ragged", type=int, default=0, help="only the ragged comparison, in batches of this size")
    ap.add_argument("--docs", type=int, default=48, help="documents of the ragged comparison")
    a = ap.parse_args()
    if a.ragged:
        for dtype in ("bf16", "fp32"):
            print(json.dumps(run_ragged(a.ragged, a.docs, dtype, max(1, a.iters // 10), 1)), flush=True)
        return
    for cfg in ((16, 64, 336, 256, 5, "bf16"), (1, 64, 336, 256, 5, "bf16"), (1, 60, 70, 128, 17, "bf16"), (1, 60, 70, 128, 17, "fp32")):
        for use_ids, graph in ((False, False), (True, False), (True, True)):
            print(json.dumps(run(*cfg, use_ids, a.iters, a.warmup, graph)), flush=True)


if __name__ == "__main__":
    main()
