#!/usr/bin/env python3
"""Time the launches of the masked loss by direct ABI calls (profiles/masked_cost.md): today's msau_label_counts_split +
msau_masked_ce_multi against msau_masked_cost at the cross entropy, the focal and the soft Dice cost, with and without class weights
(with msau_label_hist where the call needs it), at the headline shape -- B = 16 on 336 x 256, 5 classes at 8 stored channels, both
heads, bf16 and fp32.

    python tools/masked_cost_bench.py [--windows 7] [--calls 100] [--dice-k 16 32 64] > masked_cost.json

Device events around `--calls` back-to-back calls after 5 warm-up calls; `--windows` such windows per variant, the variants
alternating inside one process; per variant the median and the range over its windows, in us per call.  One JSON line."""
import argparse
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from msau_amd import _lib as L
from msau_amd.plan_loss import cost_hist_k


def variants(dtype, B, H, W, C, dice_ks, dev):
    """-> {name: callable issuing the variant's launches on the current stream}"""
    td, dt = (torch.float32, L.F32) if dtype == "fp32" else (torch.bfloat16, L.BF16)
    Cs = -(-C // 8) * 8
    g = torch.Generator().manual_seed(1)
    lg = [(torch.randn(B, H, W, Cs, generator=g) * 2).to(td).to(dev) for _ in range(2)]
    d = [torch.empty_like(x) for x in lg]
    occ = torch.rand(B, H, W, generator=g) < 0.3                               # bench.py's labels: 30 % occupancy
    lab = (torch.randint(1, C, (B, H, W), generator=g) * occ.long()).to(dev)
    cw = (torch.rand(C, generator=g) + 0.5).to(dev)
    lib = L.load()
    s = lambda: torch.cuda.current_stream().cuda_stream
    Kc = cost_hist_k(B, False)                                                 # also LossSite.counts_k at this B
    counts = torch.zeros(B * Kc, dtype=torch.int32, device=dev)
    loss = torch.zeros(3, device=dev)
    ws_multi = torch.zeros(int(lib.msau_ce_multi_ws_floats(B * H * W)), device=dev)
    ws = {k: torch.zeros(int(lib.msau_masked_cost_ws_floats(k, B, H, W, C)), device=dev) for k in (L.COST_CE, L.COST_FOCAL, L.COST_DICE)}
    hist = torch.zeros((B, 64, C), dtype=torch.int32, device=dev)

    def default():
        L.call("msau_label_counts_split", s(), lab.data_ptr(), counts.data_ptr(), B, H * W, Kc, key="msau_label_counts")
        L.call("msau_masked_ce_multi", s(), dt, lg[0].data_ptr(), lg[1].data_ptr(), lab.data_ptr(), counts.data_ptr(), d[0].data_ptr(),
               d[1].data_ptr(), loss.data_ptr(), ws_multi.data_ptr(), B, H * W, C, Cs, 1.0 / B, Kc)

    def cost(kind, param, weighted, K):
        def run():
            h = None
            if weighted or kind == L.COST_DICE:
                L.call("msau_label_hist", s(), lab.data_ptr(), None, hist.data_ptr(), B, H, W, C, K)
                h = hist.data_ptr()
            L.call("msau_masked_cost", s(), dt, kind, param, lg[0].data_ptr(), lg[1].data_ptr(), lab.data_ptr(), None,
                   cw.data_ptr() if weighted else None, h, K, d[0].data_ptr(), d[1].data_ptr(), loss.data_ptr(), ws[kind].data_ptr(),
                   B, H, W, C, Cs)
        return run

    out = {"default: label_counts + masked_ce_multi": default,
           "masked_cost ce": cost(L.COST_CE, 0.0, False, Kc), "masked_cost ce, weights": cost(L.COST_CE, 0.0, True, Kc),
           "masked_cost focal 2": cost(L.COST_FOCAL, 2.0, False, Kc), "masked_cost focal 2, weights": cost(L.COST_FOCAL, 2.0, True, Kc)}
    for K in dice_ks:
        out[f"masked_cost dice, K = {K}"] = cost(L.COST_DICE, 1.0, False, K)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--dice-k", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=336)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--n-class", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masked_cost_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = {"shape": [args.batch, args.height, args.width, args.n_class], "calls": args.calls, "windows": args.windows, "us_per_call": {}}
    for dtype in ("bf16", "fp32"):
        runs = variants(dtype, args.batch, args.height, args.width, args.n_class, args.dice_k, dev)
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in runs}
        for _ in range(args.windows):
            for name, fn in runs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    fn()
                b.record()
                b.synchronize()
                times[name].append(1e3 * a.elapsed_time(b) / args.calls)
        res["us_per_call"][dtype] = {name: {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
                                     for name, t in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
