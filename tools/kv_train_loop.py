#!/usr/bin/env python3
"""Key-value training, two routes over the same documents (layout + OCR JSONs; default: the three golden layouts, repeated):

  tables   KVTrainBatches -> TrainEngine.step_kv at --batch-size: the training tables cross the bus, one launch paints the ids and both
           label canvases, ragged forward, UNetLoss kernel, backward, clip + Adam -- nothing per pixel on the host
  trainer  msau_amd.training.Trainer's route: one-hot input and one-hot targets built on the host and uploaded, autograd
           `UNetLoss`, torch.optim.Adam, batch 1

Prints for each route the documents per second of the WHOLE step (host work included), the bytes uploaded per document and
the loss trajectory, and one JSON line.  The two routes see the same jitter settings but not the same draws, and the optimisers
differ (the engine clips the gradient norm), so the trajectories are to be read side by side, not compared digit for digit.
Not the headline metric (bench.py is); numbers are quoted in DESIGN.md 5e and profiles/kv_train.md."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.training import KVTrainBatches, UNetLoss
from msau_amd.training import kv_data

KV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "kv")


def model(n_token, n_class, dtype):
    return MSAUWrapper(n_token, n_class, dict(featRoot=8, scale_space_num=4, res_depth=2, filter_size=3, pool_size=2,
                                              final_act="softmax", num_blocks=3, dtype=dtype, seed=0)).cuda()


def batches(args, batch_size):
    return KVTrainBatches(args.layouts, args.charset, args.n_class, batch_size, args.scale_min, args.scale_max, args.text_err,
                          shuffle=True, seed=args.seed)


def run_tables(args):
    it = batches(args, args.batch_size)
    eng = TrainEngine(model(it.n_token, args.n_class, args.dtype), lr=args.lr)
    cw = [float(v) for v in args.class_weights.split(",")] if args.class_weights else None
    for _ in range(args.warmup):
        eng.step_kv(next(it), class_weights=cw, round_to=args.round_to)
    torch.cuda.synchronize()
    kv_data.STATS.update(calls=0, documents=0, host_painted=0, h2d_bytes=0)
    losses = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(eng.step_kv(next(it), class_weights=cw, round_to=args.round_to).clone())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    docs = args.steps * args.batch_size
    return dict(route="tables", batch_size=args.batch_size, docs_per_s=docs / dt, h2d_bytes_per_doc=kv_data.STATS["h2d_bytes"] / docs,
                host_painted=kv_data.STATS["host_painted"], loss=[round(float(l[0]), 5) for l in torch.stack(losses).cpu()])


def run_trainer(args):
    it = batches(args, 1)
    net = model(it.n_token, args.n_class, args.dtype)
    crit = UNetLoss({})
    opt = torch.optim.Adam(net.parameters(), lr=args.lr)
    eye_in, eye_out = np.eye(it.n_token, dtype="B"), np.eye(args.n_class, dtype="B")

    def step():
        (t,) = next(it)
        ids, lab, aux = kv_data.paint_train_host(t) if t.ok else kv_data.paint_train_painter(t)
        maps = [np.ascontiguousarray(e[m].transpose(2, 0, 1))[None] for e, m in ((eye_in, ids), (eye_out, lab), (eye_out, aux))]
        bx, bt, ba = (torch.from_numpy(m) for m in maps)
        nbytes = bx.numel() * 4 + (bt.numel() + ba.numel()) * 8                 # as Trainer._batch uploads them: float, long, long
        bx, bt, ba = bx.float().cuda(), bt.long().cuda(), ba.long().cuda()
        opt.zero_grad()
        _, logits, logits_aux = net(bx)
        _acc, loss, _final = crit(logits, bt, {"aux_logits": logits_aux, "aux_tgt": ba})
        loss.backward()
        opt.step()
        return loss.detach(), nbytes

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    losses, nbytes = [], 0
    docs = args.steps * args.batch_size
    t0 = time.perf_counter()
    for _ in range(docs):
        l, n = step()
        losses.append(l)
        nbytes += n
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(route="trainer", batch_size=1, docs_per_s=docs / dt, h2d_bytes_per_doc=nbytes / docs,
                loss=[round(float(l), 5) for l in torch.stack(losses).cpu()][::max(1, args.batch_size)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("layouts", nargs="*", default=[os.path.join(KV, f"layout{i}.json") for i in range(3)])
    ap.add_argument("--charset", default=os.path.join(KV, "charset.txt"))
    ap.add_argument("--n-class", type=int, default=17)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--scale-min", type=float, default=2.0)
    ap.add_argument("--scale-max", type=float, default=4.0)
    ap.add_argument("--text-err", type=float, default=0.1)
    ap.add_argument("--class-weights", default="", help="comma-separated, n_class values (tables route)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--round-to", type=int, default=32, help="canvas sizes are rounded up to a multiple (fewer distinct plans)")
    ap.add_argument("--routes", default="tables,trainer")
    args = ap.parse_args()
    out = []
    for route in args.routes.split(","):
        r = run_tables(args) if route == "tables" else run_trainer(args)
        out.append(r)
        print(f"{r['route']:8s} batch {r['batch_size']:3d}: {r['docs_per_s']:9.1f} documents/s (whole step)  "
              f"{r['h2d_bytes_per_doc']:12.0f} bytes uploaded per document")
        print(f"{'':8s} loss: {r['loss']}")
    print(json.dumps(dict(dtype=args.dtype, steps=args.steps, results=out)))


if __name__ == "__main__":
    main()
