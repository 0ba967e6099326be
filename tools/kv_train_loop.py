#!/usr/bin/env python3
"""Key-value training, two routes over the same documents (layout + OCR JSONs; default: the three golden layouts, repeated):

  tables   KVTrainBatches -> TrainEngine.step_kv at --batch-size: the training tables cross the bus, one launch paints the ids and both
           label canvases, ragged forward, UNetLoss kernel, backward, the optimiser (--optimizer adam: clip + Adam, the default;
           rmsprop / momentum, --weight-decay, --no-clip: msau_optim_step; `--optimizer rmsprop --no-clip --lr 1e-3` is the
           reference Trainer's optimiser) -- nothing per pixel on the host
  trainer  msau_amd.training.Trainer's route: one-hot input and one-hot targets built on the host and uploaded, autograd
           `UNetLoss`, the torch.optim counterpart of --optimizer (never clipped), batch 1

Prints for each route the documents per second of the WHOLE step (host work included), the bytes uploaded per document and
the loss trajectory, and one JSON line.  The two routes see the same jitter settings but not the same draws, and the optimisers
differ (the engine clips the gradient norm), so the trajectories are to be read side by side, not compared digit for digit.
--warp affine|rotate turns on the generator's augmentation (kwargs_dat affine_tr / rotate_tr): the tables route resamples the painted
canvases on the device (msau_kv_warp_train), the trainer route warps the one-hot planes x 255 with scipy.ndimage on the host, plane
by plane, as the generator does -- the comparison that `--warp` is about.  --warp elastic is the generator's elastic_tr
(`KVTrainBatches(..., imresize="pillow")`: the fields are drawn on the host with Pillow, msau_kv_elastic_train resamples; the trainer
route calls scipy's map_coordinates(order=1) per plane).  --time-launch adds, for the tables route under a --warp, the device time of
the warp launch alone on the last group (events around --steps calls, upload included) and the host time of a document's draw.
Not the headline metric (bench.py is); numbers are quoted in DESIGN.md 5e and profiles/kv_train.md.

--eval times VALIDATION instead (forward only, loss and accuracy per document), again two routes over the same deterministic tables
(`KVTrainBatches.validation()`, repeated to --eval-docs documents):

  eval_kv  MSAUWrapper.eval_kv at batch 1 and at --batch-size: tables up, painter, ragged forward fed with ids, msau_unet_eval; the
           rows stay on the device and are read once at the end (training.kv_trainer.summarize)
  trainer  what msau_amd.training.Trainer's validation loop does per document: one-hot input and targets built on the host, forward
           with fp32 NCHW export, `UNetLoss` (argmax + a host read for the accuracy, two CE launches), float() of the loss

Each route is timed --repeats times, the routes alternating inside one process; the table gives the median and the spread of the
documents per second (host work included, the window ends in a device synchronise) and the epoch figures of both routes, which
must agree.  The markdown table goes to --out (profiles/kv_eval.md)."""
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
    kwargs_dat = {"affine": {"affine_tr": True}, "rotate": {"rotate_tr": True}, "elastic": {"elastic_tr": True}}.get(args.warp, {})
    return KVTrainBatches(args.layouts, args.charset, args.n_class, batch_size, args.scale_min, args.scale_max, args.text_err,
                          shuffle=True, seed=args.seed, kwargs_dat=kwargs_dat, imresize="pillow" if args.warp == "elastic" else None)


def scipy_warp(t, maps):
    """the generator's host route for a table's warp: the one-hot maps [h, w, c] x 255 as uint8, every plane through scipy's cubic
    spline, thresholded at > 64; the targets made one-hot again (1 first, then the smallest set class, else 0)"""
    from scipy import ndimage
    from msau_amd.training.kv_warp import Elastic, _label_of, elastic_coords
    if isinstance(t.warp, Elastic):                                         # (order 1, at the elastic warp's coordinates)
        coords = elastic_coords(t.warp)
        warp_plane = lambda plane: ndimage.map_coordinates(plane, coords, order=1)
    else:
        warp_plane = lambda plane: ndimage.affine_transform(plane, t.warp.matrix, offset=t.warp.offset, output_shape=t.warp.out_shape)
    out = []
    for k, m in enumerate(maps):
        planes = m * np.uint8(255)
        res = np.stack([warp_plane(planes[:, :, d]) for d in range(planes.shape[2])], axis=2) > 64
        out.append(res.astype("B") if k == 0 else np.eye(m.shape[2], dtype="B")[_label_of(res)])
    return out


def cost_of(args):
    """--cost / --gamma / --smooth as the `cost` of TrainEngine.step_kv / MSAUWrapper.eval_kv and as UNetLoss's kwargs (the trainer
    routes); None for the cross entropy"""
    return {"cross_entropy": None, "focal": {"cost_name": "focal", "gamma": args.gamma}, "dice": {"cost_name": "dice", "smooth": args.smooth}}[args.cost]


def run_tables(args):
    it = batches(args, args.batch_size)
    eng = TrainEngine(model(it.n_token, args.n_class, args.dtype), lr=args.lr, optimizer=args.optimizer, weight_decay=args.weight_decay,
                      max_norm=None if args.no_clip else 1.0)
    print("optimiser launches:", ", ".join(f"{key} ({nbytes} B)" for key, nbytes in eng.optim_launches()))
    cw = [float(v) for v in args.class_weights.split(",")] if args.class_weights else None
    cost = cost_of(args)
    for _ in range(args.warmup):
        eng.step_kv(next(it), class_weights=cw, round_to=args.round_to, cost=cost)
    torch.cuda.synchronize()
    kv_data.STATS.update(calls=0, documents=0, host_painted=0, h2d_bytes=0, host_warped=0)
    losses = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(eng.step_kv(next(it), class_weights=cw, round_to=args.round_to, cost=cost).clone())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    docs = args.steps * args.batch_size
    extra = time_launch(args, eng, it) if args.time_launch and args.warp else {}
    return dict(**extra, route="tables", cost=args.cost, batch_size=args.batch_size, optimizer=args.optimizer, clip=not args.no_clip, weight_decay=args.weight_decay,
                optim_launches=[key for key, _ in eng.optim_launches()], docs_per_s=docs / dt,
                h2d_bytes_per_doc=kv_data.STATS["h2d_bytes"] / docs,
                host_painted=kv_data.STATS["host_painted"], host_warped=kv_data.STATS["host_warped"], warp=args.warp, loss=[round(float(l[0]), 5) for l in torch.stack(losses).cpu()])


def time_launch(args, eng, it):
    """the warp launch of one group alone, as step_kv issues it (upload of its records, the tiles, the flags): device events around
    --steps calls; and the host time of a document's warp draw"""
    from msau_amd.training import kv_warp
    tables = next(it)
    t0 = time.perf_counter()
    for t in tables:
        it._augment(t)
    draw_ms = (time.perf_counter() - t0) * 1e3 / len(tables)
    elastic = args.warp == "elastic"
    ident, launch = (kv_warp.identity_elastic, kv_warp.elastic_train_device) if elastic else (kv_warp.identity_warp, kv_warp.warp_train_device)
    warps = [ident(t.shape) if t.warp is None else t.warp for t in tables]
    ids, labels, aux, sizes = kv_data.paint_train_device(tables, round_to=args.round_to, device=eng.model._flat.device)
    wsizes, (Ho, Wo) = kv_warp.warped_canvas(warps, round_to=args.round_to)
    grid = eng.input_nhwc(len(tables), Ho, Wo)
    m = eng.model
    dtype = m._plan_for_shape(len(tables), Ho, Wo, grid.device, True).dtype
    go = lambda: launch(ids, labels, aux, sizes, warps, grid, m.channels, m.n_class, dtype)
    for _ in range(3):
        go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.steps):
        go()
    b.record()
    torch.cuda.synchronize()
    return dict(warp_launch_ms=a.elapsed_time(b) / args.steps, warp_canvas=[len(tables), int(ids.shape[1]), int(ids.shape[2]), Ho, Wo],
                warp_pixels=int(wsizes.prod(axis=1).sum()), warp_draw_ms_per_doc=draw_ms)


def run_trainer(args):
    it = batches(args, 1)
    net = model(it.n_token, args.n_class, args.dtype)
    crit = UNetLoss(cost_of(args) or {})
    opt = {"adam": lambda ps: torch.optim.Adam(ps, lr=args.lr, weight_decay=args.weight_decay),
           "rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=args.lr, weight_decay=args.weight_decay),
           "momentum": lambda ps: torch.optim.SGD(ps, lr=args.lr, momentum=0.9, weight_decay=args.weight_decay)}[args.optimizer](net.parameters())
    eye_in, eye_out = np.eye(it.n_token, dtype="B"), np.eye(args.n_class, dtype="B")

    def step():
        (t,) = next(it)
        ids, lab, aux = kv_data.paint_train_host(t) if t.ok else kv_data.paint_train_painter(t)
        maps = [e[m] for e, m in ((eye_in, ids), (eye_out, lab), (eye_out, aux))]
        if t.warp is not None:
            maps = scipy_warp(t, maps)
        maps = [np.ascontiguousarray(m.transpose(2, 0, 1))[None] for m in maps]
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
    return dict(route="trainer", cost=args.cost, batch_size=1, warp=args.warp, docs_per_s=docs / dt, h2d_bytes_per_doc=nbytes / docs,
                loss=[round(float(l), 5) for l in torch.stack(losses).cpu()][::max(1, args.batch_size)])


def eval_tables(args, it):
    groups = it.validation()
    docs = [t for g in groups for t in g]
    return [docs[i % len(docs)] for i in range(args.eval_docs)]


def run_eval_kv(args, net, docs, batch_size):
    from msau_amd.training.kv_trainer import summarize
    groups = [docs[i:i + batch_size] for i in range(0, len(docs), batch_size)]
    for g in groups[:args.warmup] + groups[-1:]:                          # every canvas of the timed window (the last may be smaller)
        net.eval_kv(g, round_to=args.round_to, cost=cost_of(args))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = [net.eval_kv(g, round_to=args.round_to, cost=cost_of(args)) for g in groups]
    s = summarize(torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]))      # the one read: ends the window
    return len(docs) / (time.perf_counter() - t0), s


def run_eval_trainer(args, net, docs, n_token):
    crit = UNetLoss(cost_of(args) or {})
    eye_in, eye_out = np.eye(n_token, dtype="B"), np.eye(args.n_class, dtype="B")

    def one(t):
        ids, lab, aux = kv_data.paint_train_host(t) if t.ok else kv_data.paint_train_painter(t)
        maps = [np.ascontiguousarray(e[m].transpose(2, 0, 1))[None] for e, m in ((eye_in, ids), (eye_out, lab), (eye_out, aux))]
        bx, bt, ba = (torch.from_numpy(m) for m in maps)
        bx, bt, ba = bx.float().cuda(), bt.long().cuda(), ba.long().cuda()
        with torch.no_grad():
            _, logits, logits_aux = net(bx)
            acc, loss, final = crit(logits, bt, {"aux_logits": logits_aux, "aux_tgt": ba})
        return acc, float(loss), float(final)

    for t in docs[:max(args.warmup, 3)]:
        one(t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = [one(t) for t in docs]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    acc, loss, final = (float(np.mean([r[i] for r in res])) for i in range(3))
    return len(docs) / dt, dict(loss=loss, final=final, acc=acc, documents=len(docs))


def run_eval(args):
    if not torch.cuda.is_available():
        raise SystemExit("kv_train_loop --eval measures on an MI355X; no GPU is visible (nothing was measured)")
    it = batches(args, args.batch_size)
    net = model(it.n_token, args.n_class, args.dtype)
    docs = eval_tables(args, it)
    routes = [("eval_kv", 1), ("eval_kv", args.batch_size), ("trainer", 1)]
    rates = {r: [] for r in routes}
    figures = {}
    for _ in range(args.repeats):                                         # alternating: a drift of the machine hits every route
        for r in routes:
            rate, s = run_eval_kv(args, net, docs, r[1]) if r[0] == "eval_kv" else run_eval_trainer(args, net, docs, it.n_token)
            rates[r].append(rate)
            figures[r] = s
    lines = [f"`tools/kv_train_loop.py --eval --dtype {args.dtype} --eval-docs {args.eval_docs} --repeats {args.repeats}` on "
             f"{torch.cuda.get_device_name(0)}: validation documents per second, host work included, median of {args.repeats} "
             f"(min .. max), the routes alternating in one process; canvases of the golden layouts at scale 3.", "",
             "| route | batch | documents/s | loss | final | acc |", "|---|---|---|---|---|---|"]
    out = []
    for r in routes:
        v, s = sorted(rates[r]), figures[r]
        med = float(np.median(v))
        lines.append(f"| {r[0]} | {r[1]} | {med:.1f} ({v[0]:.1f} .. {v[-1]:.1f}) | {s['loss']:.6f} | {s['final']:.6f} | {s['acc']:.6f} |")
        out.append(dict(route=r[0], batch_size=r[1], docs_per_s=med, docs_per_s_min=v[0], docs_per_s_max=v[-1], loss=s["loss"],
                        final=s["final"], acc=s["acc"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps(dict(mode="eval", cost=args.cost, dtype=args.dtype, eval_docs=args.eval_docs, repeats=args.repeats, results=out)))


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
    ap.add_argument("--optimizer", default="adam", choices=["adam", "rmsprop", "momentum"], help="the engine's optimiser (tables route) "
                    "and its torch.optim counterpart (trainer route)")
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--no-clip", action="store_true", help="tables route: no global-norm clip (the reference's Trainer never clips)")
    ap.add_argument("--scale-min", type=float, default=2.0)
    ap.add_argument("--scale-max", type=float, default=4.0)
    ap.add_argument("--text-err", type=float, default=0.1)
    ap.add_argument("--class-weights", default="", help="comma-separated, n_class values (tables route)")
    ap.add_argument("--cost", default="cross_entropy", choices=["cross_entropy", "focal", "dice"], help="the loss of every route, training and --eval")
    ap.add_argument("--gamma", type=float, default=2.0, help="--cost focal")
    ap.add_argument("--smooth", type=float, default=1.0, help="--cost dice")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warp", default="", choices=["", "affine", "rotate", "elastic"], help="the generator's augmentation: on the device in the "
                    "tables route, scipy.ndimage on the host in the trainer route")
    ap.add_argument("--time-launch", action="store_true", help="tables route with --warp: also time the warp launch alone and the draw")
    ap.add_argument("--round-to", type=int, default=32, help="canvas sizes are rounded up to a multiple (fewer distinct plans)")
    ap.add_argument("--routes", default="tables,trainer")
    ap.add_argument("--eval", action="store_true", help="time validation (eval_kv against the Trainer's route) instead of training")
    ap.add_argument("--eval-docs", type=int, default=96, help="--eval: documents per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="--eval: timed windows per route")
    ap.add_argument("--out", default="", help="--eval: write the markdown table here")
    args = ap.parse_args()
    if args.eval:
        run_eval(args)
        return
    out = []
    for route in args.routes.split(","):
        r = run_tables(args) if route == "tables" else run_trainer(args)
        out.append(r)
        print(f"{r['route']:8s} batch {r['batch_size']:3d}: {r['docs_per_s']:9.1f} documents/s (whole step)  "
              f"{r['h2d_bytes_per_doc']:12.0f} bytes uploaded per document")
        print(f"{'':8s} loss: {r['loss']}")
        if "warp_launch_ms" in r:
            print(f"{'':8s} warp launch alone: {r['warp_launch_ms']:.3f} ms (B, H, W, Ho, Wo = {r['warp_canvas']}, {r['warp_pixels']} pixels inside); "
                  f"draw on the host: {r['warp_draw_ms_per_doc']:.3f} ms per document; step: {1e3 * r['batch_size'] / r['docs_per_s']:.2f} ms")
    print(json.dumps(dict(dtype=args.dtype, steps=args.steps, results=out)))


if __name__ == "__main__":
    main()
