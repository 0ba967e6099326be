#!/usr/bin/env python3
"""FUNSD chargrid training entry point on MI355X -- counterpart of the reference script of the same name
(reference: train_chargrid_funsd_msau.py:16-118 train, :121-163 evaluate, :175-258 main).

Same flow and defaults: pickles written by funsd_preprocessing_word_level.py -> per-document chargrids
(batch 1, variable H x W) -> MSAU(featRoot 8, 4 scales, res_depth 2, softmax) -> Adam(lr 1e-4) with global-norm
clip 1.0 -> accuracy / micro precision / recall over labelled pixels after every epoch -> state_dict saved
every 10 epochs under ckpt/<dataset>_<method>_h<hidden>_o<out>/<epoch>.pth.tar.

--batch-size N trains ragged batches (msau_amd.data.ragged: each document computes what it would alone, the loss is the mean of
the documents' losses); --eval-batch-size N evaluates in ragged batches.  The evaluation counts a confusion matrix on the device
(MSAUWrapper.confusion_matrix) and prints sklearn's classification report for the test split, as the reference does.
--entity-level adds the entity-level figures: every annotated entity box gets the class most of its pixels predict
(MSAUWrapper.box_predictions, counted on the device as well) and a second accuracy / report is printed over entities.

--cost {cross_entropy,focal,dice} (--gamma, --smooth) and --class-weights w0,w1,... train the masked loss under the focal or the
soft Dice cost and with class weights; the epoch print then carries the validation loss under the same cost
(MSAUWrapper.eval_loss, on the device).  The defaults are the reference's masked cross entropy.

Two step implementations, selected with --loop:
  engine     (default) msau_amd.TrainEngine: fused masked-CE + clip + Adam, no per-step host sync
  reference  model(V) -> model.loss -> loss.backward() -> clip_grad_norm_ -> optimizer.step(), line for line
"""
import argparse
import json
import os
import random
import time

import numpy as np
import torch

from msau_amd import MSAUWrapper as MSAU
from msau_amd import TrainEngine
from msau_amd.data import FUNSDCharGridDataLoaderBoxMaskBoxLabel
from msau_amd.data import ragged, raster
from msau_amd.training import metrics, save_checkpoint


def ckpt_filename(save_dir, args, epoch=-1, isbest=False):
    """utils/io_utils.py:37-80: <dataset>_<method>_h<hidden>_o<out>/[best|<epoch>].pth.tar (epoch 0 -> no number)"""
    d = os.path.join(save_dir, f"{args.bmname or args.dataset}_{args.method}_h{args.hidden_dim}_o{args.output_dim}")
    os.makedirs(d, exist_ok=True)
    if isbest:
        d = os.path.join(d, "best")
    elif epoch > 0:
        d = os.path.join(d, str(epoch))
    return d + ".pth.tar"


def eval_count(n_docs, max_num_examples=None):
    """how many documents, from the start of the dataset, `evaluate` looks at: the reference stops after the batch for which
    `(batch_idx + 1) * batch_size > max_num_examples` (train_chargrid_funsd_msau.py:144-146) and evaluates at batch 1, so the
    first max_num_examples + 1 -- whatever batch size the evaluation runs at here"""
    return n_docs if max_num_examples is None else min(n_docs, max_num_examples + 1)


def canvases(docs, batch_size, round_to=16):
    """the (B, H, W) inputs a pass over `docs` feeds the model: the documents' own shapes at batch 1, else the ragged canvases of
    msau_amd.data.ragged.batches + pack (every one is a plan)"""
    if batch_size == 1:
        return {(1,) + tuple(d["mask"].shape[2:]) for d in docs}
    out = set()
    for idx in ragged.batches(docs, batch_size, round_to):
        hw = [tuple(docs[i]["mask"].shape[2:]) for i in idx]
        out.add((len(idx), -(-max(h for h, _ in hw) // round_to) * round_to, -(-max(w for _, w in hw) // round_to) * round_to))
    return out


def evaluate(dataset, model, args, name="Validation", testing=False, max_num_examples=None, labels_map=None, batch_size=None):
    """accuracy over the labelled pixels (reference :121-163) from a confusion matrix that the device accumulates
    (MSAUWrapper.confusion_matrix): no logits leave the device and the host reads the matrix once.  batch_size (default
    --eval-batch-size) > 1 runs the documents in ragged batches.  The test split also prints the classification report.
    With args.entity_level every document brings its entity boxes ("boxes", int32 [m, 6]); a second matrix counts (entity label,
    class most of the entity's pixels predict) on the device (MSAUWrapper.box_predictions, a forward of its own; whole boxes vote,
    same `zero_as`), and the entity accuracy and report are printed after the per-pixel ones and returned as "entity_acc" /
    "entity_matrix"."""
    model.eval()
    device = model.flat_parameters.device
    bs = batch_size if batch_size is not None else getattr(args, "eval_batch_size", 1)
    docs = dataset[:eval_count(len(dataset), max_num_examples)]
    zero_as = labels_map["other"] if testing and labels_map is not None and "other" in labels_map else None   # reference :140
    cm = torch.zeros((model.n_class, model.n_class), dtype=torch.int64, device=device)
    entities = getattr(args, "entity_level", False)           # documents then carry "boxes": their entity boxes [m, 6]
    em = torch.zeros_like(cm) if entities else None
    with torch.no_grad():
        if bs == 1:
            for data in docs:
                x = data["mask"].float().to(device)
                model.confusion_matrix(x, data["label"].long(), zero_as=zero_as, out=cm)
                if entities:
                    model.box_predictions(x, data["boxes"], zero_as=zero_as, out=em)
        else:
            for idx in ragged.batches(docs, bs):
                x, lab, sizes = ragged.pack([docs[i] for i in idx])
                x = x.to(device)
                model.confusion_matrix(x, lab, sizes=sizes, zero_as=zero_as, out=cm)
                if entities:
                    none = np.zeros((0, 6), np.int32)
                    _, boxes, _, _, _ = ragged.pack_boxes([(none, docs[i]["boxes"]) + tuple(docs[i]["mask"].shape[2:]) for i in idx])
                    model.box_predictions(x, boxes, sizes=sizes, zero_as=zero_as, out=em)
    cm = cm.cpu().numpy()
    result = metrics.scores(cm)
    print(name, " accuracy:", result["acc"])
    names = list(labels_map.keys()) if labels_map is not None else None
    if testing:
        print(metrics.classification_report(cm, names))
    if entities:
        em = em.cpu().numpy()
        result = dict(result, entity_acc=metrics.scores(em)["acc"], entity_matrix=em)
        print(name, " entity accuracy:", result["entity_acc"])
        print(metrics.classification_report(em, names))
    return result


def cost_of(args):
    """-> (cost, class_weights) as TrainEngine / MSAUWrapper.loss / eval_loss take them, from --cost / --gamma / --smooth / --class-weights"""
    name = getattr(args, "cost", "cross_entropy")
    cost = {"cost_name": "focal", "gamma": args.gamma} if name == "focal" else {"cost_name": "dice", "smooth": args.smooth} if name == "dice" else None
    return cost, getattr(args, "class_weights", None)


def validation_loss(dataset, model, args, batch_size=None):
    """the mean over the documents of the loss that is trained (final + auxiliary head, under --cost and --class-weights), forward
    only and summed on the device (MSAUWrapper.eval_loss): the host reads one number"""
    model.eval()
    device = model.flat_parameters.device
    cost, cw = cost_of(args)
    bs = batch_size if batch_size is not None else getattr(args, "eval_batch_size", 1)
    total = torch.zeros((), device=device)
    if bs == 1:
        for data in dataset:
            total += model.eval_loss(data["mask"].float().to(device), data["label"].long().to(device), cost=cost, class_weights=cw)[0].sum()
    else:
        for idx in ragged.batches(dataset, bs):
            x, lab, sizes = ragged.pack([dataset[i] for i in idx])
            total += model.eval_loss(x.to(device), lab.to(device), sizes, cost=cost, class_weights=cw)[0].sum()
    return float(total) / max(len(dataset), 1)


def train(dataset, model, args, val_dataset=None, test_dataset=None, labels_map=None):
    device = model.flat_parameters.device
    cost, class_weights = cost_of(args)
    if args.loop == "engine":
        engine = TrainEngine(model, lr=args.lr, max_norm=float(args.clip), cost=cost, class_weights=class_weights)
        optimizer = None
    else:
        optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=args.lr)
    best_val = {"epoch": 0, "loss": 0, "acc": 0}
    val_accs = []
    bs = getattr(args, "batch_size", 1)
    for epoch in range(args.num_epochs):
        t0 = time.time()
        model.train()
        avg_loss = torch.zeros((), device=device)
        print("Epoch: ", epoch)
        # batch 1: one document per step; --batch-size N: ragged batches of documents of similar size
        steps = ([i] for i in range(len(dataset))) if bs == 1 else ragged.batches(dataset, bs)
        for batch_idx, idx in enumerate(steps):
            if bs == 1:
                data = dataset[idx[0]]
                V = data["mask"].float().to(device)
                label = data["label"].long().to(device)
                sizes = None
            else:
                x, lab, sizes = ragged.pack([dataset[i] for i in idx])
                V, label = x.to(device), lab.to(device)
            if args.loop == "engine":
                loss = engine.step(V, label, sizes).reshape(())
            else:
                model.zero_grad()
                _, ypred, ypred_aux = model(V, sizes)
                loss = model.loss(ypred, ypred_aux, label, cost=cost, class_weights=class_weights)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), float(args.clip))
                optimizer.step()
            if batch_idx % 10 == 0:
                print("Batch {} optimized. Loss: {}".format(batch_idx, float(loss)))
            # the step's loss is the mean of its documents' losses: weight it by their number
            avg_loss += loss.detach() if bs == 1 else loss.detach() * len(idx)
        avg_loss = float(avg_loss) / max(len(dataset), 1)
        print("Avg loss: ", avg_loss, "; epoch time: ", time.time() - t0)
        evaluate(dataset, model, args, name="Train", max_num_examples=100)
        if val_dataset:
            vr = evaluate(val_dataset, model, args, name="Validation")
            print("Validation  loss:", validation_loss(val_dataset, model, args))
            val_accs.append(vr["acc"])
            if vr["acc"] > best_val["acc"] - 1e-7:
                best_val = {"acc": vr["acc"], "epoch": epoch, "loss": avg_loss}
        if test_dataset:
            tr = evaluate(test_dataset, model, args, testing=True, name="Test", labels_map=labels_map)
            print("Test result: ", dict({k: v for k, v in tr.items() if k != "entity_matrix"}, epoch=epoch))
        print("Best val result: ", best_val)
        if epoch % 10 == 0:
            torch.save(model.state_dict(), ckpt_filename(args.ckptdir, args, epoch))
    # final dict checkpoint with the reference's keys (utils/io_utils.py:83-105, called at train_...py:116)
    save_checkpoint(model, engine if args.loop == "engine" else optimizer, args, num_epochs=-1)
    return model, val_accs


def parse_args(argv=None):
    """the command line (None: sys.argv) and the fixed settings of the reference's run (train_chargrid_funsd_msau.py:175-200)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-pickle", default="./funsd_preprocess.pkl")
    ap.add_argument("--test-pickle", default="./funsd_preprocess_test.pkl")
    ap.add_argument("--num-epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--clip", type=float, default=1.0)          # the reference passes args.clip = True == 1.0
    ap.add_argument("--train-ratio", type=float, default=0.8)
    ap.add_argument("--ckptdir", default="ckpt")
    ap.add_argument("--model-kwargs-path", default=None)
    ap.add_argument("--loop", choices=["engine", "reference"], default="engine")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    ap.add_argument("--batch-size", type=int, default=1,
                    help="documents per training step; > 1 trains ragged batches of documents of similar size")
    ap.add_argument("--eval-batch-size", type=int, default=1, help="documents per evaluation forward (ragged batches when > 1)")
    ap.add_argument("--entity-level", action="store_true",
                    help="also report accuracy / precision / recall over the annotated entity boxes (each box votes with its pixels)")
    ap.add_argument("--cost", choices=["cross_entropy", "focal", "dice"], default="cross_entropy",
                    help="the masked loss's cost: the reference's cross entropy, the focal loss (--gamma) or the soft Dice loss (--smooth)")
    ap.add_argument("--gamma", type=float, default=2.0, help="focal: the exponent of (1 - p_t), >= 0")
    ap.add_argument("--smooth", type=float, default=1.0, help="dice: the smoothing term, > 0")
    ap.add_argument("--class-weights", default=None, help="w0,w1,...: one weight per class (class 0 = unlabelled first)")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.eval_batch_size < 1:
        ap.error("--batch-size and --eval-batch-size must be >= 1")
    if args.class_weights is not None:
        try:
            args.class_weights = [float(w) for w in args.class_weights.split(",")]
        except ValueError:
            ap.error("--class-weights: numbers separated by commas")
    args.bmname, args.hidden_dim, args.dataset, args.method = None, 500, "invoice", "GCN"
    return args


def main(argv=None):
    args = parse_args(argv)
    random.seed(777)
    data_loader = FUNSDCharGridDataLoaderBoxMaskBoxLabel(args.train_pickle)
    data_loader_test = FUNSDCharGridDataLoaderBoxMaskBoxLabel(args.test_pickle, data_loader.labels)
    args.output_dim = len(data_loader.labels) + 1
    os.makedirs(args.ckptdir, exist_ok=True)
    feature_dim = data_loader[0]["mask"].shape[1]
    if args.model_kwargs_path is None:
        model_kwargs = dict(model="msau", final_act="softmax", featRoot=8, scale_space_num=4, res_depth=2,
                            n_class=args.output_dim, img_channels=feature_dim, use_auxiliary_loss=False)
        with open("model_kwargs.json", "w") as fh:
            json.dump(model_kwargs, fh)
    else:
        with open(args.model_kwargs_path) as fh:
            model_kwargs = json.load(fh)
    model = MSAU(feature_dim, args.output_dim, model_kwargs=dict(model_kwargs, dtype=args.dtype)).cuda()
    indices = list(range(len(data_loader)))
    random.shuffle(indices)
    cut = int(len(indices) * args.train_ratio)

    def instance(loader, i):
        """the loader's item; with --entity-level also the document's entity boxes (the boxes its label mask is painted from)"""
        return dict(loader[i], boxes=raster.document_boxes(loader.inp_list[i])[1]) if args.entity_level else loader[i]

    train_instances = [instance(data_loader, i) for i in indices[:cut]]
    val_instances = [instance(data_loader, i) for i in indices[cut:]]
    test_instances = [instance(data_loader_test, i) for i in range(len(data_loader_test))]
    print("Num training instances: ", len(train_instances), "; Num validation instances: ", len(val_instances),
          "; Num testing instances: ", len(test_instances))
    # batch 1 with a different H x W per document (data_generator_funsd_bert.py:216-222): every shape has its own static
    # plan (buffers + launch list); ragged batches have one per canvas.  Keep them all -- the training plans and the forward-only
    # plans of the evaluation passes, bounded by model.max_plan_bytes -- instead of rebuilding a plan on every step of every epoch.
    shapes = {tuple(d["mask"].shape[2:]) for d in train_instances + val_instances + test_instances}
    evaluated = train_instances[:eval_count(len(train_instances), 100)]
    n_plans = len(canvases(train_instances, args.batch_size)) + \
        len(set().union(*(canvases(d, args.eval_batch_size) for d in (evaluated, val_instances, test_instances) if d)))
    model.max_cached_plans = max(model.max_cached_plans, 2 * len(shapes), n_plans)
    print("Distinct document shapes: ", len(shapes))
    train(train_instances, model, args, val_dataset=val_instances, test_dataset=test_instances,
          labels_map=data_loader.labels)
    print("Finished\n\n")


if __name__ == "__main__":
    main()
