"""GPU: training-side parity that round 1 left thin (VERDICT r1 "what's weak" 1, "next" 3 and 7):
  * bf16 (the benchmarked storage type): every parameter gradient against the reference's fixtures, a 20-step loss
    trajectory against fp32 storage, and a per-parameter comparison at the bench size so that the bf16-only kernel
    instances (16x32 tiles, two-output data gradients, channel-split, strided / upsampling) are each hit;
  * `UNetLoss` against values the reference's own model/training/cost.py produced;
  * a checkpoint written by the reference's utils.io_utils.save_checkpoint, loaded and resumed;
  * plan-cache / graph-cache / saved-activation hazards."""
import ast
import os

import numpy as np
import pytest
import torch

from msau_amd.model import MSAUWrapper, TrainEngine
from tests.golden_util import GOLDEN, err, load_net_case, rel_err, rel_l2, summarize

pytestmark = pytest.mark.gpu


def _model(cfg, sd, dtype, **extra):
    kw = dict(scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"], featRoot=cfg["featRoot"],
              filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax",
              num_blocks=cfg["num_blocks"], dtype=dtype, activation_name=cfg.get("activation", "relu"), **extra)
    m = MSAUWrapper(cfg["channels"], cfg["n_class"], kw)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _param_grads(m, eng):
    return {k: eng.flat_grad[m._poff[k]:m._poff[k] + p.numel()].view(p.shape) for k, p in m.named_parameters()}


# ---- (a) bf16 gradients of every parameter against the reference's fixtures ------------------------------------------
# Tolerances (stated, bf16 storage / fp32 accumulate, ~60 sequential convs): the reference fixture holds each gradient's
# L2 norm and 64 strided samples.  Per tensor: norm within NORM_TOL of the reference's, samples within SAMPLE_TOL in
# relative L2 (plus a floor of FLOOR x the largest gradient norm, for tensors whose gradient is rounding noise);
# whole network: global norm within 3e-2.
BF16_NORM_TOL, BF16_SAMPLE_TOL, BF16_FLOOR = 1e-1, 1.5e-1, 2e-3


@pytest.mark.parametrize("name", ["net_cfg2_336x256x64", "net_f4_c13_b2_64x48", "net_elu_f8_c13_33x26"])
def test_bf16_parameter_gradients_match_reference(name):
    g, cfg, sd, x, label = load_net_case(name)
    m = _model(cfg, sd, "bf16")
    eng = TrainEngine(m, lr=1e-4)
    loss = eng.step(x.cuda(), label.cuda())
    torch.cuda.synchronize()
    assert abs(float(loss) - float(g["loss"])) < 3e-2 * abs(float(g["loss"]))
    assert abs(float(eng.grad_norm) - float(g["grad_norm"])) < 3e-2 * float(g["grad_norm"])
    grads = _param_grads(m, eng)
    names = [str(s) for s in g["param_names"]]
    dead = set(str(s) for s in g["dead_params"])
    gmax = max(float(s[0]) for s in g["grad_summary"])
    worst = (0.0, 0.0)
    for i, k in enumerate(names):
        if k in dead:
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        s, smp = summarize(grads[k])
        ref_n, ref_smp = float(g["grad_summary"][i][0]), np.asarray(g["grad_samples"][i], np.float64)
        dn = abs(s[0] - ref_n)
        ds = float(np.linalg.norm(smp - ref_smp))
        floor = BF16_FLOOR * gmax
        assert dn <= BF16_NORM_TOL * ref_n + floor, (k, s[0], ref_n)
        assert ds <= BF16_SAMPLE_TOL * float(np.linalg.norm(ref_smp)) + floor * np.sqrt(len(smp) / max(grads[k].numel(), 1)) + \
            1e-3 * float(np.abs(ref_smp).max()), (k, ds, float(np.linalg.norm(ref_smp)))
        worst = (max(worst[0], dn / (ref_n + floor)), max(worst[1], ds / (float(np.linalg.norm(ref_smp)) + floor)))
    print(f"{name}: worst per-tensor norm deviation {worst[0]:.3e}, worst sample rel-L2 {worst[1]:.3e}")


# ---- (b) 20 steps, fp32 vs bf16 storage, same weights, same batch ------------------------------------------------------
def test_bf16_loss_trajectory_tracks_fp32_over_20_steps():
    g, cfg, sd, x, label = load_net_case("net_f4_c13_b2_64x48")
    traj = {}
    for dtype in ("fp32", "bf16"):
        m = _model(cfg, sd, dtype)
        eng = TrainEngine(m, lr=1e-3)
        losses = [eng.step(x.cuda(), label.cuda()).clone() for _ in range(20)]
        torch.cuda.synchronize()
        traj[dtype] = np.array([float(l) for l in losses])
    f, b = traj["fp32"], traj["bf16"]
    assert abs(f[0] - float(g["loss"])) < 1e-4 * float(g["loss"])
    assert f[-1] < 0.9 * f[0], f                                       # it trains
    gap = np.abs(f - b) / f
    print("fp32", np.round(f, 4), "\nbf16", np.round(b, 4), "\nmax rel gap", gap.max())
    assert gap.max() < 1e-2, (f, b)                                    # stated tolerance: 1e-2 of the loss at every step (observed 1.5e-3)


# ---- (c) bench size: every parameter gradient, bf16 storage vs the fp32-storage engine -----------------------------------
def test_bench_size_bf16_gradients_track_fp32_storage_per_parameter():
    """B=16, 336x256x64, 3 stages: the workload bench.py times.  This is the only size at which the 16x32-tile (WGW=2),
    two-output (DOUT), channel-split (SPLIT) and strided / upsampling bf16 instances are all selected."""
    from oracle import msau_oracle as O
    from msau_amd.plan import ConvOp
    x, label = O.synthetic_batch(16, 64, 336, 256, 5, seed=3)
    x, label = x.cuda(), label.cuda()
    res = {}
    for dtype in ("fp32", "bf16"):
        kw = dict(scale_space_num=4, res_depth=2, featRoot=8, final_act="softmax", num_blocks=3, dtype=dtype, seed=0)
        m = MSAUWrapper(64, 5, kw).cuda()
        eng = TrainEngine(m)
        loss = eng.step(x, label)
        torch.cuda.synchronize()
        if dtype == "bf16":
            plan = m._plan_for(x, True)
            keys = {op.fkey for op in plan.ops if isinstance(op, ConvOp)} | \
                   {dm[0] for op in plan.ops if isinstance(op, ConvOp) for dm in op.dmeta if dm is not None}
            for want in ("dout", "ups2", "s2", "dual"):
                assert any(want in k for k in keys), (want, sorted(keys))
        res[dtype] = (float(loss), float(eng.grad_norm), {k: v.clone() for k, v in _param_grads(m, eng).items()})
        del eng, m
        torch.cuda.empty_cache()
    (lf, nf, gf), (lb, nb, gb) = res["fp32"], res["bf16"]
    assert abs(lf - lb) < 2e-2 * lf and abs(nf - nb) < 3e-2 * nf, (lf, lb, nf, nb)
    gmax = max(float(v.norm()) for v in gf.values())
    worst = 0.0
    for k, ref in gf.items():
        if float(ref.abs().max()) == 0.0:
            assert float(gb[k].abs().max()) == 0.0, k
            continue
        e = float((gb[k] - ref).norm()) / (float(ref.norm()) + 2e-3 * gmax)
        worst = max(worst, e)
        assert e < 1e-1, (k, e)                                        # stated tolerance: rel-L2 1e-1 per tensor
    print("bench-size bf16 vs fp32 storage: worst per-parameter rel-L2", worst)


# ---- N3: UNetLoss against the reference's own values -----------------------------------------------------------------------
def test_unet_loss_matches_reference_fixture():
    """model/training/cost.py:35-65 run by oracle/gen_goldens.py::train_goldens -> (acc, loss, final, gradients)"""
    from msau_amd.training import UNetLoss
    g = np.load(os.path.join(GOLDEN, "train", "unet_loss.npz"))
    crit = UNetLoss({})
    for tag in ("a", "b", "c"):
        lg = torch.from_numpy(g[f"{tag}.logits"]).cuda().requires_grad_(True)
        lab = torch.from_numpy(g[f"{tag}.label"]).cuda()
        C = lg.shape[1]
        tgt = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).float()
        with_aux = f"{tag}.aux" in g.files
        ax = torch.from_numpy(g[f"{tag}.aux"]).cuda().requires_grad_(True) if with_aux else None
        acc, loss, final = crit(lg, tgt, {"aux_logits": ax, "aux_tgt": tgt} if with_aux else {})
        loss.backward()
        assert abs(acc - float(g[f"{tag}.acc"])) < 1e-6, tag
        assert abs(float(loss) - float(g[f"{tag}.loss"])) < 1e-5 * abs(float(g[f"{tag}.loss"])), tag
        if with_aux:
            assert abs(float(final) - float(g[f"{tag}.final"])) < 1e-5 * abs(float(g[f"{tag}.final"])), tag
            assert rel_err(ax.grad.cpu(), g[f"{tag}.gaux"]) < 1e-5, tag
        else:
            assert final is None and np.isnan(g[f"{tag}.final"])
        assert rel_err(lg.grad.cpu(), g[f"{tag}.glogits"]) < 1e-5, tag


def test_unet_loss_with_class_weights_matches_reference_fixture():
    """`UNetLoss({"class_weights": ...})` = torch.nn.CrossEntropyLoss(weight) (model/training/cost.py:24-31) against values the
    reference's own class produced (oracle/gen_goldens.py::weighted_loss_goldens): 5 and 17 classes with auxiliary logits, 4 classes
    without, one class of weight zero.  `msau_softmax_ce_weighted`: un-normalised gradient + both sums in one pass."""
    from msau_amd.training import UNetLoss
    g = np.load(os.path.join(GOLDEN, "train", "unet_loss_weighted.npz"))
    for tag in ("a", "b", "c"):
        crit = UNetLoss({"class_weights": [float(v) for v in g[f"{tag}.class_weights"]]}).cuda()
        lg = torch.from_numpy(g[f"{tag}.logits"]).cuda().requires_grad_(True)
        lab = torch.from_numpy(g[f"{tag}.label"]).cuda()
        C = lg.shape[1]
        tgt = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).float()
        with_aux = f"{tag}.aux" in g.files
        ax = torch.from_numpy(g[f"{tag}.aux"]).cuda().requires_grad_(True) if with_aux else None
        acc, loss, final = crit(lg, tgt, {"aux_logits": ax, "aux_tgt": tgt} if with_aux else {})
        loss.backward()
        assert abs(acc - float(g[f"{tag}.acc"])) < 1e-6, tag
        assert abs(float(loss) - float(g[f"{tag}.loss"])) < 1e-5 * abs(float(g[f"{tag}.loss"])), tag
        if with_aux:
            assert abs(float(final) - float(g[f"{tag}.final"])) < 1e-5 * abs(float(g[f"{tag}.final"])), tag
            assert rel_err(ax.grad.cpu(), g[f"{tag}.gaux"]) < 1e-5, tag
        else:
            assert final is None and np.isnan(g[f"{tag}.final"])
        assert rel_err(lg.grad.cpu(), g[f"{tag}.glogits"]) < 1e-5, tag
    # uniform weights are the plain loss
    gp = np.load(os.path.join(GOLDEN, "train", "unet_loss.npz"))
    lg = torch.from_numpy(gp["c.logits"]).cuda()
    tgt = torch.nn.functional.one_hot(torch.from_numpy(gp["c.label"]).cuda(), lg.shape[1]).permute(0, 3, 1, 2).float()
    _, lw, _ = UNetLoss({"class_weights": [3.0] * lg.shape[1]}).cuda()(lg, tgt, {})
    assert abs(float(lw) - float(gp["c.loss"])) < 1e-5 * abs(float(gp["c.loss"]))


# ---- N3: a checkpoint the reference wrote --------------------------------------------------------------------------------------
def test_reference_checkpoint_resumes_on_the_engine(tmp_path):
    """utils.io_utils.save_checkpoint's file (after one clip + Adam step of the reference): the HIP network reproduces the
    reference's post-step logits, TrainEngine takes over the Adam moments, and our own checkpoint round-trips."""
    import types
    from msau_amd.training import load_checkpoint, save_checkpoint
    gdir = os.path.join(GOLDEN, "train")
    meta = np.load(os.path.join(gdir, "ref_checkpoint_meta.npz"), allow_pickle=True)
    cfg = ast.literal_eval(str(meta["cfg"]))
    m = MSAUWrapper(cfg["channels"], cfg["n_class"], dict(scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                                                         featRoot=cfg["featRoot"], final_act="softmax", dtype="fp32")).cuda()
    eng = TrainEngine(m, lr=3e-3)
    ck = load_checkpoint(os.path.join(gdir, "ref_checkpoint.pth.tar"), model=m, optimizer=eng, trusted=True)
    x = torch.from_numpy(meta["x"]).cuda()
    with torch.no_grad():
        _, logits, aux = m(x)
    assert rel_err(logits.cpu(), meta["logits_after"]) < 2e-4 and rel_err(aux.cpu(), meta["aux_after"]) < 2e-4
    # Adam state: per-parameter moments by registration order, step count, hyper-parameters of the reference's optimizer
    assert eng.lr == 1e-4 and float(eng.state[0]) == 1.0
    st = ck["optimizer_state"]
    live = [(k, p) for k, p in m._named]
    order = [pid for grp in st["param_groups"] for pid in grp["params"]]
    assert len(order) == len(live)
    n_seen = 0
    for pid, (k, p) in zip(order, live):
        off, n = m._poff[k], p.numel()
        if pid in st["state"]:
            assert torch.equal(eng.m[off:off + n].cpu(), st["state"][pid]["exp_avg"].reshape(-1).cpu()), k
            assert torch.equal(eng.v[off:off + n].cpu(), st["state"][pid]["exp_avg_sq"].reshape(-1).cpu()), k
            n_seen += 1
        else:
            assert k in m._dead and float(eng.m[off:off + n].abs().max()) == 0.0, k
    assert n_seen == len(live) - len(m._dead)
    # our writer: same keys, resumable
    lab = (torch.rand(1, x.shape[2], x.shape[3], device="cuda") * cfg["n_class"]).long()
    eng.step(x, lab)
    args = types.SimpleNamespace(ckptdir=str(tmp_path), bmname=None, dataset="funsd", method="msau", hidden_dim=20, output_dim=20)
    path = save_checkpoint(m, eng, args, num_epochs=8)
    m2 = MSAUWrapper(cfg["channels"], cfg["n_class"], dict(scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                                                          featRoot=cfg["featRoot"], final_act="softmax", dtype="fp32")).cuda()
    eng2 = TrainEngine(m2)
    ck2 = load_checkpoint(path, model=m2, optimizer=eng2)
    assert set(ck2) == set(ck) and ck2["epoch"] == 8
    assert torch.equal(m2.flat_parameters, m.flat_parameters) and torch.equal(eng2.m, eng.m) and torch.equal(eng2.v, eng.v)
    assert float(eng2.state[0]) == 2.0 and eng2.lr == eng.lr
    l1, l2 = eng.step(x, lab), eng2.step(x, lab)
    torch.cuda.synchronize()
    assert float(l1) == float(l2) and torch.equal(m2.flat_parameters, m.flat_parameters)


# ---- stale graphs, plan thrash, overwritten saved activations --------------------------------------------------------
def test_train_graphs_die_with_their_plan():
    """use_graph=True with more shapes than the plan cache holds: returning to an evicted shape must rebuild plan AND
    graph (round 1 kept the graph keyed by shape and replayed it into freed buffers)."""
    from oracle import msau_oracle as O
    g, cfg, sd, x, label = load_net_case("net_f4_c13_b2_64x48")
    shapes = [(24, 40), (33, 31), (17, 48), (40, 24), (25, 25), (24, 40)]
    res = {}
    for use_graph in (False, True):
        m = _model(cfg, sd, "fp32", deterministic=True)
        m.max_cached_plans = 2
        eng = TrainEngine(m, use_graph=use_graph)
        out = []
        for (H, W) in shapes:
            xs, ls = O.synthetic_batch(2, cfg["channels"], H, W, cfg["n_class"], H * 100 + W)
            out.append(float(eng.step(xs.cuda(), ls.cuda())))
        torch.cuda.synchronize()
        assert len(m._plans) <= 2
        res[use_graph] = (out, m.flat_parameters.clone())
    assert res[False][0] == res[True][0], res
    assert torch.equal(res[False][1], res[True][1])


# ---- graphs keyed by id(engine), hyper-parameters frozen into the captured optimiser step -------------------------
def test_train_graphs_belong_to_one_engine_and_follow_its_hyper_parameters():
    """(1) a second TrainEngine for the same model never replays the first one's graphs, even when CPython hands it the
    dead engine's id(): engines file their graphs under a counter, and a freed engine's entries are dropped;
    (2) load_state_dict / set_hyper after a graph step re-capture the optimiser graph (lr, betas, eps, max_norm are by-value
    kernel arguments): the graph engine keeps matching an eager engine through a change of lr and a state reload."""
    g, cfg, sd, x, label = load_net_case("net_f4_c13_b2_64x48")
    x, label = x.cuda(), label.cuda()
    m = _model(cfg, sd, "fp32", deterministic=True)
    e1 = TrainEngine(m, lr=1e-3, use_graph=True)
    e1.step(x, label)
    plan = m._plan_for(x, True)
    tok1 = e1._token
    assert tok1 in plan._tgraphs
    del e1
    import gc
    gc.collect()
    assert tok1 not in plan._tgraphs                      # a dead engine leaves nothing to replay
    e2 = TrainEngine(m, lr=1e-5, use_graph=True)
    assert e2._token != tok1
    res = {}
    for use_graph in (False, True):
        mm = _model(cfg, sd, "fp32", deterministic=True)
        eng = TrainEngine(mm, lr=1e-3, use_graph=use_graph)
        losses = [float(eng.step(x, label)) for _ in range(2)]
        eng.set_hyper(lr=1e-5)
        losses += [float(eng.step(x, label)) for _ in range(2)]
        st = eng.state_dict()
        st["lr"] = 3e-4
        eng.load_state_dict(st)
        losses += [float(eng.step(x, label)) for _ in range(2)]
        torch.cuda.synchronize()
        res[use_graph] = (losses, mm.flat_parameters.clone())
    assert res[False][0] == res[True][0], res
    assert torch.equal(res[False][1], res[True][1])


def test_backward_after_a_second_forward_of_the_same_shape_raises():
    g, cfg, sd, x, label = load_net_case("net_f8_c13_33x26")
    m = _model(cfg, sd, "fp32")
    xa, xb = x.cuda(), (x * 0.5).cuda()
    _, la, aa = m(xa)
    _, lb, ab = m(xb)                                    # overwrites the activations the first backward would read
    loss_a = m.loss(la, aa, label.cuda())
    with pytest.raises(RuntimeError, match="overwritten"):
        loss_a.backward()
    m.zero_grad()
    m.loss(lb, ab, label.cuda()).backward()              # the latest forward is fine
    assert all(p.grad is not None for k, p in m.named_parameters() if k not in m._dead)


def test_plan_cache_is_bounded_by_bytes_as_well_as_count():
    g, cfg, sd, x, label = load_net_case("net_f4_c13_b2_64x48")
    m = _model(cfg, sd, "fp32")
    m.max_cached_plans = 64
    with torch.no_grad():
        m(x.cuda())
        one = sum(p.activation_bytes() for p in m._plans.values())
        m.max_plan_bytes = int(2.5 * one)
        for k in range(1, 6):
            m(x[:, :, :64 - k, :].contiguous().cuda())
    assert 1 <= len(m._plans) <= 3 and sum(p.activation_bytes() for p in m._plans.values()) <= m.max_plan_bytes


# ---- N1: dense (BERT) painter on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_dense_rasteriser_matches_the_reference_bertgrids(dtype, tmp_path):
    """msau_raster_dense + msau_raster_labels against tests/golden/funsd/bertgrid.npz DIRECTLY: the grids and label maps the
    reference's own loader (`get_box_mask_box_label`, data_generator_funsd_bert.py:64-93,240) painted from the same documents and
    per-line feature vectors -- both splits, bit exact in the storage type -- and against the product's CPU painter."""
    import json, pickle
    from msau_amd.data import funsd as F
    from msau_amd.data.raster import document_line_boxes, rasterize_dense
    G = os.path.join(GOLDEN, "funsd")
    g = np.load(os.path.join(G, "bertgrid.npz"), allow_pickle=True)
    train, inv = F.get_preprocessed_list_word_msau(os.path.join(G, "train"))
    test, _ = F.get_preprocessed_list_word_msau(os.path.join(G, "test"), inv_dict_charset=inv)
    checked = 0
    for split, docs in (("train", train), ("test", test)):
        docs.sort(key=lambda d: d["file_path"])
        for di, d in enumerate(docs):
            d["transformer_feature"] = g[f"{split}{di}.feats"]
        with open(tmp_path / f"{split}.pkl", "wb") as fh:
            pickle.dump(docs, fh)
        ds = F.FUNSDBertDataLoaderBoxMaskBoxLabel(str(tmp_path / f"{split}.pkl"), json.loads(str(g["labels_json"])), write_labels_file=False)
        for i in range(len(ds)):
            it = ds[i]
            fb, lb, H, W = document_line_boxes(ds.inp_list[i])
            feats = np.asarray(ds.inp_list[i]["transformer_feature"], np.float32)
            grid, labels = rasterize_dense(fb, lb, feats, 1, H, W, dtype)
            C = feats.shape[1]
            gold = torch.from_numpy(np.ascontiguousarray(g[f"{split}{i}.mask"]))[0].permute(1, 2, 0)    # the reference's array, [H,W,C]
            assert tuple(gold.shape) == (H, W, C), (split, i)
            for want in (gold, it["mask"][0].permute(1, 2, 0)):
                if dtype == "bf16":
                    want = want.to(torch.bfloat16)
                assert torch.equal(grid[0, :, :, :C].float().cpu(), want.float()), (split, i)   # bit exact in the storage type
            assert float(grid[0, :, :, C:].abs().max()) == 0.0 if grid.shape[3] > C else True
            assert np.array_equal(labels[0].cpu().numpy(), g[f"{split}{i}.label"][0].astype(np.int64)), (split, i)
            assert torch.equal(labels[0].cpu(), it["label"][0].long()), (split, i)
            checked += 1
    assert checked >= 2


def test_graphs_of_a_dead_engine_are_not_destroyed_inside_somebody_elses_capture():
    """A stream capture is global: a device synchronisation (or hipGraphDestroy) from a finaliser that happens to run while
    another engine captures aborts the process at hipStreamEndCapture (seen once in four full runs of this suite).  Dropped
    graphs are parked while a capture section is open and destroyed at the next safe point."""
    import weakref
    from msau_amd import model as M
    g, cfg, sd, x, label = load_net_case("net_f4_c13_b2_64x48")
    x, label = x.cuda(), label.cuda()
    m = _model(cfg, sd, "fp32", deterministic=True)
    eng = TrainEngine(m, lr=1e-3, use_graph=True)
    eng.step(x, label)
    plan = m._plan_for(x, True)
    tok = eng._token
    assert tok in plan._tgraphs and not M._graveyard
    with M._capture_section():                              # as if another engine were in the middle of torch.cuda.graph(...)
        TrainEngine._drop_graphs(weakref.ref(m), tok)      # what the dead engine's finaliser does
        assert tok not in plan._tgraphs and len(M._graveyard) == 1
    M._bury_graphs()
    assert not M._graveyard
    eng2 = TrainEngine(m, lr=1e-3, use_graph=True)          # and capturing goes on working
    assert np.isfinite(float(eng2.step(x, label)))


@pytest.mark.parametrize("dtype,dense", [("fp32", True), ("bf16", True), ("bf16", False)])
def test_training_from_box_lists_equals_the_step_on_the_painted_tensor(dtype, dense, monkeypatch):
    """TrainEngine.step_boxes / step_nhwc (N1; data_generator_funsd_bert.py:64-93,240): the box lists are painted on the device
    straight into the plan's NHWC input buffer -- no fp32 NCHW tensor, no boundary conversion -- against TrainEngine.step on
    the same grid handed over as the reference does (float [B,C,H,W]): every bit of loss, gradient and updated parameters.
    dense: 24-d feature vectors per line box (the BERT painter); else one-hot character ids."""
    from msau_amd.data.raster import rasterize, rasterize_dense
    monkeypatch.setenv("MSAU_OWNER_CONV", "0")             # the PAINTED path (the box-list-fed first conv has its own test below)
    torch.manual_seed(3)
    B, H, W, C, ncls = 3, 40, 56, 24, 5
    rng = np.random.default_rng(11)
    boxes, labs = [], []
    for b in range(B):
        for i in range(14):
            y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 6))
            y1, x1 = y0 + int(rng.integers(1, 6)), x0 + int(rng.integers(2, 12))       # some reach over the edge: clipped
            boxes.append((b, y0, y1, x0, x1, len(boxes) if dense else int(rng.integers(0, C))))
            labs.append((b, y0, y1, x0, x1, int(rng.integers(1, ncls))))
    boxes, labs = np.asarray(boxes, np.int32), np.asarray(labs, np.int32)
    feats = rng.standard_normal((len(boxes), C)).astype(np.float32) if dense else None
    kw = dict(scale_space_num=3, res_depth=2, featRoot=8, final_act="softmax", num_blocks=2, dtype=dtype, seed=4, deterministic=True)
    res = {}
    for mode in ("boxes", "tensor"):
        m = MSAUWrapper(C, ncls, kw).cuda()
        eng = TrainEngine(m)
        if mode == "boxes":
            losses = [float(eng.step_boxes(boxes, labs, B, H, W, feats=feats)) for _ in range(2)]
            # the grid was painted into the plan's own buffer: same storage
            assert eng.input_nhwc(B, H, W).data_ptr() == m._plan_for_shape(B, H, W, torch.device("cuda", 0), True).x_in.data.data_ptr()
        else:
            if dense:
                grid, labels = rasterize_dense(boxes, labs, feats, B, H, W, dtype)
            else:
                grid, labels = rasterize(boxes, labs, B, H, W, C, dtype)
            x = grid[..., :C].float().permute(0, 3, 1, 2).contiguous()      # what a host-side loader would hand over
            losses = [float(eng.step(x, labels)) for _ in range(2)]
            # ... and a foreign NHWC tensor (one device copy) is the same step again
            m2 = MSAUWrapper(C, ncls, kw).cuda()
            e2 = TrainEngine(m2)
            l2 = [float(e2.step_nhwc(grid, labels)) for _ in range(2)]
            assert l2 == losses and torch.equal(m2.flat_parameters, m.flat_parameters)
        torch.cuda.synchronize()
        res[mode] = (losses, eng.flat_grad.clone(), m.flat_parameters.clone())
    assert res["boxes"][0] == res["tensor"][0]
    assert torch.equal(res["boxes"][1], res["tensor"][1]) and torch.equal(res["boxes"][2], res["tensor"][2])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_from_id_masks_equals_dense_one_hot_input(dtype):
    """TrainEngine.step_ids (N1: only the character-id mask crosses the boundary; the one-hot grid is synthesised in LDS by
    the first conv and its weight gradient -- bf16 -- or painted on the device -- fp32)
    against TrainEngine.step on the dense float tensor of the same ids: every bit of loss, gradients and updated
    parameters.  Includes ids outside the charset (painted as empty pixels, like unknown characters in the reference's
    `transform_from_charset`, funsd_preprocessing_word_level.py:50-57)."""
    g, cfg, sd, x, label = load_net_case("net_cfg2_336x256x64")
    C = cfg["channels"]
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(-1, C + 2, (2, 336, 256), generator=gen, dtype=torch.int32)      # -1, C, C+1: empty
    ids[torch.rand(ids.shape, generator=gen) < 0.6] = -1
    valid = (ids >= 0) & (ids < C)
    dense = torch.zeros(2, C, 336, 256)
    dense.scatter_(1, ids.clamp(0, C - 1).long()[:, None], valid[:, None].float())
    lab = torch.randint(1, cfg["n_class"], ids.shape, generator=gen) * valid.long()
    res = []
    for feed in ("dense", "ids"):
        m = _model(cfg, sd, dtype, deterministic=True)
        eng = TrainEngine(m)
        for _ in range(2):
            loss = eng.step(dense.cuda(), lab.cuda()) if feed == "dense" else eng.step_ids(ids.cuda(), lab.cuda())
        torch.cuda.synchronize()
        res.append((float(loss), eng.flat_grad.clone(), m.flat_parameters.clone()))
        if feed == "ids":
            # bf16: the first conv and its weight gradient read the id mask directly (MSAU_CONV_IDS, one-hot tile synthesised
            # in LDS); fp32 storage has no id-mask weight-gradient instance and paints the dense input
            plan = next(iter(m._plans.values()))
            assert (plan._ids_conv is not None) == (dtype == "bf16")
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_train_step_is_bit_reproducible_beside_the_side_stream():
    """Regression for the round-1 "one-ulp finding": with the weight gradients running on the side stream, 25-40 % of fresh
    processes (about 3 % of warm steps) returned a level-0 LRN backward that differed in a few 16-lane groups.  Root cause:
    packed-fp32 instruction chains (v_pk_add_f32 with op_sel) in lrn_fast_kernel under concurrent load; elementwise.hip is
    now built without them (msau_amd/build.py).  40 cold steps from the same weights on the same batch must agree bit for
    bit -- in the default mode, no `deterministic` flag, overlap on."""
    g, cfg, sd, x, label = load_net_case("net_cfg2_336x256x64")
    xb, lb = x.cuda().repeat(4, 1, 1, 1).contiguous(), label.cuda().repeat(4, 1, 1).contiguous()
    m = _model(cfg, sd, "bf16")
    flat0 = m.flat_parameters.clone()
    ref = None
    for it in range(40):
        m.flat_parameters.copy_(flat0)
        eng = TrainEngine(m)
        loss = eng.step(xb, lb)
        torch.cuda.synchronize()
        cur = (float(loss), eng.flat_grad.clone())
        if ref is None:
            ref = cur
        else:
            assert cur[0] == ref[0] and torch.equal(cur[1], ref[1]), f"step {it} differs from step 0"


def test_profiled_step_runs_the_records_of_the_step():
    """A step under `L.Profiler()` enqueues the very msau_op arrays of the step, one record per call: with `overlap_wgrad=False`
    (both steps then go through msau_run_ops on one stream: the same launches in the same order) loss, gradient and updated
    parameters are bit-identical to the unprofiled step's, and the profiler's keys and counts are those of `plan.launch_meta`.
    A profiled step with the default `overlap_wgrad` (one stream too, while it is being timed) leaves the same keys and counts."""
    from msau_amd import _lib as L
    g, cfg, sd, x, label = load_net_case("net_f8_c13_33x26")
    assert cfg["num_blocks"] == 3
    xb, lb = x.cuda(), label.cuda()

    def step(profiled, **extra):
        m = _model(cfg, sd, "bf16", **extra)
        eng = TrainEngine(m)
        plan = m._plan_for(xb, True)                 # built, and its lazily resolved input feed settled, outside the profiled
        plan._feed_ids(None)                         # region: their host-side queries of the library are no launches
        prof = L.Profiler() if profiled else None
        L.set_profiler(prof)
        try:
            loss = eng.step(xb, lb)
        finally:
            L.set_profiler(None)
        torch.cuda.synchronize()
        counts = {k: n for k, (n, _) in prof.summary().items()} if profiled else None
        assert m._plan_for(xb, True) is plan
        meta = {k: n for k, (n, _, _) in plan.launch_meta.items()}
        return (float(loss), eng.flat_grad.clone(), m.flat_parameters.clone()), counts, meta

    plain, _, _ = step(False, overlap_wgrad=False)
    prof, counts, meta = step(True, overlap_wgrad=False)
    assert plain[0] == prof[0] and torch.equal(plain[1], prof[1]) and torch.equal(plain[2], prof[2])
    assert float(plain[1].abs().max()) > 0.0
    print("profiled:", counts, "\nlaunch_meta:", meta)
    assert counts == meta, {k: (counts.get(k), meta.get(k)) for k in set(counts) | set(meta) if counts.get(k) != meta.get(k)}
    _, counts2, meta2 = step(True)
    assert counts2 == meta2 == counts, {k: (counts2.get(k), meta2.get(k)) for k in set(counts2) | set(meta2) if counts2.get(k) != meta2.get(k)}


@pytest.mark.parametrize("dense", [True, False])
def test_prefetched_box_batches_train_exactly_like_step_boxes(dense, monkeypatch):
    """TrainEngine.prefetch_boxes / step_prefetched: the next batch is painted into the plan's SECOND input buffer on the side
    stream while the current step runs.  A sequence of DIFFERENT batches (so a stale or swapped buffer would show) must give
    the losses, gradients and parameters of the same batches through step_boxes, bit for bit."""
    monkeypatch.setenv("MSAU_OWNER_CONV", "0")             # both sides PAINT the grid (step_boxes would otherwise feed the box lists)
    torch.manual_seed(3)
    B, H, W, C, ncls = 3, 40, 56, 24, 5
    rng = np.random.default_rng(12)

    def batch():
        boxes, labs = [], []
        for b in range(B):
            for i in range(12):
                y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 6))
                y1, x1 = y0 + int(rng.integers(1, 6)), x0 + int(rng.integers(2, 12))
                boxes.append((b, y0, y1, x0, x1, len(boxes) if dense else int(rng.integers(0, C))))
                labs.append((b, y0, y1, x0, x1, int(rng.integers(1, ncls))))
        boxes, labs = np.asarray(boxes, np.int32), np.asarray(labs, np.int32)
        feats = rng.standard_normal((len(boxes), C)).astype(np.float32) if dense else None
        return boxes, labs, feats
    batches = [batch() for _ in range(5)]
    kw = dict(scale_space_num=3, res_depth=2, featRoot=8, final_act="softmax", num_blocks=2, dtype="bf16", seed=4, deterministic=True)
    res = {}
    for mode in ("prefetch", "plain"):
        m = MSAUWrapper(C, ncls, kw).cuda()
        eng = TrainEngine(m)
        losses = []
        if mode == "plain":
            for bx, lb, ft in batches:
                losses.append(float(eng.step_boxes(bx, lb, B, H, W, feats=ft)))
        else:
            eng.prefetch_boxes(batches[0][0], batches[0][1], B, H, W, feats=batches[0][2])
            for i in range(len(batches)):
                if i + 1 < len(batches):
                    bx, lb, ft = batches[i + 1]
                    eng.prefetch_boxes(bx, lb, B, H, W, feats=ft)
                losses.append(float(eng.step_prefetched()))
            plan = m._plan_for_shape(B, H, W, torch.device("cuda", 0), True)
            assert plan.input_buffer(0).data_ptr() != plan.input_buffer(1).data_ptr()
        torch.cuda.synchronize()
        res[mode] = (losses, eng.flat_grad.clone(), m.flat_parameters.clone())
    assert res["prefetch"][0] == res["plain"][0], (res["prefetch"][0], res["plain"][0])
    assert torch.equal(res["prefetch"][1], res["plain"][1]) and torch.equal(res["prefetch"][2], res["plain"][2])


@pytest.mark.parametrize("dtype,C", [("fp32", 24), ("bf16", 24), ("bf16", 33), ("bf16", 100)])     # 33: roundup(C, 32) > max(C, 32) -- the workspace
def test_first_conv_fed_with_box_lists_matches_the_painted_grid(dtype, C, monkeypatch):
    """MSAU_CONV_OWNER (csrc/ownerconv.hip): TrainEngine.step_boxes with a feature table never paints the embedding grid -- the
    first conv gathers per-tap partial products T[feature row][tap][co], its weight gradient sums the output gradient per box
    and tap -- against the same steps on the painted tensor (MSAU_OWNER_CONV=0).  Same rounded operands, fp32 sums in another
    order: losses, the first conv's weight and bias gradient, the whole gradient and the updated parameters agree to rounding.
    Overlapping boxes (the last one painted owns the pixel), boxes over the edge, an empty sample, a feature row used twice."""
    torch.manual_seed(3)
    B, H, W, ncls = 4, 40, 56, 5
    rng = np.random.default_rng(21)
    boxes, labs = [], []
    for b in range(B - 1):                                  # the last sample stays empty
        for i in range(16):
            y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 6))
            y1, x1 = y0 + int(rng.integers(1, 6)), x0 + int(rng.integers(2, 14))
            boxes.append((b, y0, y1, x0, x1, len(boxes) if i else 0))          # feature row 0 is shared by three boxes
            labs.append((b, y0, y1, x0, x1, int(rng.integers(1, ncls))))
    boxes, labs = np.asarray(boxes, np.int32), np.asarray(labs, np.int32)
    feats = rng.standard_normal((len(boxes), C)).astype(np.float32)
    kw = dict(scale_space_num=3, res_depth=2, featRoot=8, final_act="softmax", num_blocks=2, dtype=dtype, seed=4, deterministic=True)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MSAU_OWNER_CONV", mode)
        m = MSAUWrapper(C, ncls, kw).cuda()
        eng = TrainEngine(m)
        losses = [float(eng.step_boxes(boxes, labs, B, H, W, feats=feats)) for _ in range(3)]
        torch.cuda.synchronize()
        plan = m._plan_for_shape(B, H, W, torch.device("cuda", 0), True)
        assert (getattr(plan, "_owner_keep", None) is not None) == (mode == "1")
        c = next(op for op in plan.ops if getattr(op, "x1", None) is plan.x_in)
        wo, bo, n = plan.poff[c.wname], plan.poff[c.bname], int(np.prod(plan.pshape[c.wname]))
        g = eng.flat_grad.float().cpu()
        res[mode] = (losses, g, m.flat_parameters.float().cpu(), g[wo:wo + n].clone(), g[bo:bo + 8].clone())
    # (third step: Adam's first updates are lr * sign(g), so entries whose gradient is rounding noise take different signs on the two
    #  paths and the trajectories part at the 1e-4 level even in fp32)
    tol = 2e-2 if dtype == "bf16" else 1e-3
    for a, b in zip(res["1"][0], res["0"][0]):
        assert abs(a - b) < (2e-3 if dtype == "bf16" else 1e-5) * abs(b), (res["1"][0], res["0"][0])
    assert float(res["0"][3].abs().max()) > 0 and err(res["1"][3], res["0"][3], True) < tol
    assert float(res["0"][4].abs().max()) > 0 and err(res["1"][4], res["0"][4], True) < tol
    assert err(res["1"][1], res["0"][1], True) < tol
    assert err(res["1"][2], res["0"][2], True) < (1e-3 if dtype == "bf16" else 1e-5)
    # and a step on a painted tensor afterwards goes back to the tensor-fed launches
    monkeypatch.setenv("MSAU_OWNER_CONV", "1")
    x = torch.randn(B, C, H, W, device="cuda")
    lab = torch.randint(0, ncls, (B, H, W), device="cuda")
    l0 = float(eng.step(x, lab))
    assert np.isfinite(l0)


def _paint_dense_cpu(boxes, feats, B, H, W):
    """CPU painter of a box list, as data_generator_funsd_bert.py:64-93 leaves the grid: boxes in order, later ones overwrite,
    numpy slicing clips at the edge; value = row of the feature table"""
    C = feats.shape[1]
    grid = np.zeros((B, C, H, W), np.float32)
    for b, y0, y1, x0, x1, v in boxes:
        grid[b, :, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = feats[v][:, None, None]
    return grid


def _paint_labels_cpu(labs, B, H, W):
    lab = np.zeros((B, H, W), np.int64)
    for b, y0, y1, x0, x1, v in labs:
        lab[b, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = v
    return lab


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_box_list_fed_step_at_the_size_of_baseline_config_4_vs_oracle(dtype):
    """BASELINE configs[3] at its own size through the path that carries its headline number: 768 embedding channels (12 chunks
    of 64), 336x256, 2 stages, TrainEngine.step_boxes with a feature table (MSAU_CONV_OWNER: the grid is never painted) --
    against the CPU oracle's forward + loss + backward on the grid a CPU painter paints from the same boxes
    (data_generator_funsd_bert.py:64-93,240): the loss, the first conv's weight and bias gradient, every other parameter
    gradient.  Text-line-like boxes, some overlapping, some over the edge, one sample nearly empty."""
    from oracle import msau_oracle as O
    B, H, W, C, ncls, stages = 2, 336, 256, 768, 5, 2
    rng = np.random.default_rng(44)
    boxes, labs = [], []
    for b, nlines in ((0, 70), (1, 3)):
        for i in range(nlines):
            h = int(rng.integers(2, 7)); w = int(rng.integers(12, 120))
            y0 = int(rng.integers(-2, H - 2)); x0 = int(rng.integers(-6, W - 8))
            boxes.append((b, y0, y0 + h, x0, x0 + w, len(boxes)))
            labs.append((b, y0, y0 + h, x0, x0 + w, int(rng.integers(1, ncls))))
    boxes, labs = np.asarray(boxes, np.int32), np.asarray(labs, np.int32)
    feats = rng.standard_normal((len(boxes), C)).astype(np.float32)
    if dtype == "bf16":
        feats = torch.from_numpy(feats).bfloat16().float().numpy()          # bf16-representable: both sides see the same inputs
    cfg = dict(O.DEFAULT_CFG, channels=C, num_blocks=stages)
    sd = O.init_params(cfg, seed=45)
    kw = dict(scale_space_num=4, res_depth=2, featRoot=8, final_act="softmax", num_blocks=stages, dtype=dtype)
    m = MSAUWrapper(C, ncls, kw)
    m.load_state_dict(sd)
    m = m.cuda()
    eng = TrainEngine(m)
    loss = eng.step_boxes(boxes, labs, B, H, W, feats=feats)
    torch.cuda.synchronize()
    plan = m._plan_for_shape(B, H, W, torch.device("cuda", 0), True)
    assert getattr(plan, "_owner_keep", None) is not None, "the box-list path did not take the first conv"
    # the checker
    x = torch.from_numpy(_paint_dense_cpu(boxes, feats, B, H, W))
    label = torch.from_numpy(_paint_labels_cpu(labs, B, H, W))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lr, ar = O.msau_forward(leaves, x, cfg)
    ref_loss = O.msau_loss(lr, ar, label)
    ref_loss.backward()
    # (bf16: the gradient that reaches the first conv has come back through ~40 bf16 layers -- the bound is the network's, as for every other
    #  parameter; the fp32 case is what pins the box-list arithmetic itself)
    ltol, gtol, ftol = (1e-4, 3e-3, 2e-3) if dtype == "fp32" else (3e-2, 1e-1, 1e-1)
    assert abs(float(loss) - float(ref_loss)) < ltol * abs(float(ref_loss)), (float(loss), float(ref_loss))
    c = next(op for op in plan.ops if getattr(op, "x1", None) is plan.x_in)
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in leaves.values() if p.grad is not None)))
    for k, off in m._poff.items():
        ref = leaves[k].grad
        got = eng.flat_grad[off:off + leaves[k].numel()].view(leaves[k].shape).float().cpu()
        if ref is None:
            assert float(got.abs().max()) == 0.0, k
            continue
        tol = ftol if k in (c.wname, c.bname) else gtol
        if dtype == "bf16" and (".attention_block.f." in k or ".attention_block.g." in k):
            # the score projections' gradients are differences of nearly equal softmax-weighted sums (shift invariance): with two
            # samples, one of them nearly empty, bf16 rounding noise anywhere upstream moves them most -- 0.08-0.12 observed across
            # this round's (bit-exact or <= 1 ulp) kernel changes, against 0.02-0.05 for every other tensor
            tol = 2e-1
        if float(ref.norm()) > 1e-4 * gn:
            assert err(got, ref, True) < tol, (k, err(got, ref, True))
    assert abs(float(eng.grad_norm) - gn) < (2e-3 if dtype == "fp32" else 3e-2) * gn


@pytest.mark.gpu
def test_fork_events_without_the_system_fence_give_the_same_bits(tmp_path):
    """csrc/sequence.hip creates the FORK events (main -> side) with hipEventDisableSystemFence.  One cold
    training step of the cfg-2 golden net per FRESH process (tools/det_check.py: exact fingerprints of every activation and
    gradient): two processes with the flag, one with HIP's default events (MSAU_EVENT_FENCE=1) -- one bit pattern."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for i, fence in enumerate(("0", "1", "0")):
        out = str(tmp_path / f"r{i}.pt")
        env = dict(os.environ, MSAU_EVENT_FENCE=fence)
        subprocess.run([sys.executable, os.path.join(root, "tools", "det_check.py"), "run", out], env=env, check=True, cwd=root,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        outs.append(torch.load(out))
    keys = list(outs[0])
    assert len(keys) > 100 and set(keys) == set(outs[1]) == set(outs[2])
    for d in outs[1:]:
        bad = [k for k in keys if not torch.equal(outs[0][k], d[k])]
        assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("words,iters", [(16 * 1024, 3000), (1 << 20, 1500), (11 * (1 << 20), 400), (64 * (1 << 20), 60)])
def test_fork_without_the_system_fence_shows_the_producers_writes_to_the_other_queue(words, iters):
    """What the fence-less FORK events of msau_run_ops_overlap rest on (round-4 advice: "add a stress test with producer / consumer on
    different queues checking DATA, not just determinism").  A kernel on the main stream rewrites a buffer (64 KB: resident in every
    L2 .. 256 MB: beyond the Infinity Cache; 44 MB: a level-0 activation), a hipEventDisableSystemFence event forks, a kernel on a
    stream that provably runs on ANOTHER hardware queue (_lib.concurrent_stream) counts the words that do not hold the new pattern,
    with another thread -> word mapping than the producer's -- the previous round's consumer has left the OLD pattern in the L2s of the
    XCDs it ran on.  Any stale read is a non-zero count.  The same loop with default events is the control."""
    from msau_amd import _lib as L
    import ctypes as C
    dev = torch.device("cuda", 0)
    main = torch.cuda.current_stream(dev)
    side = L.concurrent_stream(dev)
    assert side is not None and side.cuda_stream != main.cuda_stream
    for fence in (0, 1):
        bad = C.c_int64(-1)
        L.call("msau_fork_visibility_check", main.cuda_stream, side.cuda_stream, iters, words, fence, C.byref(bad))
        assert bad.value == 0, (fence, words, bad.value)
