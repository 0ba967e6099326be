"""CPU: ragged batches from box lists -- `msau_amd.data.ragged.pack_boxes`, the painting rule of a ragged canvas ("clip to the
document, last box wins") against every document painted alone by the CPU painters, and the host-side checks of
`TrainEngine.step_boxes(..., sizes=)` / `step_ids(..., sizes=)` that need no device."""
import numpy as np
import pytest
import torch

from msau_amd import MSAUWrapper, TrainEngine
from msau_amd.data.ragged import pack, pack_boxes
from msau_amd.data.raster import document_boxes, document_line_boxes

from . import ragged_boxes_util as U


def _doc(rng, h, w, n, C=None, cross=False):
    fb, lb = [], []
    for i in range(n):
        y0, x0 = int(rng.integers(-2 if cross else 0, h)), int(rng.integers(-3 if cross else 0, w))
        y1, x1 = y0 + int(rng.integers(1, 7)), x0 + int(rng.integers(2, 12))
        fb.append((7, y0, y1, x0, x1, i))                      # (the sample column is rewritten by pack_boxes)
        lb.append((7, y0, y1, x0, x1, int(rng.integers(1, 5))))
    fb, lb = np.asarray(fb, np.int32).reshape(-1, 6), np.asarray(lb, np.int32).reshape(-1, 6)
    if C is None:
        return fb, lb, h, w
    return fb, lb, h, w, rng.standard_normal((n, C)).astype(np.float32)


def test_pack_boxes_columns_offsets_tables_sizes_and_canvas():
    rng = np.random.default_rng(0)
    docs = [_doc(rng, 37, 29, 5, 6), _doc(rng, 40, 41, 0, 6), _doc(rng, 21, 33, 7, 6)]
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs, round_to=16)
    assert (H, W) == (48, 48) and sizes.dtype == torch.int64 and sizes.tolist() == [[37, 29], [40, 41], [21, 33]]
    assert pack_boxes(docs, round_to=1)[4] == (40, 41) and pack_boxes(docs, round_to=64)[4] == (64, 64)
    assert gb.dtype == np.int32 and lb.dtype == np.int32 and gb.shape == (12, 6) and lb.shape == (12, 6)
    assert gb[:, 0].tolist() == [0] * 5 + [2] * 7 and lb[:, 0].tolist() == [0] * 5 + [2] * 7
    assert gb[:, 5].tolist() == list(range(12))                # rows of document 2 come after the 5 of document 0 (document 1: none)
    assert feats.shape == (12, 6) and np.array_equal(feats, np.concatenate([d[4] for d in docs]))
    # every input box appears once, geometry and label untouched, and its feature row is still its own
    k = 0
    for d in docs:
        for i in range(len(d[0])):
            assert np.array_equal(gb[k, 1:5], d[0][i, 1:5]) and np.array_equal(lb[k, 1:], d[1][i, 1:])
            assert np.array_equal(feats[gb[k, 5]], d[4][d[0][i, 5]])
            k += 1
    assert k == len(gb)
    assert docs[0][0][0, 0] == 7                               # the inputs are not written to
    # the same rounding rule as `pack` on the painted documents
    dense = [{"mask": torch.zeros((1, 6, d[2], d[3])), "label": torch.zeros((1, d[2], d[3]))} for d in docs]
    x, _, s2 = pack(dense, round_to=16)
    assert tuple(x.shape[-2:]) == (H, W) and torch.equal(s2, sizes)
    # without feature tables (one-hot character boxes): values stay what they are, -1 included
    cb = np.asarray([(0, 1, 2, 1, 2, -1), (0, 2, 3, 1, 2, 4)], np.int32)
    g2, l2, f2, _, _ = pack_boxes([(cb, cb, 5, 5), (cb, cb, 6, 4)])
    assert f2 is None and g2[:, 5].tolist() == [-1, 4, -1, 4] and g2[:, 0].tolist() == [0, 0, 1, 1]


def test_pack_boxes_errors():
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="no documents"):
        pack_boxes([])
    with pytest.raises(ValueError, match="round_to"):
        pack_boxes([_doc(rng, 8, 8, 2, 4)], round_to=0)
    with pytest.raises(ValueError, match="channels"):
        pack_boxes([_doc(rng, 8, 8, 2, 4), _doc(rng, 8, 8, 2, 5)])
    with pytest.raises(ValueError, match="either every document"):
        pack_boxes([_doc(rng, 8, 8, 2, 4), _doc(rng, 8, 8, 2)])
    with pytest.raises(ValueError, match="feature row"):
        d = _doc(rng, 8, 8, 2, 4)
        pack_boxes([(d[0], d[1], 8, 8, d[4][:1])])
    with pytest.raises(ValueError, match=r"\[n, 6\]"):
        pack_boxes([(np.zeros((2, 5), np.int32), np.zeros((0, 6), np.int32), 8, 8)])
    with pytest.raises(ValueError, match="size"):
        pack_boxes([(np.zeros((0, 6), np.int32), np.zeros((0, 6), np.int32), 0, 8)])


def test_ragged_painting_rule_equals_each_golden_document_painted_alone(tmp_path):
    """the restatement the GPU tests compare the device painters with, pinned here to the CPU painters (themselves pinned to the
    reference's arrays by tests/test_data_cpu.py): dense (text-line) and one-hot (character) grids of the committed documents, once
    at their own size and once declared SMALLER than their boxes reach, so that boxes cross their document's edge inside the
    canvas -- numpy slicing on the smaller array is the crop of the full painting"""
    docs, n_chars = U.golden_documents(tmp_path)
    assert len(docs) >= 3
    for shrink in ((0, 0), (3, 5)):
        dense_in, char_in, want = [], [], []
        for dense, chars, i in docs:
            fb, lb, h, w = document_line_boxes(dense.inp_list[i])
            cb, clb, hc, wc = document_boxes(chars.inp_list[i])
            feats = np.asarray(dense.inp_list[i]["transformer_feature"], np.float32)
            h2, w2, hc2, wc2 = h - shrink[0], w - shrink[1], hc - shrink[0], wc - shrink[1]
            dense_in.append((fb, lb, h2, w2, feats))
            char_in.append((cb, clb, hc2, wc2))
            a, c = dense[i], chars[i]
            want.append((a["mask"][0, :, :h2, :w2].numpy(), a["label"][0, :h2, :w2].numpy(),
                         c["mask"][0, :, :hc2, :wc2].numpy(), c["label"][0, :hc2, :wc2].numpy()))
        gb, lb, feats, sizes, (H, W) = pack_boxes(dense_in)
        grid, lab = U.dense_ragged(gb, feats, sizes.tolist(), H, W), U.labels_ragged(lb, sizes.tolist(), H, W)
        cgb, clb, none, csizes, (Hc, Wc) = pack_boxes(char_in)
        cgrid, clab = U.onehot_ragged(cgb, csizes.tolist(), Hc, Wc, n_chars), U.labels_ragged(clb, csizes.tolist(), Hc, Wc)
        assert none is None
        crossing = 0
        for b, (m, l, cm, cl) in enumerate(want):
            for got, glab, wm, wl, (h, w) in ((grid, lab, m, l, sizes[b].tolist()), (cgrid, clab, cm, cl, csizes[b].tolist())):
                canvas = np.zeros((wm.shape[0],) + got.shape[1:3], np.float32)      # the document at the origin of a zero canvas
                canvas[:, :h, :w] = wm
                lcanvas = np.zeros(got.shape[1:3], np.int64)
                lcanvas[:h, :w] = wl
                assert np.array_equal(got[b].transpose(2, 0, 1), canvas), (shrink, b)
                assert np.array_equal(glab[b], lcanvas), (shrink, b)
            h, w = sizes[b].tolist()
            mine = gb[gb[:, 0] == b]
            crossing += int(((mine[:, 2] > h) | (mine[:, 4] > w)).sum())
        assert (crossing > 0) == (shrink != (0, 0)), crossing


def test_ragged_painting_rule_on_synthetic_boxes_over_the_edge():
    """boxes starting at negative coordinates, running over their document's right / bottom edge (inside the canvas) and lying wholly
    between the document and the canvas edge, an empty document, overlaps: per document, numpy slicing on its own array"""
    rng = np.random.default_rng(5)
    docs = [_doc(rng, 37, 29, 14, 5, cross=True), _doc(rng, 40, 40, 0, 5), _doc(rng, 21, 33, 14, 5, cross=True)]
    extra = np.asarray([(0, 5, 9, 30, 44, 0), (0, 38, 46, 2, 9, 1)], np.int32)      # wholly outside document 0, inside the canvas
    docs[0] = (np.concatenate([docs[0][0], extra]), np.concatenate([docs[0][1], extra]), 37, 29, docs[0][4])
    gb, lb, feats, sizes, (H, W) = pack_boxes(docs)
    assert (H, W) == (48, 48)
    grid, lab, owner = U.dense_ragged(gb, feats, sizes.tolist(), H, W), U.labels_ragged(lb, sizes.tolist(), H, W), U.owner_ragged(gb, sizes.tolist(), H, W)
    for b, d in enumerate(docs):
        h, w = d[2], d[3]
        alone, lalone = np.zeros((5, h, w), np.float32), np.zeros((h, w), np.int64)
        for (_, y0, y1, x0, x1, v), (_, _, _, _, _, lv) in zip(d[0].tolist(), d[1].tolist()):
            alone[:, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = d[4][v][:, None, None]
            lalone[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = lv
        assert np.array_equal(grid[b, :h, :w].transpose(2, 0, 1), alone) and np.array_equal(lab[b, :h, :w], lalone)
        assert not grid[b, h:].any() and not grid[b, :, w:].any() and not lab[b, h:].any() and not lab[b, :, w:].any()
        assert (owner[b, h:] == -1).all() and (owner[b, :, w:] == -1).all()
    assert (owner[1] == -1).all() and (owner[0] >= 0).any()


def test_sizes_are_checked_on_the_host_before_any_launch():
    m = MSAUWrapper(13, 5, dict(scale_space_num=3, res_depth=1, featRoot=8, num_blocks=2))
    eng = TrainEngine.__new__(TrainEngine)                     # (the constructor wants the model on a GPU; these checks do not)
    eng.model, eng.use_graph = m, False
    none = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError, match=r"1 <= h <= 16 and 1 <= w <= 32"):
        eng.step_boxes(none, none, 2, 16, 32, sizes=[[17, 3], [1, 1]])
    with pytest.raises(ValueError, match=r"shape \(2, 2\)"):
        eng.step_boxes(none, none, 2, 16, 32, sizes=[[3, 3]])
    with pytest.raises(ValueError, match="CPU integer tensor"):
        eng.step_boxes(none, none, 2, 16, 32, sizes=torch.ones((2, 2)))
    ids, lab = torch.zeros((2, 16, 32), dtype=torch.int32), torch.zeros((2, 16, 32))
    with pytest.raises(ValueError, match=r"1 <= h <= 16 and 1 <= w <= 32"):
        eng.step_ids(ids, lab, sizes=[[16, 33], [1, 1]])
    with pytest.raises(ValueError, match=r"1 <= h <= 16"):
        eng.step_ids(ids, lab, sizes=[[0, 3], [1, 1]])
    with pytest.raises(NotImplementedError, match="dense batches only"):
        eng.prefetch_boxes(none, none, 2, 16, 32, sizes=[[1, 1], [1, 1]])
    eng.use_graph = True
    with pytest.raises(RuntimeError, match="use_graph=False"):
        eng.step_boxes(none, none, 2, 16, 32, sizes=[[3, 3], [1, 1]])
    with pytest.raises(ValueError, match=r"1 <= h <= 16"):
        m.confusion_matrix_boxes(none, none, 2, 16, 32, sizes=[[17, 3], [1, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.confusion_matrix_boxes(none, none, 2, 16, 32, sizes=[[3, 3], [1, 1]])


def test_eager_entry_points_refuse_a_graph_engine_under_their_own_name_before_anything_else():
    """every argument below fails at whatever looks at it, and the engine has no attribute but `model` and `use_graph`: the refusal
    comes first"""
    m = MSAUWrapper(13, 5, dict(scale_space_num=3, res_depth=1, featRoot=8, num_blocks=2))
    eng = TrainEngine.__new__(TrainEngine)
    eng.model, eng.use_graph = m, True
    cpu = torch.zeros((2, 16, 32))
    calls = dict(step_ids=lambda: eng.step_ids(None, cpu, sizes=[[17, 3]]),
                 step_unet=lambda: eng.step_unet(None, cpu, cpu, class_weights=[1.0]),
                 step_kv=lambda: eng.step_kv(None),
                 step_nhwc=lambda: eng.step_nhwc(None, cpu),
                 step_boxes=lambda: eng.step_boxes(None, None, 2, 16, 32),
                 prefetch_boxes=lambda: eng.prefetch_boxes(None, None, 2, 16, 32))
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=rf"^{name} is an eager path \(use_graph=False\)"):
            call()
    with pytest.raises(RuntimeError, match=r"^step_boxes is an eager path \(use_graph=False\)"):
        eng.step_boxes(None, None, 2, 16, 32, feats=None, sizes=[[17, 3], [1, 1]])


@pytest.mark.parametrize("dtype_name,channels", [("fp32", 13), ("bf16", 24), ("bf16", 768)])
def test_a_ragged_plan_gets_the_box_list_instance_of_its_first_conv(dtype_name, channels):
    """plans build without a device: the first conv of a ragged plan carries MSAU_CONV_EXTENT, and the box-list instance takes it
    (msau_conv2d_launch_info bits 5 and 7 with MSAU_CONV_OWNER added), for training and forward-only plans"""
    import ctypes as C
    from msau_amd import _lib as L
    m = MSAUWrapper(channels, 5, dict(scale_space_num=4, res_depth=2, featRoot=8, num_blocks=3, dtype=dtype_name, seed=0))
    for training in (True, False):
        plan = m._plan_for_shape(3, 48, 48, torch.device("cpu"), training, ragged=True)
        assert plan._feed_owner(None) and plan._owner_conv is not None and plan._owner_keep is None
        d = L.ConvDesc.from_buffer_copy(plan._owner_conv.fdesc)
        assert d.flags & L.CONV_EXTENT and d.extent
        d.flags |= L.CONV_OWNER
        info = (L.i32 * 8)()
        L.call("msau_conv2d_launch_info", plan.dtype, C.byref(d), info)
        assert info[7] & 32 and info[7] & 128, list(info)
        d.flags |= L.CONV_RELU_IN                               # a flag the instance does not implement: refused, with or without extents
        L.call("msau_conv2d_launch_info", plan.dtype, C.byref(d), info)
        assert not info[7] & 128, list(info)
