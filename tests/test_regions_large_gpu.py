"""The large form of the region kernel on the device (`regions_device(large=True)`, csrc/regions.hip `msau_kv_regions_large`)
against `regions_host`, integer for integer, on documents of more pixels than the LDS form holds, and KVModel's
`large_documents=True` against its host fallback.  Before a comparison every test asserts, from scipy's own counts, that the
document is over the pixel limit and fits the per-class limits and the capacities it passes: a fallback cannot hide a wrong
table."""
import json
import os

import numpy as np
import pytest
import torch

from msau_amd.inference import KVModel
from msau_amd.inference import glyphs as G
from msau_amd.inference import regions as R
from oracle import msau_oracle as O
from tests import glyphs_util as GU
from tests import regions_util as U
from tests.regions_large_util import large_cases

pytestmark = pytest.mark.gpu
KV = U.KV


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _device(docs, n_class, ragged, large=True, cap_regions=None, cap_pairs=None, seed=0):
    am, lm, cm, sizes = U.pack_canvas(docs, n_class, seed=seed, round_to=16 if ragged else 1, neighbours=ragged)
    if not ragged:
        assert all(d[0].shape == am.shape[1:] for d in docs)
    return R.regions_device(torch.from_numpy(am).cuda(), _dev16(lm), _dev16(cm), [d[3] for d in docs], n_class,
                            sizes=sizes if ragged else None, cap_regions=cap_regions, cap_pairs=cap_pairs, large=large)


def _assert_large_fits(want, doc, cap_regions=None, cap_pairs=None):
    lim = R.device_limits()
    nr, nr_class, npair, npair_class = U.counts(want)
    assert doc[0].size > lim["max_pixels"]
    assert nr <= (cap_regions or R.DEFAULT_CAP_REGIONS) and nr_class <= lim["max_regions_per_class"], (nr, nr_class)
    assert npair <= (cap_pairs or R.DEFAULT_CAP_PAIRS) and npair_class <= lim["max_pairs_per_class"], (npair, npair_class)
    assert all(0 <= int(v) <= len(doc[3]) for v in np.unique(doc[1]))


@pytest.fixture(scope="module")
def cases():
    """[(name, document, n_class, table of regions_host)]: computed once, read only"""
    out = []
    for name, doc, n_class in large_cases():
        want = R.regions_host(*doc, n_class)
        _assert_large_fits(want, doc)
        out.append((name, doc, n_class, want))
    return out


@pytest.fixture(scope="module")
def gold():
    return U.load_gold()


def test_large_documents_dense(cases):
    before = R.STATS["large_documents"]
    for name, doc, n_class, want in cases:
        got, flags = _device([doc], n_class, ragged=False)
        assert flags == [0], (name, flags)
        assert got[0] == want, name
    assert R.STATS["large_documents"] == before + len(cases)


def test_large_documents_ragged(cases):
    for name, doc, n_class, want in cases:
        got, flags = _device([doc], n_class, ragged=True, seed=3)          # other classes right up to the extent
        assert flags == [0], (name, flags)
        assert got[0] == want, name
    # groups of large documents of one class count: 17 classes, then 5
    for n_class in (17, 5):
        group = [c for c in cases if c[2] == n_class and not c[0].startswith("thin")]
        assert len(group) >= 2
        got, flags = _device([c[1] for c in group], n_class, ragged=True)
        assert flags == [0] * len(group)
        assert got == [c[3] for c in group]


def test_only_the_large_documents_change_between_large_false_and_true(cases, gold):
    g, meta = gold
    by = {c[0]: c for c in cases}
    small = [U.gold_doc(g, meta, 1)[0], U.with_lines(U.blocky_map(np.random.default_rng(40), 48, 72, 17), 41)]
    docs = [small[0], by["257x191"][1], small[1], by["overflow_test_map"][1]]
    want = [R.regions_host(*small[0], 17), by["257x191"][3], R.regions_host(*small[1], 17), by["overflow_test_map"][3]]
    off, flags_off = _device(docs, 17, ragged=True, large=False)
    assert flags_off == [0, R.OVF_PIXELS, 0, R.OVF_PIXELS] and off[1] is None and off[3] is None
    assert off[0] == want[0] and off[2] == want[2]
    before = R.STATS["large_documents"]
    on, flags_on = _device(docs, 17, ragged=True, large=True)
    assert flags_on == [0] * 4 and on == want
    assert R.STATS["large_documents"] == before + 2
    # a batch without a large document: the keyword changes nothing and launches nothing
    on, flags_on = _device(small, 17, ragged=True, large=True)
    assert flags_on == [0, 0] and on == [want[0], want[2]] and R.STATS["large_documents"] == before + 2


def test_large_overflow_flags(cases):
    _, big, _, want = next(c for c in cases if c[0] == "overflow_test_map")
    lim = R.device_limits()
    nr, _, npair, _ = U.counts(want)
    assert _device([big], 17, ragged=False, cap_regions=nr - 1, cap_pairs=npair)[1] == [R.OVF_REGIONS]
    assert _device([big], 17, ragged=False, cap_regions=nr, cap_pairs=npair - 1)[1] == [R.OVF_PAIRS]
    got, flags = _device([big], 17, ragged=False, cap_regions=nr, cap_pairs=npair)
    assert flags == [0] and got[0] == want
    noise = U.with_lines(np.random.default_rng(6).integers(0, 4, size=(160, 160)), 7)
    assert noise[0].size > lim["max_pixels"] and U.counts(R.regions_host(*noise, 4))[1] > lim["max_regions_per_class"]
    got, flags = _device([noise, big], 17, ragged=True)
    assert flags == [R.OVF_REGIONS, 0] and got[0] is None and got[1] == want
    assert _device([big[:3] + (big[3][:3],)], 17, ragged=False)[1] == [R.OVF_LINES]


def test_large_consecutive_calls_leave_no_state(cases):
    by = {c[0]: c for c in cases}
    a_docs, b_docs = [by["257x191"][1], by["overflow_test_map"][1]], [by["overflow_test_map"][1], by["257x191"][1]]
    a = _device(a_docs, 17, ragged=True)
    R._buffers.clear()
    R._workspaces.clear()
    small = _device([by["300x256"][1]], 5, ragged=False)                  # a smaller workspace first, then one that has to grow
    b = _device(b_docs, 17, ragged=True)
    a2 = _device(a_docs, 17, ragged=True)
    spiral = _device([by["spiral"][1]], 5, ragged=False)                  # one region over labels the last call left behind
    a3 = _device(a_docs, 17, ragged=True)
    assert a == a2 == a3 and a[1] == [0, 0] and a[0] == [by["257x191"][3], by["overflow_test_map"][3]]
    assert b[0] == a[0][::-1] and small[0] == [by["300x256"][3]] and spiral[0] == [by["spiral"][3]]


# ---- end to end ------------------------------------------------------------------------------------------------------------
BIAS_CLASS, BIAS = 3, 6.0        # the seeded net's class map has thousands of regions per class on the big page; with the end
                                 # conv's bias of one field class raised it has a few hundred (asserted below from scipy's counts)


def _kv_model(dtype, tmp_path):
    meta = json.load(open(os.path.join(KV, "kv.json")))
    cfg, seed = meta["net"]["cfg"], meta["net"]["seed"]
    sd = O.init_params(cfg, seed)
    sd[f"msau_net.end_convs.{cfg.get('num_blocks', 3) - 1}.custom_conv.bias"][BIAS_CLASS] += BIAS
    wpath = str(tmp_path / f"kv_weights_{dtype}.pt")
    torch.save(sd, wpath)
    km = KVModel()
    km.load(model_weight=wpath, charset=os.path.join(KV, "charset.txt"), n_class=meta["n_class"], dtype=dtype,
            model_kwargs=dict(featRoot=cfg["featRoot"], scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                              filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax"))
    return km


def _reset():
    for s in (R.STATS, G.STATS):
        for k in s:
            s[k] = 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kvmodel_large_documents_equals_host_fallback(dtype, tmp_path, capsys):
    km = _kv_model(dtype, tmp_path)
    lim = R.device_limits()
    big = GU.write_layout(GU.big_layout(), tmp_path / "big.json")
    gold_files = [os.path.join(KV, f"layout{i}.json") for i in range(3)]
    labels = tmp_path / "labels"
    labels.mkdir()
    for name, src in (("layout0", gold_files[0]), ("layout2", gold_files[2])):
        (labels / f"{name}.json").write_text(open(src).read())
    truth = dict(GU.big_layout(), img_shape=[150, 420])                  # the big page's ground truth: three lines of the raised class
    for line in truth["lines"][:3]:
        line["type"], line["value"] = 1, BIAS_CLASS - 1
    GU.write_layout(truth, labels / "big.json")
    # the big page's own class map fits everything but the pixel limit
    masks = km._generate_masks_from_label(big)
    assert masks[0].size > lim["max_pixels"]
    _a_pred, a_cls = km._run_net(masks[0])
    nr, nr_class, npair, npair_class = U.counts(R.regions_host(a_cls, masks[1], masks[2], [l["box"] for l in masks[3]], km.n_class))
    assert 0 < nr <= R.DEFAULT_CAP_REGIONS // 2 and nr_class <= lim["max_regions_per_class"] // 2, (nr, nr_class)
    assert npair <= R.DEFAULT_CAP_PAIRS // 2 and npair_class <= lim["max_pairs_per_class"] // 2, (npair, npair_class)
    files = [gold_files[0], big, gold_files[1], gold_files[2]]
    many = files + [big]                                                 # batch 4: a group of 4 and a group of 1
    out, stats = {}, {}
    with pytest.raises(ValueError):
        km.predict((big, None), large_documents=True)                    # needs device_post
    for masks_on in (False, True):
        for large in (False, True):
            kw = dict(device_post=True, device_masks=masks_on, large_documents=large)
            _reset()
            res = {"predict": [km.predict((f, None), **kw) for f in (big, gold_files[0])],
                   "predict_batch": km.predict_batch(files, **kw)}
            for bs in (1, 4):
                capsys.readouterr()
                r = km.run_test(many, str(tmp_path), label_dir=str(labels), batch_size=bs, **kw)
                res[f"run_test_{bs}"] = (r, json.loads(json.dumps(km.eval_results)), capsys.readouterr().out)
            out[masks_on, large], stats[masks_on, large] = res, dict(R.STATS)
    # the big page: predict, predict_batch, 2 of run_test at 1 and 2 at 4
    for masks_on in (False, True):
        assert out[masks_on, True] == out[masks_on, False]
        assert stats[masks_on, False]["fallbacks"] == 6 and stats[masks_on, False]["large_documents"] == 0
        assert stats[masks_on, True]["fallbacks"] == 0 and stats[masks_on, True]["large_documents"] == 6
    assert out[True, True] == out[False, True]
    res = out[True, True]
    assert res["predict"][0] == (res["predict_batch"][1], None) and any(v for v in res["predict_batch"][1].values())
    assert "big" in res["run_test_4"][2] and sum(c["num_label"] for c in res["run_test_4"][1]) > 0
