"""A confidence per region on the device: `regions_device(..., probs=)` (csrc/regions.hip, `msau_kv_regions_scored` and
`msau_kv_regions_large_scored`) against `regions_host(..., probs=)`, integers exact, its tables against the unscored call's,
`MSAUWrapper.predict_regions(scores=True)` on the probabilities the head wrote, and KVModel's `confidence=True` on its three paths.
No tolerances: every compared quantity is an integer or a float64 computed on the host from integers."""
import json
import os

import numpy as np
import pytest
import torch

from msau_amd.inference import KVModel
from msau_amd.inference import regions as R
from oracle import msau_oracle as O
from tests import regions_util as U
from tests.regions_large_util import large_cases
from tests.regions_scored_util import doc_probs, full_doc, pack_probs, scored_cases

pytestmark = pytest.mark.gpu
KV = U.KV


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _device(docs, probs, n_class, ragged, large=False, outside=None, seed=0):
    """the documents as one batch through the scored and the unscored kernel -> ((tables, flags, scores), (tables, flags))"""
    am, lm, cm, sizes = U.pack_canvas(docs, n_class, seed=seed, round_to=16 if ragged else 1, neighbours=ragged)
    pr = torch.from_numpy(pack_probs(probs, am.shape, n_class, outside, seed=seed)).cuda()
    args = (torch.from_numpy(am).cuda(), _dev16(lm), _dev16(cm), [d[3] for d in docs], n_class)
    kw = dict(sizes=sizes if ragged else None, large=large)
    return R.regions_device(*args, probs=pr, **kw), R.regions_device(*args, **kw)


def _check(docs, probs, n_class, ragged, **kw):
    want = [R.regions_host(*d, n_class, probs=p) for d, p in zip(docs, probs)]
    lim = R.device_limits()
    for (table, _), d in zip(want, docs):                                 # a refusal cannot hide a wrong sum
        nr, nr_class, npair, npair_class = U.counts(table)
        assert nr <= R.DEFAULT_CAP_REGIONS and nr_class <= lim["max_regions_per_class"]
        assert npair <= R.DEFAULT_CAP_PAIRS and npair_class <= lim["max_pairs_per_class"]
    (tables, flags, scores), (tables0, flags0) = _device(docs, probs, n_class, ragged, **kw)
    assert flags == [0] * len(docs) == flags0
    assert tables == tables0 == [w[0] for w in want]
    assert scores == [w[1] for w in want]
    assert all(isinstance(v, int) for s in scores for c in s.values() for v in c)
    return scores


def test_scored_device_equals_host_statement_on_small_cases():
    lim = R.device_limits()
    cases = [c for c in scored_cases(lim["max_pixels"]) if c[0] != "pixel_limit"]
    assert {"spiral", "comb", "blocky", "ties", "n_class_40", "thin_1x9", "empty"} <= {c[0] for c in cases}
    before = dict(R.STATS)
    for name, doc, n_class, pr in cases:
        _check([doc], [pr], n_class, ragged=False)
    assert R.STATS["calls"] == before["calls"] + 2 * len(cases) and R.STATS["d2h_bytes"] > before["d2h_bytes"]


def test_scored_device_saturation_at_the_pixel_limit():
    lim = R.device_limits()
    doc, pr = full_doc(lim["max_pixels"] // 192, 192)
    assert doc[0].size == lim["max_pixels"]
    scores = _check([doc], [pr], 3, ragged=False)
    assert scores[0][2] == [(lim["max_pixels"] // 192) * 190 * 65536]


def test_scored_device_ragged_batch_of_three_with_neighbours():
    cases = {c[0]: c for c in scored_cases(R.device_limits()["max_pixels"])}
    docs = [cases[n][1] for n in ("blocky", "single_pixels", "four_borders")]
    rng = np.random.default_rng(60)
    probs = [doc_probs(rng, d[0], 6) for d in docs]
    _check(docs, probs, 6, ragged=True, seed=1)                           # random classes and probabilities up to every extent
    _check(docs, probs, 6, ragged=True, outside=1.0)                      # p = 1 for every class outside the documents


def test_scored_device_large_form():
    doc, pr = full_doc(260, 260)
    before = R.STATS["large_documents"]
    scores = _check([doc], [pr], 3, ragged=False, large=True)
    assert scores[0][2] == [67080 * 65536] and scores[0][2][0] > 2 ** 32
    assert R.STATS["large_documents"] == before + 2
    _, doc, n_class = next(c for c in large_cases() if c[0] == "257x191")
    pr = doc_probs(np.random.default_rng(61), doc[0], n_class)
    _check([doc], [pr], n_class, ragged=True, large=True, outside=1.0)


def test_scored_device_consecutive_calls_on_the_cached_buffers():
    rng = np.random.default_rng(62)
    many = U.with_lines(U.blocky_map(rng, 48, 72, 6, flip=0.3), 63)
    few = U.with_lines(U.blocky_map(rng, 48, 72, 6, flip=0.0), 64)
    p_many, p_few = doc_probs(rng, many[0], 6), doc_probs(rng, few[0], 6)
    assert U.counts(R.regions_host(*many, 6))[0] > 4 * U.counts(R.regions_host(*few, 6))[0] > 0
    R._buffers.clear()
    _check([many], [p_many], 6, ragged=False)
    assert sorted(len(k) for k in R._buffers) == [5, 6] and any(k[-1] == "scored" for k in R._buffers)
    _check([few], [p_few], 6, ragged=False)                               # same shapes: the same cached buffers
    assert len(R._buffers) == 2
    # a flagged document has no scores, the other documents of the batch have theirs
    lim = R.device_limits()
    big = U.with_lines(U.blocky_map(rng, 130, 192, 6), 65)
    assert big[0].size > lim["max_pixels"]
    (tables, flags, scores), _ = _device([few, big], [p_few, doc_probs(rng, big[0], 6)], 6, ragged=True)
    assert flags == [0, R.OVF_PIXELS] and tables[1] is None and scores[1] is None
    assert scores[0] == R.regions_host(*few, 6, probs=p_few)[1]
    with pytest.raises(ValueError):
        R.regions_device(torch.zeros((1, 16, 16), dtype=torch.uint8).cuda(), _dev16(np.zeros((1, 16, 16), np.uint16)),
                         _dev16(np.zeros((1, 16, 16), np.uint16)), [[]], 6, probs=torch.zeros((1, 16, 16, 5)).cuda())


# ---- the network's own probabilities ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def km(tmp_path_factory):
    meta = json.load(open(os.path.join(KV, "kv.json")))
    cfg, seed = meta["net"]["cfg"], meta["net"]["seed"]
    wpath = str(tmp_path_factory.mktemp("kv_scored") / "kv_weights.pt")
    torch.save(O.init_params(cfg, seed), wpath)
    km = KVModel()
    km.load(model_weight=wpath, charset=os.path.join(KV, "charset.txt"), n_class=meta["n_class"], dtype="fp32",
            model_kwargs=dict(featRoot=cfg["featRoot"], scale_space_num=cfg["scale_space_num"], res_depth=cfg["res_depth"],
                              filter_size=cfg["filter_size"], pool_size=cfg["pool_size"], final_act="softmax"))
    return km


FILES = [os.path.join(KV, f"layout{i}.json") for i in range(3)]


def test_predict_regions_scores_equal_host_on_the_heads_outputs(km):
    from msau_amd.data.ragged import pack_ids, pack_masks
    masks = [km._generate_masks_from_label(f) for f in FILES]
    boxes = [[l["box"] for l in m[3]] for m in masks]
    ids, sizes = pack_ids([m[0] for m in masks])
    line_ids, _ = pack_masks([m[1] for m in masks])
    char_pos, _ = pack_masks([m[2] for m in masks])
    kw = dict(ids=ids.cuda(), sizes=sizes, line_ids=line_ids, char_pos=char_pos, boxes=boxes)
    tables, flags, amax, scores = km.net.predict_regions(scores=True, **kw)
    assert flags == [0, 0, 0] and km.net.last_head_probs.dtype == torch.float32
    probs, cls = km.net.last_head_probs.cpu().numpy(), amax.cpu().numpy()
    assert tuple(probs.shape) == tuple(cls.shape) + (km.n_class,)
    n_regions = 0
    for b, m in enumerate(masks):
        h, w = m[0].shape
        want = R.regions_host(cls[b, :h, :w], m[1], m[2], boxes[b], km.n_class, probs=np.ascontiguousarray(probs[b, :h, :w]))
        assert tables[b] == want[0] and scores[b] == want[1]
        n_regions += U.counts(want[0])[0]
    assert n_regions > 500                                               # a random-weight net: a speckled class map
    plain = km.net.predict_regions(**kw)
    assert len(plain) == 3 and plain[0] == tables and plain[1] == flags


def _paths(km, confidence, **kw):
    return {"host": km.predict_batch(FILES, confidence=confidence, **kw),
            "device_post": km.predict_batch(FILES, device_post=True, confidence=confidence, **kw),
            "device_masks": km.predict_batch(FILES, device_post=True, device_masks=True, confidence=confidence, **kw)}


def _assert_scored_results(scored, plain):
    assert scored["host"] == scored["device_post"] == scored["device_masks"]
    assert plain["host"] == plain["device_post"] == plain["device_masks"]
    found = 0
    for doc, doc_plain in zip(scored["host"], plain["host"]):
        assert list(doc) == list(doc_plain) and {k: v["text"] for k, v in doc.items()} == doc_plain
        for v in doc.values():
            assert set(v) == {"text", "confidence"}
            assert v["confidence"] is None or (isinstance(v["confidence"], float) and 0.0 < v["confidence"] <= 1.0)
            assert v["confidence"] is not None or v["text"] == ""
            found += v["confidence"] is not None
    assert found > 0


def test_kvmodel_confidence_is_the_same_on_the_three_paths(km, tmp_path, capsys):
    for k in R.STATS:
        R.STATS[k] = 0
    scored, plain = _paths(km, True), _paths(km, False)
    assert R.STATS["fallbacks"] == 0 and R.STATS["calls"] == 4
    _assert_scored_results(scored, plain)
    # one document at a time, and run_test: results with confidence, counts and printing of counts as without
    for f in FILES[:2]:
        single = [km.predict((f, None), confidence=True, **kw)[0]
                  for kw in ({}, dict(device_post=True), dict(device_post=True, device_masks=True))]
        assert single[0] == single[1] == single[2]
        assert {k: v["text"] for k, v in single[0].items()} == km.predict((f, None))[0]
    labels = tmp_path / "labels"
    labels.mkdir()
    (labels / "layout0.json").write_text(open(FILES[0]).read())
    runs = {}
    for conf in (False, True):
        capsys.readouterr()
        res = km.run_test(FILES, str(tmp_path), label_dir=str(labels), batch_size=3, device_post=True, confidence=conf)
        printed = capsys.readouterr().out
        runs[conf] = (res, json.loads(json.dumps(km.eval_results)), [ln for ln in printed.splitlines() if not ln.startswith("{")])
    assert runs[True][0] == scored["device_post"] and runs[False][0] == plain["device_post"]
    assert runs[True][1:] == runs[False][1:]


def test_kvmodel_confidence_falls_back_exactly(km, monkeypatch):
    """lists far too short for the net's class maps: every document overflows and is redone on the host from its crop of the
    probabilities: the same floats"""
    want = km.predict_batch(FILES, confidence=True)
    monkeypatch.setattr(R, "DEFAULT_CAP_REGIONS", 8)
    for k in R.STATS:
        R.STATS[k] = 0
    got = km.predict_batch(FILES, device_post=True, confidence=True)
    sizes = [km._generate_masks_from_label(f)[0].shape for f in FILES]
    assert R.STATS["fallbacks"] == 3 and got == want
    assert R.STATS["d2h_bytes"] >= sum(h * w * (1 + 4 * km.n_class) for h, w in sizes)      # class map and probabilities, per crop
